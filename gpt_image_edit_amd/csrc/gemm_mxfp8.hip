// MXFP8 (OCP MX v1.0: e4m3fn elements, one E8M0 scale per 32 consecutive k) path of the block GEMMs -- opt-in, inference only.
//
//   fk_quantize_mxfp8   bf16 rows (fk_rows addressing) -> e4m3 [M, K] + E8M0 [M, K / 32], one pass, one thread per block of 32
//   gemm_mxfp8_kernel   C = epilogue(deq(A) . deq(W)^T + bias) on v_mfma_scale_f32_16x16x128_f8f6f4 (both operands e4m3)
//   gemm_mxq_kernel     the same tile, its bf16-rounded result stored as e4m3 + E8M0 (gemm_epilogue.h: store_tile_mxq): the
//                       producer form for a GEMM whose only consumer is another MXFP8 GEMM (fk_gemm_mxfp8_q)
//   gemm_mxsk_kernel    split-K pairs of the 256 x 256 tile (variant 512): two workgroups per tile, each over half of K, which
//                       meet through the caller's split-K workspace -- the form the bf16 path runs its long-K N = 3072
//                       launches in (gemm_pingpong_bf16.hip: gemm8_kernel<.., SPLITK>), same workspace, same protocol
//
// The GEMM keeps the bf16 kernels' conventions so that their epilogue (gemm_epilogue.h: store_tile) takes its accumulators
// unchanged: operands swapped (W rows -> MFMA src0, activation rows -> src1), 8 waves as 2 (M) x 4 (N), a wave's output the
// 32 x 32 blocks (nf, mf) of CfgMx::tile_row / tile_col, and inside a block the 16 x 16 quad q = 2 * n16 + m16 -- the
// 16 x 16 C/D layout does not depend on the operand type on gfx950, so FragMap<true> describes these accumulators as it
// describes v_mfma_f32_16x16x32_bf16's.
//
// Operand / scale lane maps of the 16 x 16 x 128 form with 8-bit operands (measured on the GPU with random small-integer data
// and random scales against every candidate map; tests/test_hip_mxfp8.py holds the GEMM to exact results on such data): lane l
// holds row (l & 15) of its operand, with g = l >> 4, k = 16 g + j in byte j of registers 0-3 and k = 64 + 16 g + j in byte j
// of registers 4-7 (two 16-byte chunks, g and 4 + g, of a 128-byte K-tile row); byte 0 of its scale register is the E8M0
// scale of block g (k = 32 g .. 32 g + 31) of that row -- NOT the block its own bytes lie in.
//
// Main loop (plain HIP, two LDS stages): a K-tile is 128 k = one MFMA k-step.  Each K-tile's operand rows (128 B) and the
// dword of 4 scale bytes of every row are requested as LDS-DMA pieces one K-tile ahead (fk_common.h: opaque form, counted
// vmcnt, then a barrier); the 16-byte chunk c of row r sits at slot c ^ (r & 7) (swizzle applied on the DMA source address).
#include <stdlib.h>

#include <type_traits>

#include "fk_common.h"

namespace {

#include "gemm_epilogue.h"   // BM, TileRows, row16_sum, xcd_chunk_index, FragMap, store_tile, store_tile_mxq; mxfp8_quant.h

typedef __attribute__((ext_vector_type(8))) int i32x8_t;   // 32 e4m3 bytes: the 16 x 16 x 128 operand of one lane

// ---- quantizer ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void quantize_mxfp8_kernel(const bf16_t* __restrict__ x, fk_rows xr, int64_t M, int K,
                                                             uint8_t* __restrict__ q, int64_t ldq, uint8_t* __restrict__ sc,
                                                             int64_t ld_scale) {
  const int nb = K >> 5;
  const int64_t bi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (bi >= M * nb) return;
  const int64_t m = bi / nb;
  const int j = (int)(bi - m * nb);
  const u32x4_t* src = (const u32x4_t*)(x + fk_row_offset(xr, m) + j * 32);
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const u32x4_t v = src[i];
    w[4 * i] = v[0]; w[4 * i + 1] = v[1]; w[4 * i + 2] = v[2]; w[4 * i + 3] = v[3];
  }
  uint32_t out[8];
  const uint32_t sbyte = mx_quant_block(w, out);
  u32x4_t* dst = (u32x4_t*)(q + m * ldq + j * 32);
  dst[0] = u32x4_t{out[0], out[1], out[2], out[3]};
  dst[1] = u32x4_t{out[4], out[5], out[6], out[7]};
  sc[m * ld_scale + j] = (uint8_t)sbyte;
}

// ---- GEMM ---------------------------------------------------------------------------------------------------------------
template <int BN>
struct CfgMx {
  static_assert(BN == 256 || BN == 128, "256 x 256 and 256 x 128 tiles");
  static constexpr bool M16 = true;
  static constexpr int NTHREADS = 512;
  static constexpr int BK = 128;                       // k per K-tile = bytes of a tile row = one MFMA k-step
  static constexpr int MF = 4, NF = BN / 128;
  static constexpr int A_BYTES = BM * BK, W_BYTES = BN * BK;
  static constexpr int AS_OFF = A_BYTES + W_BYTES;     // dword of 4 scale bytes per row, A rows then W rows
  static constexpr int WS_OFF = AS_OFF + BM * 4;
  static constexpr int STAGE_BYTES = WS_OFF + BN * 4;
  static constexpr int W_PIECES = BN / 64;             // 1 KiB DMA pieces (8 rows) of the W tile per wave
  static constexpr int CT_LD = BN + 8;
  static constexpr int CT_BYTES = BM * CT_LD * 2;
  static constexpr int SMEM_BYTES = 2 * STAGE_BYTES > CT_BYTES ? 2 * STAGE_BYTES : CT_BYTES;
  static FK_DEV int tile_row(int wm, int mf) { return (mf >> 1) * 128 + wm * 64 + (mf & 1) * 32; }
  static FK_DEV int tile_col(int wn, int nf) { return nf * 128 + wn * 32; }
};

struct MxGroup {
  fk_gemm_mxfp8_args p[FK_MAX_GROUP];
  int tiles_before[FK_MAX_GROUP + 1];
  int n;
};
constexpr int MX_GROUP_M = 8;   // depth (row tiles) of the grouped tile order

template <int N>
FK_DEV void wait_vm() {
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else static_assert(N == 0, "add the vmcnt literal");
}

// quantized output of problem i of a launch (fk_gemm_mxfp8_q_args): bytes / scales already advanced to the column window
struct MxQOut {
  uint8_t* q;
  uint8_t* s;
  int64_t ldq, ld_scale;
};
struct MxGroupQ {
  MxGroup g;
  MxQOut o[FK_MAX_GROUP];
};

// split-K pairs (gemm_mxsk_kernel): the workspace of fk_gemm_args.splitk_ws -- slots x 256 KiB of fp32 partial tiles, then one
// (counter, flag) word pair per slot -- and the exchange (the SK_* of gemm_pingpong_bf16.hip's GroupArgs.sk_mode)
enum { SK_WHOLE = 0, SK_SYM = 1, SK_SYM_UNANNOUNCED = 2 };
struct MxGroupSk {
  MxGroup g;
  float* partials;
  unsigned* ctl;
  int mode;
};

// ---- split-K rendezvous -------------------------------------------------------------------------------------------------
// The protocol of gemm_pingpong_bf16.hip (gemm8_body, "split-K rendezvous"), restated here and not shared as one text: there it
// is written against that kernel's lambdas and register allocation, and the bf16 kernels are held to the parent commit's device
// code byte for byte.  Same workspace, same words, same payload layout, so bf16 and MXFP8 launches of one stream share a workspace.
//
// The two workgroups of a tile each hold the fp32 partial sums of half the K range and meet through workspace slot `slot`:
// 256 KiB of payload and two control words, a COUNTER and a FLAG.  Every use of a slot moves each word forward by exactly 4, so
// both are multiples of 4 (and equal) whenever a launch starts, nothing is reset between launches, and a wrap changes nothing.
// fp32 addition commutes, so own + other has the same bits whichever workgroup forms it: the form a tile takes does not show.
//   WHOLE (mode SK_WHOLE; the fallback of the symmetric form): a workgroup draws a ticket (+2) when it is done multiplying.  The
// FIRST writes its whole partial tile with write-through stores, drains them, moves the flag to base + 4 and exits; the SECOND
// waits for that flag value, acquires, adds the stored partials to its own and runs the epilogue (as its two 128-row halves).
//   SYMMETRIC: part p writes only rows [128 (1 - p), + 128) of its partial tile (acc[.][mf] covers row half mf >> 1), moves the
// flag by 2, waits for base + 4 -- both halves published --, adds the partner's rows [128 p, + 128) to its own and runs the
// epilogue on that half.  A symmetric wait is only safe for a partner that is on the chip, so every workgroup ANNOUNCES itself on
// entry (+1 on the counter) and draws its ticket with another +1; announcement a and ticket t tell a workgroup everything:
//     t = base + 1   first to finish, the partner has not announced itself   -> WHOLE, first
//     t = base + 2   first to finish, the partner is on the chip             -> SYMMETRIC
//     t = base + 3   second to finish; a = base + 2: the first saw t = base + 1 -> WHOLE, second; else SYMMETRIC
// so no workgroup ever waits for one that has not drawn a ticket or announced itself.  SK_SYM_UNANNOUNCED (tests) decides as if
// the partner's announcement had not been seen.  Every wait is bounded: a corrupted workspace ends in a wrong tile, which the
// tests see, not in a hung device.  Payload: write-through (sc1) 16-byte stores -> per-wave vmcnt(0) -> barrier -> one-lane
// relaxed agent-scope flag add; consumer: one-lane relaxed bounded poll -> ONE agent acquire -> barrier -> sc1 loads.
template <int EPI, int BN>
FK_DEV void sk_finish(const f32x16_t (&acc)[CfgMx<BN>::NF][CfgMx<BN>::MF], const fk_gemm_args& p, const MxGroupSk& sk, char* smem,
                      int slot, int sk_part, unsigned sk_ann, int m0, int n0, int wm, int wn) {
  using C = CfgMx<BN>;
  static_assert(BN == 256, "split-K pairs: the 256 x 256 tile");
  const int tid = threadIdx.x;
  typedef __attribute__((address_space(1))) unsigned gu32;
  gu32* const ctl = (gu32*)(sk.ctl + 2 * (size_t)slot);
  const __amdgpu_buffer_rsrc_t rs_p =
      __builtin_amdgcn_make_buffer_rsrc((void*)(sk.partials + (size_t)slot * (BM * BN)), 0, BM * BN * 4, 0x00020000);
  const bool announced = sk.mode != SK_WHOLE;
  // the K loop ended with a barrier: every wave is done with the stages, whose first words now carry the ticket and the role
  if (tid == 0) {
    const unsigned t = __hip_atomic_fetch_add(ctl, announced ? 1u : 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned role;   // 0 = WHOLE first, 1 = WHOLE second, 2 = SYMMETRIC
    if (!announced) role = (t & 2u) ? 1u : 0u;
    else {
      const bool blind = sk.mode == SK_SYM_UNANNOUNCED;
      if ((t & 3u) == 3u) role = (blind || (sk_ann & 3u) == 2u) ? 1u : 2u;
      else role = ((t & 3u) == 2u && !blind) ? 2u : 0u;
    }
    ((volatile unsigned*)smem)[0] = t;
    ((volatile unsigned*)smem)[1] = role;
  }
  __syncthreads();
  const unsigned ticket = __builtin_amdgcn_readfirstlane(((volatile unsigned*)smem)[0]);
  const unsigned role = __builtin_amdgcn_readfirstlane(((volatile unsigned*)smem)[1]);
  const unsigned target = (ticket & ~3u) + 4u;   // the flag once everything this rendezvous needs is published
  auto wait_flag = [&]() {
    if (tid == 0) {
      // bounded (~seconds): the partner is resident and microseconds from publishing
      int spins = 0;
      while (__hip_atomic_load(ctl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != target && spins < (1 << 22)) {
        __builtin_amdgcn_s_sleep(8);
        ++spins;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
  };
  auto publish = [&](unsigned step) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains its own stores
    __syncthreads();
    if (tid == 0) __hip_atomic_fetch_add(ctl + 1, step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  // 16-byte pieces of the accumulators per thread: piece r of thread t at (r * 512 + t) * 16, rows [0, 128) of the tile in
  // pieces [0, NV / 2) -- piece = (row half, nf, mf & 1, quad)
  constexpr int NV = C::NF * C::MF * 4, NH = NV / 2;
  auto store_piece = [&](int r) {
    const f32x16_t& a = acc[(r % NH) / 8][2 * (r / NH) + (r / 4) % 2];
    const int q = r & 3;
    const u32x4_t v = {__float_as_uint(a[4 * q]), __float_as_uint(a[4 * q + 1]), __float_as_uint(a[4 * q + 2]),
                       __float_as_uint(a[4 * q + 3])};
    __builtin_amdgcn_raw_buffer_store_b128(v, rs_p, tid * 16, r * (C::NTHREADS * 16), /*sc1: write through*/ 16);
  };
  // rows [128 keep, + 128) of the tile: all 16 pieces of the partner's at once (into registers the K loop no longer needs),
  // own + other on the way into the epilogue
  auto finish_half = [&](auto keep_c) {
    constexpr int keep = decltype(keep_c)::value;
    u32x4_t other[NH];
#pragma unroll
    for (int r = 0; r < NH; ++r)
      other[r] = __builtin_amdgcn_raw_buffer_load_b128(rs_p, tid * 16, (keep * NH + r) * (C::NTHREADS * 16), /*sc1*/ 16);
    store_tile<EPI, BN, C, keep, 4>(acc, p, smem, m0, n0, wm, wn, other);
  };
  if (role == 0u) {
#pragma unroll
    for (int r = 0; r < NV; ++r) store_piece(r);
    publish(4u);
    return;
  }
  if (role == 2u) {
    // part p hands over the pieces of row half 1 - p and finishes half p
    if (sk_part == 0) {
#pragma unroll
      for (int r = 0; r < NH; ++r) store_piece(NH + r);
    } else {
#pragma unroll
      for (int r = 0; r < NH; ++r) store_piece(r);
    }
    publish(2u);
  }
  wait_flag();
  // SYMMETRIC: the half this part keeps; WHOLE, second: the whole tile as its two halves, one after the other
  if (role == 1u || sk_part == 0) finish_half(std::integral_constant<int, 0>{});
  if (role == 1u || sk_part == 1) finish_half(std::integral_constant<int, 1>{});
}

// one output tile; QOUT: the quantized-output epilogue into qo[problem] instead of store_tile; SK: workgroup t is part t & 1 of
// tile t >> 1 (slot t >> 1 of the workspace), multiplies K-tiles [part * nk / 2, + nk / 2) and finishes through sk_finish above
template <int EPI, int BN, bool QOUT, bool SK = false>
FK_DEV void mx_tile(const MxGroup& ga, const MxQOut* qo, const MxGroupSk* sk = nullptr) {
  using C = CfgMx<BN>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = SK ? xcd_chunk_index() >> 1 : xcd_chunk_index();
  const int sk_part = SK ? xcd_chunk_index() & 1 : 0;
  int pi = 0;
#pragma unroll
  for (int i = 1; i < FK_MAX_GROUP; ++i)
    if (i < ga.n && t >= ga.tiles_before[i]) pi = i;
  const fk_gemm_mxfp8_args& P = ga.p[pi];
  const fk_gemm_args& p = P.g;
  int m0, n0;
  {
    const int tl = t - ga.tiles_before[pi];
    const int nbm = (p.M + BM - 1) / BM, nbn = p.N / BN;
    const int per_group = MX_GROUP_M * nbn;
    const int g = tl / per_group, first_m = g * MX_GROUP_M;
    const int gm = min(nbm - first_m, MX_GROUP_M), rem = tl - g * per_group;
    m0 = (first_m + rem % gm) * BM;
    n0 = (rem / gm) * BN;
  }
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int nk = SK ? (p.K / C::BK) >> 1 : p.K / C::BK;
  const int kt0 = SK ? sk_part * nk : 0;   // this workgroup's first K-tile
  const int mlast = p.M - 1 - m0;   // rows past M are read as row M - 1 (never stored)

  // ---- LDS-DMA sources.  Tile piece = 8 rows x 128 B, lane -> (row lane >> 3, slot lane & 7), source chunk slot ^ (row & 7);
  // waves 0-3 fetch the A scale dwords of rows 64 w + lane, waves 4 .. 4 + BN / 64 - 1 those of W
  const BufDesc da = make_buf_desc((const char*)P.A8 + (int64_t)m0 * P.lda8, 0x7fffffffu);
  const BufDesc dw = make_buf_desc((const char*)P.W8 + (int64_t)n0 * P.ldw8, 0x7fffffffu);
  const BufDesc dsa = make_buf_desc((const uint8_t*)P.A_scale + (int64_t)m0 * P.lda_scale, 0x7fffffffu);
  const BufDesc dsw = make_buf_desc((const uint8_t*)P.W_scale + (int64_t)n0 * P.ldw_scale, 0x7fffffffu);
  const int lrow = lane >> 3, slot = lane & 7;
  int a_voff[4], w_voff[C::W_PIECES];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = (wave * 4 + j) * 8 + lrow;
    a_voff[j] = min(r, mlast) * (int)P.lda8 + ((slot ^ (r & 7)) << 4);
  }
#pragma unroll
  for (int j = 0; j < C::W_PIECES; ++j) {
    const int r = (wave * C::W_PIECES + j) * 8 + lrow;
    w_voff[j] = r * (int)P.ldw8 + ((slot ^ (r & 7)) << 4);
  }
  const bool sc_a = wave < 4, sc_w = !sc_a && wave < 4 + C::W_PIECES;
  const int sc_voff = sc_a ? min(wave * 64 + lane, mlast) * (int)P.lda_scale : (wave - 4) * 64 * (int)P.ldw_scale + lane * (int)P.ldw_scale;
  auto issue = [&](int stage, int kt) {
    if constexpr (SK) kt += kt0;
    char* base = smem + stage * C::STAGE_BYTES;
    // the scale piece first: the wait below counts only the tile pieces of the NEXT K-tile as still in flight
    if (sc_a) buffer_lds_opaque<4>(dsa, lds_addr_of(base + C::AS_OFF + wave * 256), sc_voff, kt * 4);
    else if (sc_w) buffer_lds_opaque<4>(dsw, lds_addr_of(base + C::WS_OFF + (wave - 4) * 256), sc_voff, kt * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) buffer_lds_opaque<16>(da, lds_addr_of(base + (wave * 4 + j) * 1024), a_voff[j], kt * C::BK);
#pragma unroll
    for (int j = 0; j < C::W_PIECES; ++j)
      buffer_lds_opaque<16>(dw, lds_addr_of(base + C::A_BYTES + (wave * C::W_PIECES + j) * 1024), w_voff[j], kt * C::BK);
  };

  // ---- fragments: row (lane & 15) of a 16-row block, chunks g and 4 + g (g = lane >> 4); scale: byte g of the row's dword
  const int frow = lane & 15, g = lane >> 4;
  const int c0 = (g ^ (frow & 7)) << 4, c1 = ((4 + g) ^ (frow & 7)) << 4;
  auto frag = [&](const char* tile, int row0) {
    const char* rp = tile + (row0 + frow) * C::BK;
    const u32x4_t lo = *(const u32x4_t*)(rp + c0), hi = *(const u32x4_t*)(rp + c1);
    return i32x8_t{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
  };
  auto scale = [&](const char* s, int row0) { return (int)(*(const uint32_t*)(s + (row0 + frow) * 4) >> (8 * g)); };

  f32x16_t acc[C::NF][C::MF];
#pragma unroll
  for (int i = 0; i < C::NF; ++i)
#pragma unroll
    for (int j = 0; j < C::MF; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  issue(0, 0);
  // split-K pairs: "I am on the chip" (sk_finish).  Behind the prologue's requests, so the round trip of the add hides behind
  // theirs; only wave 0 waits for it, and the value stays scalar.
  unsigned sk_ann = 0;
  if constexpr (SK) {
    if (sk->mode != SK_WHOLE && wave == 0) {
      unsigned r = 0;
      if (lane == 0)
        r = __hip_atomic_fetch_add((__attribute__((address_space(1))) unsigned*)(sk->ctl + 2 * (size_t)t), 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
      sk_ann = __builtin_amdgcn_readfirstlane(r);
    }
  }
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) {
      issue((kt + 1) & 1, kt + 1);   // its stage was last read before the trailing barrier of iteration kt - 1
      wait_vm<4 + C::W_PIECES>();
    } else {
      wait_vm<0>();
    }
    __syncthreads();
    const char* st = smem + (kt & 1) * C::STAGE_BYTES;
    i32x8_t wf[C::NF][2];
    int wsc[C::NF][2];
#pragma unroll
    for (int nf = 0; nf < C::NF; ++nf)
#pragma unroll
      for (int n16 = 0; n16 < 2; ++n16) {
        const int r0 = C::tile_col(wn, nf) + 16 * n16;
        wf[nf][n16] = frag(st + C::A_BYTES, r0);
        wsc[nf][n16] = scale(st + C::WS_OFF, r0);
      }
#pragma unroll
    for (int mf = 0; mf < C::MF; ++mf) {
      i32x8_t af[2];
      int asc[2];
#pragma unroll
      for (int m16 = 0; m16 < 2; ++m16) {
        const int r0 = C::tile_row(wm, mf) + 16 * m16;
        af[m16] = frag(st, r0);
        asc[m16] = scale(st + C::AS_OFF, r0);
      }
#pragma unroll
      for (int nf = 0; nf < C::NF; ++nf)
#pragma unroll
        for (int n16 = 0; n16 < 2; ++n16)
#pragma unroll
          for (int m16 = 0; m16 < 2; ++m16) {
            const int q = 2 * n16 + m16;
            // formats 0 / 0 = e4m3 x e4m3; scale byte 0 of each lane's scale register
            quad_set(acc[nf][mf], q,
                     __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[nf][n16], af[m16], quad_get(acc[nf][mf], q), 0, 0,
                                                                       0, wsc[nf][n16], 0, asc[m16]));
          }
    }
    __syncthreads();
  }
  if constexpr (SK) sk_finish<EPI, BN>(acc, p, *sk, smem, t, sk_part, sk_ann, m0, n0, wm, wn);
  else if constexpr (QOUT) store_tile_mxq<EPI, BN, C>(acc, p, qo[pi].q, qo[pi].s, qo[pi].ldq, qo[pi].ld_scale, smem, m0, n0, wm, wn);
  else store_tile<EPI, BN, C>(acc, p, smem, m0, n0, wm, wn);
}

template <int EPI, int BN>
__global__ __launch_bounds__(512, 2) void gemm_mxfp8_kernel(const MxGroup ga) {
  mx_tile<EPI, BN, false>(ga, nullptr);
}

template <int EPI, int BN>
__global__ __launch_bounds__(512, 2) void gemm_mxq_kernel(const MxGroupQ gq) {
  mx_tile<EPI, BN, true>(gq.g, gq.o);
}

// split-K pairs: grid = 2 x tiles, workgroup b is part b & 1 of tile b >> 1 in the XCD-chunked order (both parts of a tile on one
// XCD wherever the grid divides: the exchange then stays in that XCD's L2)
template <int EPI>
__global__ __launch_bounds__(512, 2) void gemm_mxsk_kernel(const MxGroupSk gs) {
  mx_tile<EPI, 256, false, true>(gs.g, nullptr, &gs);
}

int cu_count_mx() {
  static int cus = 0;
  if (!cus) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
    else return 256;
  }
  return cus;
}

template <int EPI, int BN>
int launch_mx(MxGroup& ga, int tiles, hipStream_t stream) {
  using C = CfgMx<BN>;
  auto kern = gemm_mxfp8_kernel<EPI, BN>;
  FK_ENSURE_MAX_LDS(kern, C::SMEM_BYTES, "fk_gemm_mxfp8");
  hipLaunchKernelGGL(kern, dim3(tiles), dim3(C::NTHREADS), C::SMEM_BYTES, stream, ga);
  FK_CHECK_LAUNCH("fk_gemm_mxfp8");
  return FK_OK;
}

template <int EPI, int BN>
int launch_mxq(MxGroupQ& gq, int tiles, hipStream_t stream) {
  using C = CfgMx<BN>;
  auto kern = gemm_mxq_kernel<EPI, BN>;
  FK_ENSURE_MAX_LDS(kern, C::SMEM_BYTES, "fk_gemm_mxfp8_q");
  hipLaunchKernelGGL(kern, dim3(tiles), dim3(C::NTHREADS), C::SMEM_BYTES, stream, gq);
  FK_CHECK_LAUNCH("fk_gemm_mxfp8_q");
  return FK_OK;
}

template <int EPI>
int launch_mxsk(const MxGroupSk& gs, int tiles, hipStream_t stream) {
  using C = CfgMx<256>;
  auto kern = gemm_mxsk_kernel<EPI>;
  FK_ENSURE_MAX_LDS(kern, C::SMEM_BYTES, "fk_gemm_mxfp8 (split-K pairs)");
  hipLaunchKernelGGL(kern, dim3(2 * tiles), dim3(C::NTHREADS), C::SMEM_BYTES, stream, gs);
  FK_CHECK_LAUNCH("fk_gemm_mxfp8 (split-K pairs)");
  return FK_OK;
}

template <int EPI>
int launch_mx_bn(MxGroup& ga, int tiles, int bn, hipStream_t stream) {
  return bn == 256 ? launch_mx<EPI, 256>(ga, tiles, stream) : launch_mx<EPI, 128>(ga, tiles, stream);
}

// a 256-row tile's rows addressable with 32-bit byte offsets from its first row (what TileRows / the DMA offsets assume)
bool rows32(const fk_rows& r, int elem) {
  const long long ld = r.ld < 0 ? -r.ld : r.ld, bs = r.batch_stride < 0 ? -r.batch_stride : r.batch_stride;
  if (r.ld < 0 || (BM * ld + (r.rows_per_batch > 0 ? bs : 0)) * elem >= (1ll << 31)) return false;
  return !(r.rows_per_batch > 0 && r.batch_stride < r.rows_per_batch * r.ld);
}

// qout: the quantized-output form (fk_gemm_mxfp8_q) -- g.C / g.c are unused, the epilogue is FK_EPI_NONE or GELU_TANH
int validate_mx(const fk_gemm_mxfp8_args& a, const char* fn, bool qout = false) {
  const fk_gemm_args& p = a.g;
  FK_CHECK_ARG(a.A8 && a.A_scale && a.W8 && a.W_scale && (qout || p.C), "%s: null operand, scale or output pointer", fn);
  FK_CHECK_ARG(p.M >= 0 && p.N > 0 && p.K > 0, "%s: M %d N %d K %d", fn, p.M, p.N, p.K);
  if (p.K % 128 != 0 || p.N % 256 != 0) {
    fk_set_error("%s: needs K %% 128 == 0 and N %% 256 == 0 (M %d N %d K %d)", fn, p.M, p.N, p.K);
    return FK_EUNSUPPORTED;
  }
  if (!(p.out_fp32 == 0 || p.out_fp32 == 2) || p.layout != 0 || p.f32_flags != 0 ||
      !(p.epilogue == FK_EPI_NONE || (p.out_fp32 == 0 && (p.epilogue == FK_EPI_GELU_TANH || p.epilogue == FK_EPI_GATE_RES ||
                                                           p.epilogue == FK_EPI_QKV)))) {
    fk_set_error("%s: epilogue %d / out_fp32 %d / layout %d: supported are FK_EPI_NONE, GELU_TANH, GATE_RES, QKV (bf16 out) "
                 "and FK_EPI_NONE with out_fp32 = 2, layout 0", fn, p.epilogue, p.out_fp32, p.layout);
    return FK_EUNSUPPORTED;
  }
  if (qout && (p.out_fp32 != 0 || !(p.epilogue == FK_EPI_NONE || p.epilogue == FK_EPI_GELU_TANH))) {
    fk_set_error("%s: the quantized output takes FK_EPI_NONE or FK_EPI_GELU_TANH (epilogue %d, out_fp32 %d)", fn, p.epilogue, p.out_fp32);
    return FK_EUNSUPPORTED;
  }
  // the output / bias / residual / gate / QKV fields as fk_gemm_bf16 checks them (the epilogue is the same code)
  FK_CHECK_ARG(qout || (uintptr_t)p.C % 16 == 0, "%s: C must be 16-byte aligned", fn);
  if (qout)
    FK_CHECK_ARG(!p.bias || (uintptr_t)p.bias % 8 == 0, "%s: bias must be 8-byte aligned", fn);
  else if (p.out_fp32 == 2)
    FK_CHECK_ARG(p.c.ld % 4 == 0 && (p.c.rows_per_batch <= 0 || p.c.batch_stride % 4 == 0) && (!p.bias || (uintptr_t)p.bias % 8 == 0),
                 "%s: out_fp32 = 2 needs ldc %% 4 == 0 and an 8-byte aligned bias", fn);
  else
    FK_CHECK_ARG(p.c.ld % 8 == 0 && (p.c.rows_per_batch <= 0 || p.c.batch_stride % 8 == 0) && (!p.bias || (uintptr_t)p.bias % 8 == 0),
                 "%s: ldc / C batch stride must be multiples of 8, bias 8-byte aligned", fn);
  if (p.epilogue == FK_EPI_GATE_RES) {
    FK_CHECK_ARG(p.res && (uintptr_t)p.res % 16 == 0 && p.r.ld % 8 == 0 && (p.r.rows_per_batch <= 0 || p.r.batch_stride % 8 == 0),
                 "%s: residual pointer/stride invalid", fn);
    FK_CHECK_ARG(p.gate && (uintptr_t)p.gate % 16 == 0 && p.gate_batch_stride % 8 == 0 && p.gate_rows_per_batch > 0,
                 "%s: gate pointer/stride invalid", fn);
  }
  if (p.epilogue == FK_EPI_QKV) {
    FK_CHECK_ARG(p.q_out && p.k_out && p.wq && p.wk && p.rope_cs, "%s: FK_EPI_QKV needs q_out, k_out, wq, wk and rope_cs", fn);
    FK_CHECK_ARG(p.qkv_heads > 0 && (p.N == 3 * p.qkv_heads * 128 || p.N == 2 * p.qkv_heads * 128) && p.qkv_s_total > 0 &&
                     p.qkv_s_offset >= 0,
                 "%s: FK_EPI_QKV needs N = 3*H*128 (q | k | v) or 2*H*128 (q | k)", fn);
    const int64_t rpb = p.c.rows_per_batch > 0 ? p.c.rows_per_batch : p.M;
    const int64_t nb = p.c.rows_per_batch > 0 ? (p.M + p.c.rows_per_batch - 1) / p.c.rows_per_batch : 1;
    FK_CHECK_ARG((int64_t)p.qkv_s_offset + rpb <= p.qkv_s_total, "%s: FK_EPI_QKV token rows s_offset %d + %lld exceed S_total %d",
                 fn, p.qkv_s_offset, (long long)rpb, p.qkv_s_total);
    FK_CHECK_ARG(nb * p.qkv_heads * p.qkv_s_total < (int64_t)1 << 31, "%s: FK_EPI_QKV head-major outputs are limited to 2^31 rows", fn);
    FK_CHECK_ARG(((uintptr_t)p.q_out | (uintptr_t)p.k_out | (uintptr_t)p.wq | (uintptr_t)p.wk | (uintptr_t)p.rope_cs) % 16 == 0,
                 "%s: FK_EPI_QKV pointers must be 16-byte aligned", fn);
  }
  FK_CHECK_ARG(a.lda8 >= p.K && a.lda8 % 16 == 0 && a.ldw8 >= p.K && a.ldw8 % 16 == 0 &&
               a.lda_scale >= p.K / 32 && a.lda_scale % 4 == 0 && a.ldw_scale >= p.K / 32 && a.ldw_scale % 4 == 0,
               "%s: operand rows need ld >= K, ld %% 16 == 0; scale rows ld >= K / 32, ld %% 4 == 0 (lda8 %lld ldw8 %lld "
               "lda_scale %lld ldw_scale %lld)", fn, (long long)a.lda8, (long long)a.ldw8, (long long)a.lda_scale,
               (long long)a.ldw_scale);
  FK_CHECK_ARG(((uintptr_t)a.A8 | (uintptr_t)a.W8) % 16 == 0 && ((uintptr_t)a.A_scale | (uintptr_t)a.W_scale) % 4 == 0,
               "%s: operands must be 16-byte, scales 4-byte aligned", fn);
  const bool res = p.epilogue == FK_EPI_GATE_RES;
  if ((long long)BM * a.lda8 >= (1ll << 31) || (long long)BM * a.ldw8 >= (1ll << 31) || (long long)BM * a.lda_scale >= (1ll << 31) ||
      (long long)BM * a.ldw_scale >= (1ll << 31) || (!qout && !rows32(p.c, p.out_fp32 == 2 ? 4 : 2)) || (res && !rows32(p.r, 2))) {
    fk_set_error("%s: row strides must keep a 256-row tile within 2 GiB", fn);
    return FK_EUNSUPPORTED;
  }
  return FK_OK;
}
}  // namespace

extern "C" int fk_quantize_mxfp8(const void* x, fk_rows xr, int64_t M, int32_t K, void* q, int64_t ldq, void* scales,
                                 int64_t ld_scale, fk_stream_t stream) {
  FK_CHECK_ARG(x && q && scales, "fk_quantize_mxfp8: null pointer");
  FK_CHECK_ARG(M >= 0 && K > 0, "fk_quantize_mxfp8: M %lld K %d", (long long)M, K);
  if (K % 32 != 0) {
    fk_set_error("fk_quantize_mxfp8: K %% 32 == 0 needed (K %d)", K);
    return FK_EUNSUPPORTED;
  }
  FK_CHECK_ARG(xr.ld >= K && xr.ld % 8 == 0 && (uintptr_t)x % 16 == 0 && (xr.rows_per_batch <= 0 || xr.batch_stride % 8 == 0),
               "fk_quantize_mxfp8: x rows must be 16-byte aligned with ld >= K");
  FK_CHECK_ARG(ldq >= K && ldq % 16 == 0 && (uintptr_t)q % 16 == 0 && ld_scale >= K / 32,
               "fk_quantize_mxfp8: q rows 16-byte aligned with ldq >= K, ld_scale >= K / 32");
  if (M == 0) return FK_OK;
  const int64_t blocks = M * (K / 32);
  const int64_t grid = (blocks + 255) / 256;
  FK_CHECK_ARG(grid < (1ll << 31), "fk_quantize_mxfp8: too many rows");
  hipLaunchKernelGGL(quantize_mxfp8_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, xr, M, K,
                     (uint8_t*)q, ldq, (uint8_t*)scales, ld_scale);
  FK_CHECK_LAUNCH("fk_quantize_mxfp8");
  return FK_OK;
}

// fk_gemm_args.variant_used: 128 / 256 = the 256 x 128 / 256 x 256 tile, 512 = split-K pairs of the 256 x 256 tile
extern "C" int fk_gemm_mxfp8_grouped(const fk_gemm_mxfp8_args* args, int32_t n, fk_stream_t stream_) {
  FK_CHECK_ARG(args != nullptr && n >= 1 && n <= FK_MAX_GROUP, "fk_gemm_mxfp8_grouped: 1 <= n <= %d", FK_MAX_GROUP);
  const fk_gemm_args& c0 = args[0].g;
  for (int i = 0; i < n; ++i) {
    const int rc = validate_mx(args[i], n == 1 ? "fk_gemm_mxfp8" : "fk_gemm_mxfp8_grouped");
    if (rc != FK_OK) return rc;
    FK_CHECK_ARG(args[i].g.N == c0.N && args[i].g.K == c0.K && args[i].g.epilogue == c0.epilogue &&
                 args[i].g.out_fp32 == c0.out_fp32, "fk_gemm_mxfp8_grouped: all problems must share N, K, epilogue and out_fp32");
  }
  FK_CHECK_ARG(c0.variant == 0 || c0.variant == 128 || c0.variant == 256 || c0.variant == 512,
               "fk_gemm_mxfp8: variant %d is not 0, 128, 256 or 512 (split-K pairs)", c0.variant);
  // plan: as fk_gemm_bf16 validates it (explicit bit, allow bits, at most one exchange bit); only bit 1 and the exchange matter here
  constexpr int SK_BITS = FK_GEMM_PLAN_SPLITK_WHOLE | FK_GEMM_PLAN_SPLITK_SYMMETRIC | FK_GEMM_PLAN_SPLITK_UNANNOUNCED;
  const int sk_bits = c0.plan & SK_BITS;
  // (the tile-walk bits travel with a block's plan and mean nothing to these kernels)
  if ((c0.plan != 0 && ((c0.plan & ~(15 | SK_BITS | FK_GEMM_PLAN_WALK_BITS)) != 0 || !(c0.plan & FK_GEMM_PLAN_EXPLICIT))) || (sk_bits & (sk_bits - 1)) != 0) {
    fk_set_error("fk_gemm_mxfp8: plan %d is not 0 (default) or FK_GEMM_PLAN_EXPLICIT | allow bits 0..2 | at most one "
                 "FK_GEMM_PLAN_SPLITK_* exchange", c0.plan);
    return FK_EINVAL;
  }
  MxGroupSk gs;
  MxGroup& ga = gs.g;
  ga.n = n;
  long nbm = 0;
  ga.tiles_before[0] = 0;
  for (int i = 0; i < FK_MAX_GROUP; ++i) ga.p[i] = args[i < n ? i : 0];
  for (int i = 0; i < n; ++i) nbm += (args[i].g.M + BM - 1) / BM;
  // launch plan: 256 x 256 tiles unless they leave part of the chip idle in a single round (then twice as many 256 x 128 ones)
  const long t256 = nbm * (c0.N / 256);
  // split-K pairs: two half-K workgroups per 256 x 256 tile in ONE round of CUs -- the bf16 planner's class (K >= 6144, an even
  // number of K-tiles, 2 x tiles <= CUs, a slot per tile), for the epilogues of the long-K launches.  Handing over a workspace
  // is the opt-in: without one nothing is ever split.
  const int ws_slots = c0.splitk_ws ? c0.splitk_slots : 0;
  const bool sk_epi = c0.epilogue == FK_EPI_NONE || c0.epilogue == FK_EPI_GATE_RES;
  const bool sk_shape = c0.K >= 6144 && (c0.K / 128) % 2 == 0;
  int bn;
  if (c0.variant == 512) {   // forced: every misuse is an error (nothing falls back silently)
    if (!sk_epi || !sk_shape) {
      fk_set_error("fk_gemm_mxfp8: variant 512 (split-K pairs) takes FK_EPI_NONE (bf16 or out_fp32 = 2) or FK_EPI_GATE_RES, K >= 6144 "
                   "and an even K / 128 (epilogue %d, K %d)", c0.epilogue, c0.K);
      return FK_EUNSUPPORTED;
    }
    FK_CHECK_ARG(ws_slots > 0 && t256 <= ws_slots, "fk_gemm_mxfp8: variant 512 (split-K pairs) needs a split-K workspace with a slot "
                 "per 256 x 256 tile (%ld tiles, %d slots)", t256, ws_slots);
    bn = 512;
  } else if (c0.variant) {
    bn = c0.variant;
  } else {
    const bool allow_sk = c0.plan == 0 || (c0.plan & 2);
    const bool sk = ws_slots > 0 && allow_sk && sk_epi && sk_shape && 2 * t256 <= cu_count_mx() && t256 <= ws_slots;
    bn = sk ? 512 : (t256 < cu_count_mx() ? 128 : 256);
  }
  const int width = bn == 512 ? 256 : bn;
  long tiles = 0;
  for (int i = 0; i < n; ++i) {
    ga.tiles_before[i] = (int)tiles;
    tiles += (long)((args[i].g.M + BM - 1) / BM) * (c0.N / width);
  }
  for (int i = n; i <= FK_MAX_GROUP; ++i) ga.tiles_before[i] = (int)tiles;
  if (c0.variant_used) *c0.variant_used = bn;
  if (tiles == 0) return FK_OK;
  FK_CHECK_ARG(tiles < (1l << 31), "fk_gemm_mxfp8: too many tiles");
  hipStream_t stream = (hipStream_t)stream_;
  if (bn == 512) {
    gs.partials = (float*)c0.splitk_ws;
    gs.ctl = (unsigned*)((char*)c0.splitk_ws + (size_t)ws_slots * (BM * 256 * 4));
    gs.mode = sk_bits == FK_GEMM_PLAN_SPLITK_WHOLE ? SK_WHOLE : sk_bits == FK_GEMM_PLAN_SPLITK_UNANNOUNCED ? SK_SYM_UNANNOUNCED : SK_SYM;
    if (c0.out_fp32 == 2) return launch_mxsk<FK_EPI_F32DBG>(gs, (int)tiles, stream);
    return c0.epilogue == FK_EPI_GATE_RES ? launch_mxsk<FK_EPI_GATE_RES>(gs, (int)tiles, stream)
                                          : launch_mxsk<FK_EPI_NONE>(gs, (int)tiles, stream);
  }
  switch (c0.out_fp32 == 2 ? FK_EPI_F32DBG : c0.epilogue) {
    case FK_EPI_F32DBG: return launch_mx_bn<FK_EPI_F32DBG>(ga, (int)tiles, bn, stream);
    case FK_EPI_NONE: return launch_mx_bn<FK_EPI_NONE>(ga, (int)tiles, bn, stream);
    case FK_EPI_GELU_TANH: return launch_mx_bn<FK_EPI_GELU_TANH>(ga, (int)tiles, bn, stream);
    case FK_EPI_GATE_RES: return launch_mx_bn<FK_EPI_GATE_RES>(ga, (int)tiles, bn, stream);
    case FK_EPI_QKV: return launch_mx_bn<FK_EPI_QKV>(ga, (int)tiles, bn, stream);
    default: fk_set_error("fk_gemm_mxfp8: unknown epilogue %d", c0.epilogue); return FK_EUNSUPPORTED;
  }
}

extern "C" int fk_gemm_mxfp8(const fk_gemm_mxfp8_args* args, fk_stream_t stream) {
  FK_CHECK_ARG(args != nullptr, "fk_gemm_mxfp8: null args");
  return fk_gemm_mxfp8_grouped(args, 1, stream);
}

// The quantized-output form: the same launch plan and main loop; the tile leaves as e4m3 bytes + E8M0 scale bytes in a column
// window [col_offset, col_offset + N) of a [M, ldq] byte buffer (scales: [col_offset / 32, ..) of [M, ldq_scale]).
extern "C" int fk_gemm_mxfp8_q_grouped(const fk_gemm_mxfp8_q_args* args, int32_t n, fk_stream_t stream_) {
  FK_CHECK_ARG(args != nullptr && n >= 1 && n <= FK_MAX_GROUP, "fk_gemm_mxfp8_q_grouped: 1 <= n <= %d", FK_MAX_GROUP);
  const char* fn = n == 1 ? "fk_gemm_mxfp8_q" : "fk_gemm_mxfp8_q_grouped";
  const fk_gemm_args& c0 = args[0].a.g;
  for (int i = 0; i < n; ++i) {
    const fk_gemm_mxfp8_q_args& a = args[i];
    const int rc = validate_mx(a.a, fn, true);
    if (rc != FK_OK) return rc;
    const fk_gemm_args& g = a.a.g;
    FK_CHECK_ARG(g.N == c0.N && g.K == c0.K && g.epilogue == c0.epilogue, "%s: all problems must share N, K and the epilogue", fn);
    FK_CHECK_ARG(a.Q && a.Q_scale, "%s: null quantized output", fn);
    FK_CHECK_ARG(a.col_offset >= 0 && a.col_offset % 32 == 0, "%s: column offset %lld must be a multiple of 32", fn,
                 (long long)a.col_offset);
    FK_CHECK_ARG(a.ldq >= a.col_offset + g.N && a.ldq_scale >= (a.col_offset + g.N) / 32,
                 "%s: ldq %lld / ldq_scale %lld do not hold columns [%lld, %lld)", fn, (long long)a.ldq, (long long)a.ldq_scale,
                 (long long)a.col_offset, (long long)(a.col_offset + g.N));
    FK_CHECK_ARG((uintptr_t)a.Q % 16 == 0 && a.ldq % 16 == 0 && (uintptr_t)a.Q_scale % 4 == 0 && a.ldq_scale % 4 == 0,
                 "%s: output byte rows must be 16-byte aligned (Q, ldq %lld), scale rows 4-byte aligned (Q_scale, ldq_scale %lld)", fn,
                 (long long)a.ldq, (long long)a.ldq_scale);
  }
  if (c0.variant == 512) {
    fk_set_error("%s: the quantized-output form has no split-K pairs (variant 512): 0, 128 or 256", fn);
    return FK_EUNSUPPORTED;
  }
  FK_CHECK_ARG(c0.variant == 0 || c0.variant == 128 || c0.variant == 256, "%s: variant %d is not 0, 128 or 256", fn, c0.variant);
  MxGroupQ gq;
  MxGroup& ga = gq.g;
  ga.n = n;
  long nbm = 0;
  ga.tiles_before[0] = 0;
  for (int i = 0; i < FK_MAX_GROUP; ++i) {
    const fk_gemm_mxfp8_q_args& a = args[i < n ? i : 0];
    ga.p[i] = a.a;
    gq.o[i] = MxQOut{(uint8_t*)a.Q + a.col_offset, (uint8_t*)a.Q_scale + a.col_offset / 32, a.ldq, a.ldq_scale};
  }
  for (int i = 0; i < n; ++i) nbm += (args[i].a.g.M + BM - 1) / BM;
  const long t256 = nbm * (c0.N / 256);   // the launch plan of fk_gemm_mxfp8_grouped
  const int bn = c0.variant ? c0.variant : (t256 < cu_count_mx() ? 128 : 256);
  long tiles = 0;
  for (int i = 0; i < n; ++i) {
    ga.tiles_before[i] = (int)tiles;
    tiles += (long)((args[i].a.g.M + BM - 1) / BM) * (c0.N / bn);
  }
  for (int i = n; i <= FK_MAX_GROUP; ++i) ga.tiles_before[i] = (int)tiles;
  if (c0.variant_used) *c0.variant_used = bn;
  if (tiles == 0) return FK_OK;
  FK_CHECK_ARG(tiles < (1l << 31), "%s: too many tiles", fn);
  hipStream_t stream = (hipStream_t)stream_;
  if (c0.epilogue == FK_EPI_GELU_TANH)
    return bn == 256 ? launch_mxq<FK_EPI_GELU_TANH, 256>(gq, (int)tiles, stream) : launch_mxq<FK_EPI_GELU_TANH, 128>(gq, (int)tiles, stream);
  return bn == 256 ? launch_mxq<FK_EPI_NONE, 256>(gq, (int)tiles, stream) : launch_mxq<FK_EPI_NONE, 128>(gq, (int)tiles, stream);
}

extern "C" int fk_gemm_mxfp8_q(const fk_gemm_mxfp8_q_args* args, fk_stream_t stream) {
  FK_CHECK_ARG(args != nullptr, "fk_gemm_mxfp8_q: null args");
  return fk_gemm_mxfp8_q_grouped(args, 1, stream);
}
