// The large-tile GEMMs' shared pieces: 256-row tile addressing, tile order, the accumulator fragment map and the
// epilogue (store_tile).  Included INSIDE the anonymous namespace of each kernel file: every instantiation stays local
// to its translation unit, exactly as when these lived in gemm_pingpong_bf16.hip (gemm_mxfp8.hip reuses the epilogue
// through a config struct that provides NF, MF, M16, NTHREADS, CT_LD, tile_row and tile_col).
#pragma once

#include "mxfp8_quant.h"   // store_tile_mxq's quantizer arithmetic

constexpr int BM = 256;

// fk_rows addressing of the (at most BM) rows of one tile without per-row 64-bit divisions: one division per tile
// for the tile's first row, then a compare per row (a 32-bit division when a batch has fewer rows than a tile).
// The launcher guarantees that every offset relative to the tile's first row fits 31 bits (in bytes).
struct TileRows {
  int ld, wrap, rpb, b0, r0;
  int rf;       // row of the tile's first row inside its batch b0 (= r0, except that one unbatched view counts rows from r0 = 0)
  float inv;    // 1 / rpb when a batch is shorter than a tile
  bool big;     // rpb >= BM (or no batching): a tile crosses at most one batch boundary
  // flat (the launcher's mark: row m lies at m * ld, all of the problem in batch 0): no division
  FK_DEV TileRows(const fk_rows& r, int m0, bool flat = false) {
    ld = (int)r.ld;
    if (flat) { rpb = 0x7fffffff; wrap = 0; b0 = 0; r0 = rf = m0; big = true; inv = 0.f; }
    else if (r.rows_per_batch <= 0) { rpb = 0x7fffffff; wrap = 0; b0 = 0; r0 = 0; rf = m0; big = true; inv = 0.f; }
    else {
      rpb = (int)(r.rows_per_batch > 0x7fffffff ? 0x7fffffff : r.rows_per_batch);
      b0 = (unsigned)m0 / (unsigned)rpb;
      r0 = rf = m0 - b0 * rpb;
      wrap = (int)(r.batch_stride - (int64_t)rpb * r.ld);
      big = rpb >= BM;
      inv = 1.0f / (float)rpb;
    }
  }
  // batches crossed between the tile's first row and its row ml (branch-free: r0 + ml < rpb + BM, so for short
  // batches the quotient is a small integer that the float product resolves exactly)
  FK_DEV int crossed(int ml) const {
    const int r = r0 + ml;
    const int one = r >= rpb ? 1 : 0;
    const int many = (int)(((float)r + 0.5f) * inv);
    return big ? one : many;
  }
  // element offset of row ml of the tile relative to its first row
  FK_DEV int off(int ml) const { return ml * ld + crossed(ml) * wrap; }
  // element offset of the tile's first row: fk_row_offset(r, m0) from this tile's 32-bit quotient (no 64-bit division);
  // r: what the object was made from
  FK_DEV int64_t first(const fk_rows& r) const {
    return (int64_t)b0 * r.batch_stride + (int64_t)rf * r.ld;
  }
};

// sum over the 16 lanes of a DPP row, every lane receiving the total: four row-rotate adds on the VALU (no LDS
// round trips).  Bit-identical to the xor butterfly 8, 4, 2, 1: after the step of distance d the partial sums have
// period d within the row, so "rotate by d" and "xor d" name the same partner value.
template <int N>
FK_DEV float row_ror(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 + N, 0xf, 0xf, false));
}
FK_DEV float row16_sum(float v) {
  v += row_ror<8>(v);
  v += row_ror<4>(v);
  v += row_ror<2>(v);
  v += row_ror<1>(v);
  return v;
}

// tile selection: XCD chunking over the whole grid (workgroup b runs on XCD b % 8: consecutive tiles of the order
// below -- which share A rows and W columns -- stay on one XCD's L2), then problem, then grouped (GROUP_M deep) order
FK_DEV int xcd_chunk_index() {
  const int nwg = gridDim.x;
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// ---- MFMA shape ------------------------------------------------------------------------------------------------------
// M16 = false: v_mfma_f32_32x32x16_bf16 (8 passes, 16 k per instruction); M16 = true: v_mfma_f32_16x16x32_bf16 (4 passes, 32 k
// per instruction) on the SAME LDS image, the same accumulator registers and the same number of ds_read_b128 per K-tile.
// Why both exist (tools/power_probe.hip, profiles/r05_power_probe.txt): under the chip's power limit a pure MFMA stream of
// the 16 x 16 x 32 form sustains 2 017 TF/s at 1.97 GHz against 1 800 TF/s at 1.76 GHz for the 32 x 32 x 16 form -- half the
// accumulator register traffic per flop -- and the GEMM main loops are power-bound.  A 32 x 32 accumulator block (nf, mf) of
// the epilogue holds, as quad q = 2 * n16 + m16 (4 registers = 4 consecutive output columns of one row), the 16 x 16 block
// (n16, m16) in the M16 form and columns 8 q + 4 (lane >> 5) of row (lane & 31) in the other.
template <bool M16>
struct FragMap {
  static FK_DEV int row(int lane, int q) { return M16 ? (q & 1) * 16 + (lane & 15) : (lane & 31); }
  static FK_DEV int col(int lane, int q) { return M16 ? (q >> 1) * 16 + (lane >> 4) * 4 : 8 * q + 4 * (lane >> 5); }
};
FK_DEV f32x4_t quad_get(const f32x16_t& v, int q) { return f32x4_t{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]}; }
FK_DEV void quad_set(f32x16_t& v, int q, const f32x4_t& c) {
  v[4 * q] = c[0]; v[4 * q + 1] = c[1]; v[4 * q + 2] = c[2]; v[4 * q + 3] = c[3];
}

// epilogue (as gemm_bf16.hip): bias/activation -> bf16 -> LDS tile -> coalesced 16-byte rows.
// acc[nf][mf] is the 32x32 block (n-block nf, m-block mf) of wave (wm, wn) in MFMA-output layout with the
// swapped operands: lane l holds row (l & 31) of the m-block, columns 8*q + 4*(l >> 5) + j of the n-block.
//
// With one workgroup per CU nothing overlaps the epilogue, so it must not be a chain of load -> wait -> use steps
// (measured: a bias load in front of every quad and a residual / gate / rope-table load in front of every stored
// chunk made the epilogue ~15 % of a K = 3072 tile).  All global reads are therefore issued unconditionally with
// clamped indices, a batch of EPI_BATCH chunks at a time, ahead of the arithmetic of the batch; only the final
// store is predicated.
//
// HALF = 0 / 1 (the split-K pairs' symmetric exchange): only rows [128 HALF, 128 HALF + 128) of the tile; needs a config whose
// m-blocks [HALF MF / 2, + MF / 2) are exactly those rows (Cfg8).  -1: the whole tile.  The half-tile forms add the partner's
// partial sums on the way: other[nf * 2 MF + (mf - first m-block) * 4 + q] = its quad q of block (nf, mf), own + other.
// UB: chunks per batch of the output loop (gemm_mxfp8.hip's split-K pairs take 4: their accumulators stay allocated beside it).
// flat: bit 1 / 2 / 3 (gemm_tile_map.h: TM_C_FLAT, TM_R_FLAT, TM_G_FLAT) -- the launcher found the rows of C / the residual at
// m * ld / every gate row to be row 0: the per-tile divisions of their addressing are skipped.  0: fk_rows addressing throughout.
// WALK (the tile walk of gemm_pingpong_bf16.hip): the next tile's first K-tile is in flight into the front of the ring while
// this runs.  The C (half-)tile therefore lies WALK_CT_OFF bytes into LDS, the barriers wait for LDS traffic only (a
// __syncthreads() would wait for the requests in flight and for this tile's stores), the bias quads come from the caller
// (`bias_in`, loaded in front of those requests: a wait for them is then no wait for the requests), and a half-tile pass
// (HALF >= 0) adds nothing (`other` is unused); the first pass waits for those requests before it stores (below).  The arithmetic and the rounding points are those of the other forms.
constexpr int WALK_CT_OFF = 65536;
FK_DEV void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
template <int EPI, int BN, class C, int HALF = -1, int UB = 8, bool WALK = false>
FK_DEV void store_tile(const f32x16_t (&acc)[C::NF][C::MF], const fk_gemm_args& p, char* smem, int m0, int n0,
                       int wm, int wn, const u32x4_t* other = nullptr, int flat = 0, const u32x2_t (*bias_in)[4] = nullptr) {
  constexpr bool ADD_OTHER = HALF >= 0 && !WALK;
  constexpr int MF0 = HALF > 0 ? C::MF / 2 : 0, MF1 = HALF == 0 ? C::MF / 2 : C::MF;   // m-blocks stored
  constexpr int row0 = HALF > 0 ? BM / 2 : 0;                                           // first tile row stored
  int tid = threadIdx.x;
  // gemm10 (the only 256-thread caller) may run this inside a per-CU tile loop around an asm statement that leaves 36 free
  // VGPRs: an opaque copy keeps hipcc from hoisting the 32 per-lane row indices below out of that loop and spilling them
  // (so may the tile walk, whose loop holds the K loop as well)
  if constexpr (C::NTHREADS == 256 || WALK) asm volatile("" : "+v"(tid));
  const int lane = tid & 63;
  using FM = FragMap<C::M16>;
  // bias of this lane's 4-column quads (all loads in flight before the barrier below)
  u32x2_t bw[C::NF][4];
#pragma unroll
  for (int nf = 0; nf < C::NF; ++nf)
#pragma unroll
    for (int q = 0; q < 4; ++q) bw[nf][q] = u32x2_t{0u, 0u};
  if constexpr (WALK) {
#pragma unroll
    for (int nf = 0; nf < C::NF; ++nf)
#pragma unroll
      for (int q = 0; q < 4; ++q) bw[nf][q] = bias_in[nf][q];
  } else if constexpr (EPI != FK_EPI_SCALE) {
    if (p.bias) {
#pragma unroll
      for (int nf = 0; nf < C::NF; ++nf)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = n0 + C::tile_col(wn, nf) + FM::col(lane, q);
          bw[nf][q] = *(const u32x2_t*)((const bf16_t*)p.bias + min(n, p.N - 4));   // columns >= N are never stored
        }
    }
  }
  if constexpr (EPI == FK_EPI_F32DBG) {
    // parity build: fp32(acc + bias) straight from the accumulator registers (a lane owns 4 consecutive columns of a row)
#pragma unroll
    for (int nf = 0; nf < C::NF; ++nf)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = n0 + C::tile_col(wn, nf) + FM::col(lane, q);
        const float b[4] = {bf_lo(bw[nf][q][0]), bf_hi(bw[nf][q][0]), bf_lo(bw[nf][q][1]), bf_hi(bw[nf][q][1])};
#pragma unroll
        for (int mf = MF0; mf < MF1; ++mf) {
          const int m = m0 + C::tile_row(wm, mf) + FM::row(lane, q);
          f32x4_t x = quad_get(acc[nf][mf], q);
          if constexpr (HALF >= 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] += __uint_as_float(other[nf * 2 * C::MF + (mf - MF0) * 4 + q][j]);
          }
          if (m < p.M && n < p.N)
            *(f32x4_t*)((float*)p.C + fk_row_offset(p.c, m) + n) = f32x4_t{x[0] + b[0], x[1] + b[1], x[2] + b[2], x[3] + b[3]};
        }
      }
    return;
  }
  // every wave is done reading the last stage before the C tile aliases it
  if constexpr (WALK) lds_barrier(); else __syncthreads();
  // (WALK: row `row0` of the tile is the first row of the C half-tile)
  bf16_t* ct = WALK ? (bf16_t*)(smem + WALK_CT_OFF) - row0 * C::CT_LD : (bf16_t*)smem;
#pragma unroll
  for (int nf = 0; nf < C::NF; ++nf) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int nl = C::tile_col(wn, nf) + FM::col(lane, q);
      const float b[4] = {bf_lo(bw[nf][q][0]), bf_hi(bw[nf][q][0]), bf_lo(bw[nf][q][1]), bf_hi(bw[nf][q][1])};
#pragma unroll
      for (int mf = MF0; mf < MF1; ++mf) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float x = acc[nf][mf][q * 4 + j];
          if constexpr (ADD_OTHER) x += __uint_as_float(other[nf * 2 * C::MF + (mf - MF0) * 4 + q][j]);
          if constexpr (EPI == FK_EPI_SCALE) v[j] = x * p.alpha;
          else v[j] = x + b[j];
        }
        if constexpr (EPI == FK_EPI_GELU_TANH || EPI == FK_EPI_SILU) {
          // the reference graph rounds the Linear's output to bf16 before the activation
          round_bf_pair(v[0], v[1]);
          round_bf_pair(v[2], v[3]);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = EPI == FK_EPI_GELU_TANH ? gelu_tanh_f(v[j]) : silu_f(v[j]);
        }
        u32x2_t pk;
        pk[0] = pack_bf2(v[0], v[1]);
        pk[1] = pack_bf2(v[2], v[3]);
        const int ml = C::tile_row(wm, mf) + FM::row(lane, q);
        *(u32x2_t*)(ct + ml * C::CT_LD + nl) = pk;
      }
    }
  }
  if constexpr (WALK) lds_barrier(); else __syncthreads();
  // WALK, first pass: the last point of the epilogue with no store in flight -- the next tile's K-tile 0 (requested in front of
  // the epilogue; nothing else is outstanding) has landed before the first store is issued, so that no later wait for it has
  // to count past the stores
  if constexpr (WALK && HALF <= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  constexpr int CPR = BN / 8;  // 16-byte chunks per tile row
  constexpr int ITERS = (HALF >= 0 ? BM / 2 : BM) * CPR / C::NTHREADS;
  // chunks per batch; the fused QKV epilogue keeps 16 table registers per chunk, so the 4-wave kernel (32 chunks per
  // thread, VGPRs full) batches 4 and the 8-wave kernel takes all 8 of a thread's chunks at once
  // (and so do the half-tile forms, which stand twice in their kernel)
  constexpr int U = (EPI == FK_EPI_QKV && (ITERS > 8 || HALF >= 0)) ? 4 : UB;
  static_assert(ITERS % U == 0 && C::NTHREADS % CPR == 0, "epilogue batching");
  // per-tile (scalar) row addressing of the output, the residual and the gate
  constexpr bool HAS_RES = EPI == FK_EPI_GATE_RES || EPI == FK_EPI_RES;
  const bool cflat = flat & 2, rflat = flat & 4, gflat = flat & 8;
  const TileRows crow(p.c, m0, cflat);
  bf16_t* const cbase = (bf16_t*)p.C + crow.first(p.c);
  const TileRows rrow = HAS_RES ? TileRows(p.r, m0, rflat) : crow;
  const bf16_t* const rbase = HAS_RES ? (const bf16_t*)p.res + rrow.first(p.r) : nullptr;
  fk_rows gr = {0, 0, 0};
  if constexpr (EPI == FK_EPI_GATE_RES) gr.rows_per_batch = p.gate_rows_per_batch;
  const TileRows grow(gr, m0, gflat);   // b0 + crossed(ml) = the gate row of tile row ml
  const int D = EPI == FK_EPI_QKV ? p.qkv_heads * 128 : 1;
  const int which = EPI == FK_EPI_QKV ? n0 / D : 0;   // 0 = q, 1 = k, 2 = v: a tile never straddles q | k | v
  // a thread keeps its chunk column over the iterations (NTHREADS % CPR == 0): only the row advances
  const int cc = tid % CPR, ml0 = row0 + tid / CPR;
  constexpr int ML_STEP = C::NTHREADS / CPR;
  const int n = n0 + cc * 8;
  const int nc = min(n, p.N - 8);          // clamped column for the unconditional loads
  const int mlast = p.M - 1 - m0;          // last valid tile row

  if (EPI == FK_EPI_QKV && which < 2) {
    // 16 consecutive lanes hold one 128-wide head row of the tile: RMSNorm (weight) + interleaved-pair RoPE, then
    // the head-major [B, H, S_total, 128] layout
    const int hn = n - which * D;              // column inside q or k
    const int head = hn >> 7, dch = hn & 127;  // dch = 8 * chunk-in-head
    const u32x4_t ww = *(const u32x4_t*)((const bf16_t*)(which == 0 ? p.wq : p.wk) + dch);
    bf16_t* const dst = (bf16_t*)(which == 0 ? p.q_out : p.k_out);
#pragma unroll
    for (int j0 = 0; j0 < ITERS; j0 += U) {
      u32x4_t y[U];
      f32x4_t t0[U], t1[U];   // (cos, sin) of the chunk's four rotary pairs
      int srow[U], bidx[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int ml = ml0 + ML_STEP * (j0 + u);
        y[u] = *(const u32x4_t*)(ct + ml * C::CT_LD + cc * 8);
        // token of row m: batch = m / rows_per_batch (one batch when c.rows_per_batch <= 0), s = s_offset + m % rows_per_batch
        const int mlc = min(ml, mlast);
        const int nb = crow.crossed(mlc);
        bidx[u] = crow.b0 + nb;
        srow[u] = p.qkv_s_offset + crow.r0 + mlc - nb * crow.rpb;
        const float* tp = p.rope_cs + (int64_t)srow[u] * 128 + dch;   // pair dch/2 + e at floats 2e, 2e + 1
        t0[u] = *(const f32x4_t*)tp;
        t1[u] = *(const f32x4_t*)(tp + 4);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int ml = ml0 + ML_STEP * (j0 + u);
        float xv[8];
        float ss = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          xv[2 * e] = bf_lo(y[u][e]);
          xv[2 * e + 1] = bf_hi(y[u][e]);
          ss += xv[2 * e] * xv[2 * e] + xv[2 * e + 1] * xv[2 * e + 1];
        }
        ss = row16_sum(ss);
        const float rs = __builtin_amdgcn_rsqf(ss * (1.0f / 128) + 1e-6f);   // argument >= 1e-6: no denormal scaling
        const float cs[4] = {t0[u][0], t0[u][2], t1[u][0], t1[u][2]};
        const float sn[4] = {t0[u][1], t0[u][3], t1[u][1], t1[u][3]};
        u32x4_t ow;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float re = xv[2 * e] * rs, im = xv[2 * e + 1] * rs;
          round_bf_pair(re, im);
          re *= bf_lo(ww[e]);
          im *= bf_hi(ww[e]);
          round_bf_pair(re, im);
          // the same two rounded products and one sum as qkv_post_kernel (FK_EPI_QKV is held bit-identical to it)
          const float o0 = mul2_add(re, cs[e], -im, sn[e]);
          const float o1 = mul2_add(im, cs[e], re, sn[e]);
          ow[e] = pack_bf2(o0, o1);
        }
        // head-major row index in 32 bits (the launcher checks batches * heads * s_total < 2^31)
        const int hrow = (bidx[u] * p.qkv_heads + head) * p.qkv_s_total + srow[u];
        if (ml <= mlast && n < p.N) *(u32x4_t*)(dst + (int64_t)hrow * 128 + dch) = ow;
      }
    }
    return;
  }

#pragma unroll
  for (int j0 = 0; j0 < ITERS; j0 += U) {
    u32x4_t y[U], rv[U], gv[U];
    int coff[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ml = ml0 + ML_STEP * (j0 + u);
      const int mlc = min(ml, mlast);
      y[u] = *(const u32x4_t*)(ct + ml * C::CT_LD + cc * 8);
      coff[u] = crow.off(mlc) + n;
      if constexpr (EPI == FK_EPI_GATE_RES || EPI == FK_EPI_RES) rv[u] = *(const u32x4_t*)(rbase + rrow.off(mlc) + nc);
      if constexpr (EPI == FK_EPI_GATE_RES) {
        const int64_t b = grow.b0 + grow.crossed(mlc);
        gv[u] = *(const u32x4_t*)((const bf16_t*)p.gate + b * p.gate_batch_stride + nc);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ml = ml0 + ML_STEP * (j0 + u);
      u32x4_t o = y[u];
      if constexpr (EPI == FK_EPI_GATE_RES || EPI == FK_EPI_RES) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float y0 = bf_lo(o[e]), y1 = bf_hi(o[e]);
          if constexpr (EPI == FK_EPI_GATE_RES) {
            y0 *= bf_lo(gv[u][e]);
            y1 *= bf_hi(gv[u][e]);
            round_bf_pair(y0, y1);
          }
          o[e] = pack_bf2(bf_lo(rv[u][e]) + y0, bf_hi(rv[u][e]) + y1);
        }
      }
      if (ml <= mlast && n < p.N) *(u32x4_t*)(cbase + coff[u]) = o;
    }
  }
}

// Quantized-output epilogue (gemm_mxfp8.hip: gemm_mxq_kernel): the tile goes to
// LDS as bf16 exactly as store_tile puts it there -- bias, bf16 rounding of the Linear's output in front of the activation, bf16
// rounding of the result: the existing rounding points -- and every 32-column block of a row then leaves as 32 e4m3 bytes plus
// one E8M0 byte, the bytes fk_quantize_mxfp8 gives for the bf16 tile store_tile would have written.  Nothing is stored as
// bf16.  A thread owns one block per iteration: row m at q + m * ldq + n (q / s are already advanced to the caller's column
// window; N % 256 == 0, so only rows are predicated); the BN / 32 threads of a tile row write BN consecutive bytes.
template <int EPI, int BN, class C>
FK_DEV void store_tile_mxq(const f32x16_t (&acc)[C::NF][C::MF], const fk_gemm_args& p, uint8_t* __restrict__ q,
                           uint8_t* __restrict__ s, int64_t ldq, int64_t ld_scale, char* smem, int m0, int n0, int wm, int wn) {
  static_assert(EPI == FK_EPI_NONE || EPI == FK_EPI_GELU_TANH, "quantized output: plain and GELU epilogues");
  const int tid = threadIdx.x, lane = tid & 63;
  using FM = FragMap<C::M16>;
  u32x2_t bw[C::NF][4];
#pragma unroll
  for (int nf = 0; nf < C::NF; ++nf)
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) bw[nf][qd] = u32x2_t{0u, 0u};
  if (p.bias) {
#pragma unroll
    for (int nf = 0; nf < C::NF; ++nf)
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        const int n = n0 + C::tile_col(wn, nf) + FM::col(lane, qd);
        bw[nf][qd] = *(const u32x2_t*)((const bf16_t*)p.bias + min(n, p.N - 4));
      }
  }
  __syncthreads();  // every wave is done reading the last stage before the C tile aliases it
  bf16_t* ct = (bf16_t*)smem;
#pragma unroll
  for (int nf = 0; nf < C::NF; ++nf) {
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const int nl = C::tile_col(wn, nf) + FM::col(lane, qd);
      const float b[4] = {bf_lo(bw[nf][qd][0]), bf_hi(bw[nf][qd][0]), bf_lo(bw[nf][qd][1]), bf_hi(bw[nf][qd][1])};
#pragma unroll
      for (int mf = 0; mf < C::MF; ++mf) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = acc[nf][mf][qd * 4 + j] + b[j];
        if constexpr (EPI == FK_EPI_GELU_TANH) {
          round_bf_pair(v[0], v[1]);
          round_bf_pair(v[2], v[3]);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = gelu_tanh_f(v[j]);
        }
        u32x2_t pk;
        pk[0] = pack_bf2(v[0], v[1]);
        pk[1] = pack_bf2(v[2], v[3]);
        const int ml = C::tile_row(wm, mf) + FM::row(lane, qd);
        *(u32x2_t*)(ct + ml * C::CT_LD + nl) = pk;
      }
    }
  }
  __syncthreads();
  constexpr int BPR = BN / 32;                      // 32-column blocks per tile row
  constexpr int ITERS = BM * BPR / C::NTHREADS;
  constexpr int ML_STEP = C::NTHREADS / BPR;
  static_assert(C::NTHREADS % BPR == 0 && (BM * BPR) % C::NTHREADS == 0, "quantized epilogue tiling");
  const int bc = tid % BPR, ml0 = tid / BPR;
  const int mlast = p.M - 1 - m0;                   // last valid tile row
#pragma unroll
  for (int j = 0; j < ITERS; ++j) {
    const int ml = ml0 + ML_STEP * j;
    const u32x4_t* src = (const u32x4_t*)(ct + ml * C::CT_LD + bc * 32);
    uint32_t w[16], out[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const u32x4_t v = src[i];
      w[4 * i] = v[0]; w[4 * i + 1] = v[1]; w[4 * i + 2] = v[2]; w[4 * i + 3] = v[3];
    }
    const uint32_t sbyte = mx_quant_block(w, out);
    if (ml <= mlast) {
      const int64_t m = (int64_t)m0 + ml;
      u32x4_t* dst = (u32x4_t*)(q + m * ldq + n0 + bc * 32);
      dst[0] = u32x4_t{out[0], out[1], out[2], out[3]};
      dst[1] = u32x4_t{out[4], out[5], out[6], out[7]};
      s[m * ld_scale + (n0 >> 5) + bc] = (uint8_t)sbyte;
    }
  }
}
