// LoRA gradient projection (train_step.py: DenoiserTrainStep(lora=...)): the chain rule through the merge
//   W = bf16(W_base + s * up . down)            (lora_merge.hip; up = lora_B [N, r], down = lora_A [r, K])
// carries the weight gradient dW [N, K] (bf16, what the backward's wgrad GEMM wrote) onto the two factors, straight through
// the merge's one bf16 rounding:
//   d_up  [n, j] = s * sum_k dW[n, k] * down[j, k]        reduces over K
//   d_down[j, k] = s * sum_n up[n, j] * dW[n, k]          reduces over N
// Outputs fp32, contiguous.  Products on v_mfma_f32_16x16x32_bf16 with fp32 accumulation; the rank is zero-padded to
// r_pad = 32 * ceil(r / 32) (output tiles of 16), the reduction index to the step of its role (32 k / 64 n); `scale` multiplies
// the finished fp32 sum once.  HBM traffic: dW is read twice (once per role) = 4 B per weight element, the factors and the
// partials are small; 4 N K r_pad flops.
//
// Decomposition: ONE launch of `lora_grad_kernel` whose workgroups (4 waves) take one of two roles by block index, then --
// only when a role was split -- one launch of `lora_grad_reduce_kernel`.
//   role UP    a workgroup owns LG_UP_ROWS = 64 rows n (16 per wave) and one chunk [k_b, k_e) of K, walked in steps of 32 k.
//              The reduction index k is contiguous in dW's and in down's rows, which is what an MFMA operand fragment wants
//              (8 consecutive k per lane = one 16-byte load): both operands come straight from global memory, no LDS.  A = dW
//              (rows n), B = down^T (columns j); r_pad / 16 accumulators per wave.  The four waves of a workgroup read the same
//              down fragments (L1 / L2: down is at most 768 KB).
//   role DOWN  a workgroup owns LG_DN_COLS = 128 columns k (32 per wave) and one chunk [n_b, n_e) of N, walked in steps of
//              LG_DN_STEP = 64 n.  Here the reduction index n is the ROW index of both dW and up: each step stages the dW tile
//              [64 n x 128 k] and up's [64 n x r_pad] into LDS TRANSPOSED ([k][n] and [j][n], as lora_merge.hip stages down),
//              then A = up^T (rows j), B = dW (columns k); 2 * r_pad / 16 accumulators per wave.
// Occupancy.  One workgroup per 64-row strip would leave a 3072-row weight on 48 of 256 CUs, so each role's reduction is
// SPLIT into chunks: with strips = the role's strip count, granules = ceil(L / granule) (granule: LG_UP_GRAN = 256 k,
// LG_DN_GRAN = 128 n), want = ceil(256 / strips):  chunk = ceil(granules / want) granules,  splits = ceil(granules / chunk).
// At [3072, 3072]: UP 48 strips x 6 chunks of 512 k, DOWN 24 strips x 8 chunks of 384 n = 480 workgroups in the one launch.
// A role with splits == 1 writes scale * acc to its output itself.  A split role writes its unscaled fp32 partials to the
// caller's workspace ([split][N][r] and [split][r][K]; fk_lora_grad_ws_floats) and the reduce kernel forms
// scale * (p_0 + p_1 + ... ) in ascending split order, one thread per output element.
// No atomics: every output element is written once, by a sum whose order (MFMA order inside a step, steps ascending, splits
// ascending) is fixed by (N, K, r) alone -- two launches give the same bits.  dW, up and down are only read.
// Accumulate form (fk_lora_grad_acc_bf16, accumulate = 1; gradient accumulation over micro-batches): out = out_old + scale * sum.
// The add sits where the scaled value is formed -- the final store of an unsplit role, the reduce kernel of a split one -- so the
// thread that owns an element reads it once and writes it once; partials are never added to, still no atomics, the order still
// fixed by (N, K, r).  accumulate = 0 never reads the outputs (they may hold NaN bits) and is the code fk_lora_grad_bf16 runs.
// Views that are not 16-byte aligned (pointer or row stride), and row tails, take the same kernels with element-wise loads.
// First shapes that cross each boundary: N = 65 second UP strip; K = 33 second UP step; K = 257 second UP chunk (a partial);
// K = 129 second DOWN strip; N = 65 second DOWN step; N = 129 second DOWN chunk (a partial).
#include "fk_common.h"

namespace {

constexpr int LG_THREADS = 256;
constexpr int LG_UP_ROWS = 64;                       // role UP: rows n of a workgroup, 16 per wave
constexpr int LG_UP_STEP = 32;                       //          k per MFMA step
constexpr int LG_UP_GRAN = 256;                      //          k granule of a split
constexpr int LG_DN_COLS = 128;                      // role DOWN: columns k of a workgroup, 32 per wave
constexpr int LG_DN_STEP = 64;                       //            n staged per step (two MFMA steps of 32)
constexpr int LG_DN_GRAN = 128;                      //            n granule of a split
constexpr int LG_LDS_LD = LG_DN_STEP + 8;            // elements per LDS row: 144 B, rows 16-byte aligned, 4 banks apart
constexpr int LG_TARGET_WGS = 256;                   // workgroups a role aims at: one per CU

struct Plan {
  int64_t strips_up, splits_up, chunk_up;            // chunk in k
  int64_t strips_dn, splits_dn, chunk_dn;            // chunk in n
};

void split_of(int64_t L, int64_t gran, int64_t strips, int64_t* splits, int64_t* chunk) {
  const int64_t granules = (L + gran - 1) / gran;
  const int64_t want = (LG_TARGET_WGS + strips - 1) / strips;
  const int64_t cg = (granules + want - 1) / want;
  *splits = (granules + cg - 1) / cg;
  *chunk = cg * gran;
}

Plan plan_of(int64_t N, int64_t K) {
  Plan p;
  p.strips_up = (N + LG_UP_ROWS - 1) / LG_UP_ROWS;
  p.strips_dn = (K + LG_DN_COLS - 1) / LG_DN_COLS;
  split_of(K, LG_UP_GRAN, p.strips_up, &p.splits_up, &p.chunk_up);
  split_of(N, LG_DN_GRAN, p.strips_dn, &p.splits_dn, &p.chunk_dn);
  return p;
}

struct GradArgs {
  const bf16_t* dw; int64_t ld_dw;
  const bf16_t* up; int64_t ld_up;
  const bf16_t* down; int64_t ld_down;
  int32_t N, K, rank;
  float scale;
  float* out_up;                                     // d_up (splits_up == 1) or the UP partials [split][N][rank]
  float* out_dn;                                     // d_down (splits_dn == 1) or the DOWN partials [split][rank][K]
  int32_t up_blocks;                                 // blocks [0, up_blocks) take role UP
  int32_t splits_up, chunk_up, splits_dn, chunk_dn;
  int32_t vec_dw, vec_up, vec_down;                  // 16-byte loads allowed (pointer % 16 == 0 and row stride % 8 == 0)
  int32_t accumulate;                                // 1: an unsplit role adds its scaled sum to what its output holds
};

// elements [k, k + 8) of a row of `len` elements (k % 8 == 0) as an MFMA operand fragment; zeros beyond the row or when !ok
FK_DEV bf16x8_t load_frag(const bf16_t* row, int64_t k, int64_t len, bool ok, int vec) {
  u32x4_t w = {0u, 0u, 0u, 0u};
  if (ok && k < len) {
    if (vec && k + 8 <= len) {
      w = *(const u32x4_t*)(row + k);
    } else {
      uint32_t e[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) e[q] = k + q < len ? (uint32_t)row[k + q] : 0u;
#pragma unroll
      for (int q = 0; q < 4; ++q) w[q] = e[2 * q] | (e[2 * q + 1] << 16);
    }
  }
  return __builtin_bit_cast(bf16x8_t, w);
}

// rows [r0, r0 + LG_DN_STEP) x columns [c0, c0 + ncols) of a [rows_total, cols_total] matrix -> lds[col - c0][row - r0]
// (transposed); zeros outside the matrix.  ncols % 8 == 0, c0 % 8 == 0.
FK_DEV void stage_transposed(bf16_t* lds, const bf16_t* src, int64_t ld, int64_t r0, int64_t rows_total, int64_t c0,
                             int64_t cols_total, int ncols, int vec) {
  // 32 consecutive lanes take 32 consecutive rows of one 8-column chunk: their 2-byte LDS writes fall into 16 consecutive banks
  const int cpr = ncols / 8;
  for (int i = threadIdx.x; i < LG_DN_STEP * cpr; i += LG_THREADS) {
    const int blk = i >> 5;
    const int c = (blk % cpr) * 8, nn = (blk / cpr) * 32 + (i & 31);
    const int64_t row = r0 + nn, col = c0 + c;
    uint32_t e[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) e[q] = 0u;
    if (row < rows_total && col < cols_total) {
      const bf16_t* p = src + row * ld + col;
      if (vec && col + 8 <= cols_total) {
        const u32x4_t w = *(const u32x4_t*)p;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          e[2 * q] = w[q] & 0xffffu;
          e[2 * q + 1] = w[q] >> 16;
        }
      } else {
#pragma unroll
        for (int q = 0; q < 8; ++q)
          if (col + q < cols_total) e[q] = (uint32_t)p[q];
      }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) lds[(c + q) * LG_LDS_LD + nn] = (bf16_t)e[q];
  }
}

// RT: output tiles of 16 ranks = r_pad / 16 (2, 4, 6 or 8)
template <int RT>
__global__ __launch_bounds__(LG_THREADS) void lora_grad_kernel(GradArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t s_dw[LG_DN_COLS * LG_LDS_LD];     // [k][n]
  __shared__ __attribute__((aligned(16))) bf16_t s_up[RT * 16 * LG_LDS_LD];        // [j][n]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int64_t N = a.N, K = a.K;
  const int rank = a.rank;

  if ((int)blockIdx.x < a.up_blocks) {
    // ---- role UP: d_up[n, j] over k in [k_b, k_e)
    const int strip = blockIdx.x / a.splits_up, sp = blockIdx.x - strip * a.splits_up;
    const int64_t n_row = (int64_t)strip * LG_UP_ROWS + wave * 16;       // the wave's first row
    const int64_t n = n_row + l15;                                       // A operand: the lane's row of dW
    const int64_t k_b = (int64_t)sp * a.chunk_up;
    const int64_t k_e = k_b + a.chunk_up < K ? k_b + a.chunk_up : K;
    const bf16_t* dw_row = a.dw + (n < N ? n : 0) * a.ld_dw;
    f32x4_t acc[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) acc[t] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
    if (n_row < N) {                                                     // wave-uniform: a wave with no row does nothing
      for (int64_t k = k_b; k < k_e; k += LG_UP_STEP) {
        // A[row = n][kk] = dW[n][k + kk]: lane (row = l15) holds kk = 8 lg + [0, 8)
        const bf16x8_t fa = load_frag(dw_row, k + 8 * lg, K, n < N, a.vec_dw);
#pragma unroll
        for (int t = 0; t < RT; ++t) {
          // B[kk][col = j] = down[j][k + kk]: lane (col = l15) holds the same 8 kk of row j = 16 t + l15
          const int j = 16 * t + l15;
          const bf16x8_t fb = load_frag(a.down + (int64_t)(j < rank ? j : 0) * a.ld_down, k + 8 * lg, K, j < rank, a.vec_down);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc[t], 0, 0, 0);
        }
      }
    }
    // D[row][col]: row = 4 lg + reg -> n, col = l15 -> j
    const bool final_ = a.splits_up == 1;
    float* out = a.out_up + (final_ ? 0 : (int64_t)sp * N * rank);
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int j = 16 * t + l15;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t nr = n_row + 4 * lg + e;
        if (nr < N && j < rank) {
          float v = final_ ? a.scale * acc[t][e] : acc[t][e];
          if (final_ && a.accumulate) v += out[nr * rank + j];
          out[nr * rank + j] = v;
        }
      }
    }
    return;
  }

  // ---- role DOWN: d_down[j, k] over n in [n_b, n_e)
  const int tile = blockIdx.x - a.up_blocks;
  const int strip = tile / a.splits_dn, sp = tile - strip * a.splits_dn;
  const int64_t k0 = (int64_t)strip * LG_DN_COLS;
  const int64_t n_b = (int64_t)sp * a.chunk_dn;
  const int64_t n_e = n_b + a.chunk_dn < N ? n_b + a.chunk_dn : N;
  f32x4_t acc[RT][2];
#pragma unroll
  for (int t = 0; t < RT; ++t) acc[t][0] = acc[t][1] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
  for (int64_t n0 = n_b; n0 < n_e; n0 += LG_DN_STEP) {
    __syncthreads();                                  // the previous step's fragments have been read
    stage_transposed(s_dw, a.dw, a.ld_dw, n0, N, k0, K, LG_DN_COLS, a.vec_dw);
    stage_transposed(s_up, a.up, a.ld_up, n0, N, 0, rank, RT * 16, a.vec_up);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < LG_DN_STEP; c += 32) {
      // B[nn][col = k] = dW[n0 + nn][k0 + 32 wave + 16 h + col]: lane (col = l15) holds nn = c + 8 lg + [0, 8)
      bf16x8_t fb[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) fb[h] = *(const bf16x8_t*)(s_dw + (wave * 32 + h * 16 + l15) * LG_LDS_LD + c + 8 * lg);
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        // A[row = j][nn] = up[n0 + nn][16 t + row]: lane (row = l15) holds the same 8 nn
        const bf16x8_t fa = *(const bf16x8_t*)(s_up + (t * 16 + l15) * LG_LDS_LD + c + 8 * lg);
#pragma unroll
        for (int h = 0; h < 2; ++h) acc[t][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb[h], acc[t][h], 0, 0, 0);
      }
    }
  }
  // D[row][col]: row = 4 lg + reg -> j, col = l15 -> k
  const bool final_ = a.splits_dn == 1;
  float* out = a.out_dn + (final_ ? 0 : (int64_t)sp * rank * K);
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t k = k0 + wave * 32 + h * 16 + l15;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = 16 * t + 4 * lg + e;
        if (j < rank && k < K) {
          float v = final_ ? a.scale * acc[t][h][e] : acc[t][h][e];
          if (final_ && a.accumulate) v += out[(int64_t)j * K + k];
          out[(int64_t)j * K + k] = v;
        }
      }
    }
}

// out[i] = scale * (p[0][i] + p[1][i] + ...) (+ out[i] when accumulate), splits ascending; elements [0, n_up) are d_up's, the
// next n_dn are d_down's
__global__ __launch_bounds__(LG_THREADS) void lora_grad_reduce_kernel(const float* p_up, int splits_up, int64_t n_up, float* d_up,
                                                                      const float* p_dn, int splits_dn, int64_t n_dn, float* d_down,
                                                                      float scale, int accumulate) {
  int64_t i = (int64_t)blockIdx.x * LG_THREADS + threadIdx.x;
  const float* p;
  float* out;
  int splits;
  int64_t n;
  if (i < n_up) {
    p = p_up, out = d_up, splits = splits_up, n = n_up;
  } else {
    i -= n_up;
    if (i >= n_dn) return;
    p = p_dn, out = d_down, splits = splits_dn, n = n_dn;
  }
  float v = p[i];
  for (int s = 1; s < splits; ++s) v += p[(int64_t)s * n + i];
  v *= scale;
  if (accumulate) v += out[i];
  out[i] = v;
}

struct Span { uintptr_t lo, hi; };                     // [lo, hi) in bytes
Span span_of(const void* p, int64_t ld, int64_t rows, int64_t cols, size_t elem) {
  const uintptr_t lo = (uintptr_t)p;
  return Span{lo, lo + (uintptr_t)((rows - 1) * ld + cols) * elem};
}
bool overlap(const Span& x, const Span& y) { return x.lo < y.hi && y.lo < x.hi; }

int64_t ws_floats_of(const Plan& p, int64_t N, int64_t K, int64_t rank) {
  return (p.splits_up > 1 ? p.splits_up * N * rank : 0) + (p.splits_dn > 1 ? p.splits_dn * rank * K : 0);
}

}  // namespace

extern "C" int64_t fk_lora_grad_ws_floats(int32_t N, int32_t K, int32_t rank) {
  if (N < 1 || K < 1 || rank < 1 || rank > FK_LORA_MAX_RANK) return 0;
  return ws_floats_of(plan_of(N, K), N, K, rank);
}

namespace {

// `fn`: the entry point's name, the prefix of every error message
int lora_grad_launch(const char* fn, const void* dw, int64_t ld_dw, const void* up, int64_t ld_up, const void* down, int64_t ld_down,
                     int32_t N, int32_t K, int32_t rank, float scale, float* d_up, float* d_down, int32_t accumulate, float* ws,
                     int64_t ws_floats, fk_stream_t stream) {
  FK_CHECK_ARG(dw && up && down && d_up && d_down, "%s: NULL pointer", fn);
  FK_CHECK_ARG(N >= 1 && K >= 1, "%s: needs N >= 1 and K >= 1 (N = %d, K = %d)", fn, N, K);
  if (rank < 1 || rank > FK_LORA_MAX_RANK) {
    fk_set_error("%s: rank %d, supported 1 to %d", fn, rank, FK_LORA_MAX_RANK);
    return FK_EUNSUPPORTED;
  }
  FK_CHECK_ARG(ld_dw >= K && ld_up >= rank && ld_down >= K, "%s: a row stride below the row length (ld_dw = %lld, "
               "ld_down = %lld, K = %d, ld_up = %lld, rank = %d)", fn, (long long)ld_dw, (long long)ld_down, K, (long long)ld_up, rank);
  FK_CHECK_ARG(scale == scale && scale - scale == 0.0f, "%s: the scale is not finite", fn);
  FK_CHECK_ARG(accumulate == 0 || accumulate == 1, "%s: accumulate is %d, it must be 0 (overwrite) or 1 (add)", fn, accumulate);
  const Plan p = plan_of(N, K);
  const int64_t need = ws_floats_of(p, N, K, rank);
  FK_CHECK_ARG(need == 0 || (ws && ws_floats >= need), "%s: the workspace holds %lld floats, [%d, %d] at rank %d "
               "needs %lld (fk_lora_grad_ws_floats)", fn, (long long)(ws ? ws_floats : 0), N, K, rank, (long long)need);
  const Span in[3] = {span_of(dw, ld_dw, N, K, 2), span_of(up, ld_up, N, rank, 2), span_of(down, ld_down, rank, K, 2)};
  const Span o_up = span_of(d_up, rank, N, rank, 4), o_dn = span_of(d_down, K, rank, K, 4);
  const Span o_ws = span_of(ws, need, 1, need, 4);
  FK_CHECK_ARG(!overlap(o_up, o_dn), "%s: d_up overlaps d_down", fn);
  for (int i = 0; i < 3; ++i)
    FK_CHECK_ARG(!overlap(o_up, in[i]) && !overlap(o_dn, in[i]) && (need == 0 || !overlap(o_ws, in[i])),
                 "%s: an output or the workspace overlaps an input", fn);
  FK_CHECK_ARG(need == 0 || (!overlap(o_ws, o_up) && !overlap(o_ws, o_dn)), "%s: the workspace overlaps an output", fn);
  const int64_t up_blocks = p.strips_up * p.splits_up, dn_blocks = p.strips_dn * p.splits_dn;
  if (up_blocks + dn_blocks > 0x7fffffffLL) {
    fk_set_error("%s: %lld + %lld workgroups exceed one grid", fn, (long long)up_blocks, (long long)dn_blocks);
    return FK_EUNSUPPORTED;
  }
  GradArgs a;
  a.dw = (const bf16_t*)dw, a.ld_dw = ld_dw, a.up = (const bf16_t*)up, a.ld_up = ld_up;
  a.down = (const bf16_t*)down, a.ld_down = ld_down;
  a.N = N, a.K = K, a.rank = rank, a.scale = scale;
  float* part_up = ws;
  float* part_dn = ws + (p.splits_up > 1 ? p.splits_up * (int64_t)N * rank : 0);
  a.out_up = p.splits_up > 1 ? part_up : d_up;
  a.out_dn = p.splits_dn > 1 ? part_dn : d_down;
  a.up_blocks = (int32_t)up_blocks;
  a.splits_up = (int32_t)p.splits_up, a.chunk_up = (int32_t)p.chunk_up;
  a.splits_dn = (int32_t)p.splits_dn, a.chunk_dn = (int32_t)p.chunk_dn;
  a.vec_dw = (uintptr_t)dw % 16 == 0 && ld_dw % 8 == 0;
  a.vec_up = (uintptr_t)up % 16 == 0 && ld_up % 8 == 0;
  a.vec_down = (uintptr_t)down % 16 == 0 && ld_down % 8 == 0;
  a.accumulate = accumulate;
  const dim3 grid((unsigned)(up_blocks + dn_blocks)), block(LG_THREADS);
  switch ((rank + 31) / 32) {
    case 1: hipLaunchKernelGGL(lora_grad_kernel<2>, grid, block, 0, (hipStream_t)stream, a); break;
    case 2: hipLaunchKernelGGL(lora_grad_kernel<4>, grid, block, 0, (hipStream_t)stream, a); break;
    case 3: hipLaunchKernelGGL(lora_grad_kernel<6>, grid, block, 0, (hipStream_t)stream, a); break;
    default: hipLaunchKernelGGL(lora_grad_kernel<8>, grid, block, 0, (hipStream_t)stream, a); break;
  }
  FK_CHECK_LAUNCH(fn);
  if (need > 0) {
    const int64_t n_up = p.splits_up > 1 ? (int64_t)N * rank : 0, n_dn = p.splits_dn > 1 ? (int64_t)rank * K : 0;
    const int64_t blocks = (n_up + n_dn + LG_THREADS - 1) / LG_THREADS;
    hipLaunchKernelGGL(lora_grad_reduce_kernel, dim3((unsigned)blocks), block, 0, (hipStream_t)stream, part_up, (int)p.splits_up,
                       n_up, d_up, part_dn, (int)p.splits_dn, n_dn, d_down, scale, (int)accumulate);
    FK_CHECK_LAUNCH(fn);
  }
  return FK_OK;
}

}  // namespace

extern "C" int fk_lora_grad_bf16(const void* dw, int64_t ld_dw, const void* up, int64_t ld_up, const void* down, int64_t ld_down,
                                 int32_t N, int32_t K, int32_t rank, float scale, float* d_up, float* d_down, float* ws,
                                 int64_t ws_floats, fk_stream_t stream) {
  return lora_grad_launch("fk_lora_grad_bf16", dw, ld_dw, up, ld_up, down, ld_down, N, K, rank, scale, d_up, d_down, 0, ws, ws_floats,
                          stream);
}

extern "C" int fk_lora_grad_acc_bf16(const void* dw, int64_t ld_dw, const void* up, int64_t ld_up, const void* down, int64_t ld_down,
                                     int32_t N, int32_t K, int32_t rank, float scale, float* d_up, float* d_down, int32_t accumulate,
                                     float* ws, int64_t ws_floats, fk_stream_t stream) {
  return lora_grad_launch("fk_lora_grad_acc_bf16", dw, ld_dw, up, ld_up, down, ld_down, N, K, rank, scale, d_up, d_down, accumulate, ws,
                          ws_floats, stream);
}
