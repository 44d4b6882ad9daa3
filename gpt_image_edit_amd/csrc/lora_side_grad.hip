// Factored LoRA gradient (train_step.py: DenoiserTrainStep(lora=..., lora_backward="factored")): the adapter gradient of a
// linear y = x W^T, W = bf16(W_base + s * up . down), taken from the linear's own backward operands X [M, K] and dY [M, N]
// (bf16 views, M = B * R rows) WITHOUT the weight gradient dW = dY^T X [N, K] (lora_grad.hip projects that one):
//   d_up  [n, j] = s * sum_m dY[m, n] * T[m, j]      T = X down^T   [M, r]
//   d_down[j, k] = s * sum_m U[m, j]  * X[m, k]      U = dY up      [M, r]
// 4 M r_pad (N + K) flops instead of 2 M N K; X and dY are read twice each.  Outputs fp32, contiguous.  All products on
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation; the rank is zero-padded to r_pad = 32 * ceil(r / 32), every reduction index
// to the step of its role; `scale` multiplies the finished fp32 sum once.
//
// Stage 1, ONE launch of `lora_side_stage1_kernel`: a workgroup (4 waves) owns LS_ROWS = 64 rows m (16 per wave) and the whole
// reduction of one of two roles by block index.
//   role T   T[m, j] = sum_k X[m, k] down[j, k], k in steps of 32.  k is contiguous in X's and down's rows: both fragments come
//            straight from global memory (role UP of lora_grad.hip).  A = X (rows m), B = down^T (columns j).
//   role U   U[m, j] = sum_n dY[m, n] up[n, j], n in steps of LS_U_STEP = 64.  n is the ROW index of up: each step stages up's
//            [64 n x r_pad] into LDS transposed ([j][n], as lora_merge.hip / lora_grad.hip do); A = dY (rows m) from global memory.
// Each fp32 value t leaves as a bf16 pair hi = bf16(t), lo = bf16(t - hi) (the subtraction is exact, |t - hi - lo| <= 2^-18 |t|),
// stored TRANSPOSED in the workspace, [r_pad][M_pad] with M_pad = 64 * ceil(M / 64): a lane's four accumulator rows are four
// consecutive m of one j, one 8-byte store.  Rows j >= r and columns m >= M are written as zeros, so stage 2 reads them unmasked.
// Stage 2, ONE launch of `lora_side_stage2_kernel`, reduces over m -- the row index of X and dY, and (because of the transposed
// store) the contiguous index of T^T and U^T.  A workgroup owns LS_COLS = 128 output columns (32 per wave) and one chunk
// [m_b, m_e) of M, walked in steps of LS_M_STEP = 64 m; each step stages the [64 m x 128] tile of dY (role UP) or X (role DOWN)
// into LDS transposed ([col][m], role DOWN of lora_grad.hip), the T^T / U^T fragments are 16-byte global loads:
//   role UP    d_up^T[j, n]  = sum_m T^T[j, m] dY[m, n]     A = T^T (rows j), B = dY (columns n); stored as d_up[n, j]
//   role DOWN  d_down[j, k]  = sum_m U^T[j, m] X[m, k]      A = U^T (rows j), B = X  (columns k)
// hi and lo are two MFMA terms into the same accumulator (the split-bf16 form): 2 * 2 * r_pad / 16 MFMAs per wave and 32 m.
// Occupancy: the m reduction of stage 2 is SPLIT as lora_grad.hip's plan_of splits: strips = ceil(L / 128) (L = N or K),
// granules = ceil(M / LS_M_GRAN = 128), want = ceil(256 / strips), chunk = ceil(granules / want) granules, splits =
// ceil(granules / chunk).  [3072, 3072] at M = 8704: 24 strips x 10 chunks of 896 m per role = 480 workgroups; stage 1 has
// 2 * 136.  A role with splits == 1 writes scale * acc (+ the old value when accumulate) itself; a split role writes unscaled
// fp32 partials ([split][N][r] / [split][r][K]) and `lora_side_reduce_kernel` forms scale * (p_0 + p_1 + ...) in ascending split
// order, one thread per element, adding the old value there when accumulate = 1.  Three launches at most.
// No atomics: every element is written once by its owner, the order (MFMA order inside a step, steps ascending, hi before lo,
// splits ascending) is fixed by (B, R, N, K, r) alone -- two launches give the same bits.  accumulate = 0 never reads the outputs.
// Workspace (fk_lora_side_grad_ws_floats): [UP partials][DOWN partials][<= 3 floats to a 16-byte boundary][T^T hi, T^T lo,
// U^T hi, U^T lo: r_pad * M_pad bf16 each].  Views that are not 16-byte aligned (pointer, row or batch stride) and row tails
// take the same kernels with element-wise loads.
// First shapes that cross each boundary.  Stage 1: M = 65 second strip (both roles; stage 1 has no chunks); K = 33 second step
// of role T; N = 65 second step of role U.  Stage 2: N = 129 second strip of role UP, K = 129 second strip of role DOWN;
// M = 65 second step and M = 129 second chunk (a partial) of both roles.  r = 33 second pair of rank tiles.
#include "fk_common.h"

namespace {

constexpr int LS_THREADS = 256;
constexpr int LS_ROWS = 64;                          // stage 1: rows m of a workgroup, 16 per wave
constexpr int LS_T_STEP = 32;                        //          role T: k per MFMA step
constexpr int LS_U_STEP = 64;                        //          role U: n staged per step (two MFMA steps of 32)
constexpr int LS_COLS = 128;                         // stage 2: output columns of a workgroup, 32 per wave
constexpr int LS_M_STEP = 64;                        //          m staged per step
constexpr int LS_M_GRAN = 128;                       //          m granule of a split
constexpr int LS_LDS_LD = 64 + 8;                    // elements per LDS row: 144 B, rows 16-byte aligned, 4 banks apart
constexpr int LS_TARGET_WGS = 256;                   // workgroups a stage-2 role aims at: one per CU

struct View {                                        // [B, R, cols] bf16, last dimension contiguous
  const bf16_t* p;
  int64_t ld, bs;
  int32_t vec;                                       // 16-byte loads allowed (pointer % 16 == 0, ld % 8 == 0, bs % 8 == 0)
};

FK_DEV const bf16_t* row_of(const View& v, int32_t m, int32_t R) {
  const int32_t b = m / R;
  return v.p + (int64_t)b * v.bs + (int64_t)(m - b * R) * v.ld;
}

struct Plan {
  int64_t M, Mp, strips1;                            // stage 1: strips of 64 m per role
  int64_t strips_up, splits_up, chunk_up;            // stage 2, chunk in m
  int64_t strips_dn, splits_dn, chunk_dn;
};

void split_of(int64_t L, int64_t gran, int64_t strips, int64_t* splits, int64_t* chunk) {
  const int64_t granules = (L + gran - 1) / gran;
  const int64_t want = (LS_TARGET_WGS + strips - 1) / strips;
  const int64_t cg = (granules + want - 1) / want;
  *splits = (granules + cg - 1) / cg;
  *chunk = cg * gran;
}

Plan plan_of(int64_t M, int64_t N, int64_t K) {
  Plan p;
  p.M = M;
  p.strips1 = (M + LS_ROWS - 1) / LS_ROWS;
  p.Mp = p.strips1 * LS_ROWS;
  p.strips_up = (N + LS_COLS - 1) / LS_COLS;
  p.strips_dn = (K + LS_COLS - 1) / LS_COLS;
  split_of(M, LS_M_GRAN, p.strips_up, &p.splits_up, &p.chunk_up);
  split_of(M, LS_M_GRAN, p.strips_dn, &p.splits_dn, &p.chunk_dn);
  return p;
}

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

// rows [r0, r0 + 64) x columns [c0, c0 + ncols) of a matrix of rows_total x cols_total -> lds[col - c0][row - r0] (transposed);
// zeros outside the matrix.  `rowp(row)` is the row's first element.  ncols % 8 == 0, c0 % 8 == 0.
template <class RowPtr>
FK_DEV void stage_transposed(bf16_t* lds, RowPtr rowp, int32_t r0, int32_t rows_total, int32_t c0, int32_t cols_total, int ncols,
                             int vec) {
  // 32 consecutive lanes take 32 consecutive rows of one 8-column chunk: their 2-byte LDS writes fall into 16 consecutive banks
  const int cpr = ncols / 8;
  for (int i = threadIdx.x; i < 64 * cpr; i += LS_THREADS) {
    const int blk = i >> 5;
    const int c = (blk % cpr) * 8, nn = (blk / cpr) * 32 + (i & 31);
    const int32_t row = r0 + nn, col = c0 + c;
    uint32_t e[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) e[q] = 0u;
    if (row < rows_total && col < cols_total) {
      const bf16_t* p = rowp(row) + col;
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
    for (int q = 0; q < 8; ++q) lds[(c + q) * LS_LDS_LD + nn] = (bf16_t)e[q];
  }
}

struct Stage1Args {
  View x, dy;
  const bf16_t* up; int64_t ld_up;
  const bf16_t* down; int64_t ld_down;
  int32_t M, R, N, K, rank;
  int32_t vec_up, vec_down;
  int64_t Mp;
  bf16_t *t_hi, *t_lo, *u_hi, *u_lo;                 // [r_pad][Mp]
  int32_t strips;                                    // blocks [0, strips) take role T, [strips, 2 strips) role U
};

// RT: tiles of 16 ranks = r_pad / 16 (2, 4, 6 or 8)
template <int RT>
__global__ __launch_bounds__(LS_THREADS) void lora_side_stage1_kernel(Stage1Args a) {
  __shared__ __attribute__((aligned(16))) bf16_t s_up[RT * 16 * LS_LDS_LD];        // [j][n]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const bool role_u = (int)blockIdx.x >= a.strips;
  const int strip = role_u ? blockIdx.x - a.strips : blockIdx.x;
  const int32_t m_row = strip * LS_ROWS + wave * 16;                     // the wave's first row (< Mp)
  const int32_t m = m_row + l15;                                         // A operand: the lane's row of X / dY
  const bool ok = m < a.M;
  const int rank = a.rank;
  f32x4_t acc[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) acc[t] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};

  if (!role_u) {
    // ---- role T: T[m, j] over k in [0, K)
    const int64_t K = a.K;
    const bf16_t* x_row = row_of(a.x, ok ? m : 0, a.R);
    if (m_row < a.M) {                                                   // wave-uniform: a wave with no row keeps its zeros
      for (int64_t k = 0; k < K; k += LS_T_STEP) {
        // A[row = m][kk] = X[m][k + kk]: lane (row = l15) holds kk = 8 lg + [0, 8)
        const bf16x8_t fa = load_frag(x_row, k + 8 * lg, K, ok, a.x.vec);
#pragma unroll
        for (int t = 0; t < RT; ++t) {
          // B[kk][col = j] = down[j][k + kk]: lane (col = l15) holds the same 8 kk of row j = 16 t + l15
          const int j = 16 * t + l15;
          const bf16x8_t fb = load_frag(a.down + (int64_t)(j < rank ? j : 0) * a.ld_down, k + 8 * lg, K, j < rank, a.vec_down);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc[t], 0, 0, 0);
        }
      }
    }
  } else {
    // ---- role U: U[m, j] over n in [0, N); every wave takes part in the staging
    const int32_t N = a.N;
    const bf16_t* dy_row = row_of(a.dy, ok ? m : 0, a.R);
    const bf16_t* up = a.up;
    const int64_t ld_up = a.ld_up;
    for (int32_t n0 = 0; n0 < N; n0 += LS_U_STEP) {
      __syncthreads();                                // the previous step's fragments have been read
      stage_transposed(s_up, [up, ld_up](int32_t n) { return up + (int64_t)n * ld_up; }, n0, N, 0, rank, RT * 16, a.vec_up);
      __syncthreads();
#pragma unroll
      for (int c = 0; c < LS_U_STEP; c += 32) {
        // A[row = m][nn] = dY[m][n0 + c + nn]: lane (row = l15) holds nn = 8 lg + [0, 8)
        const bf16x8_t fa = load_frag(dy_row, (int64_t)n0 + c + 8 * lg, N, ok, a.dy.vec);
#pragma unroll
        for (int t = 0; t < RT; ++t) {
          // B[nn][col = j] = up[n0 + c + nn][16 t + col]: lane (col = l15) holds the same 8 nn of LDS row j
          const bf16x8_t fb = *(const bf16x8_t*)(s_up + (t * 16 + l15) * LS_LDS_LD + c + 8 * lg);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc[t], 0, 0, 0);
        }
      }
    }
  }
  // D[row][col]: row = 4 lg + reg -> m, col = l15 -> j.  hi / lo pairs of the lane's four m, transposed: [j][m]
  bf16_t* hi = role_u ? a.u_hi : a.t_hi;
  bf16_t* lo = role_u ? a.u_lo : a.t_lo;
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int64_t at = (int64_t)(16 * t + l15) * a.Mp + m_row + 4 * lg;
    const uint32_t h01 = pack_bf2(acc[t][0], acc[t][1]), h23 = pack_bf2(acc[t][2], acc[t][3]);
    const uint32_t l01 = pack_bf2(acc[t][0] - bf_lo(h01), acc[t][1] - bf_hi(h01));
    const uint32_t l23 = pack_bf2(acc[t][2] - bf_lo(h23), acc[t][3] - bf_hi(h23));
    *(u32x2_t*)(hi + at) = u32x2_t{h01, h23};
    *(u32x2_t*)(lo + at) = u32x2_t{l01, l23};
  }
}

struct Role2 {
  View src;                                          // dY (role UP) / X (role DOWN)
  const bf16_t *hi, *lo;                             // T^T (role UP) / U^T (role DOWN): [r_pad][Mp]
  float* out;                                        // the output (splits == 1) or the partials [split][L * rank]
  int32_t L;                                         // columns of src: N / K
  int32_t splits, chunk;
};

struct Stage2Args {
  Role2 up, dn;
  int32_t M, R, rank;
  int64_t Mp;
  int32_t up_blocks;                                 // blocks [0, up_blocks) take role UP
  float scale;
  int32_t accumulate;                                // 1: an unsplit role adds its scaled sum to what its output holds
};

template <int RT>
__global__ __launch_bounds__(LS_THREADS) void lora_side_stage2_kernel(Stage2Args a) {
  __shared__ __attribute__((aligned(16))) bf16_t s_src[LS_COLS * LS_LDS_LD];       // [col][m]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const bool is_up = (int)blockIdx.x < a.up_blocks;
  const Role2 r = is_up ? a.up : a.dn;
  const int tile = is_up ? blockIdx.x : blockIdx.x - a.up_blocks;
  const int strip = tile / r.splits, sp = tile - strip * r.splits;
  const int32_t c0 = strip * LS_COLS;
  const int32_t M = a.M, R = a.R, rank = a.rank;
  const int32_t m_b = sp * r.chunk;
  const int32_t m_e = M - m_b > r.chunk ? m_b + r.chunk : M;
  const View src = r.src;
  f32x4_t acc[RT][2];
#pragma unroll
  for (int t = 0; t < RT; ++t) acc[t][0] = acc[t][1] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
  for (int32_t m0 = m_b; m0 < m_e; m0 += LS_M_STEP) {
    __syncthreads();                                  // the previous step's fragments have been read
    stage_transposed(s_src, [src, R](int32_t m) { return row_of(src, m, R); }, m0, M, c0, r.L, LS_COLS, src.vec);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < LS_M_STEP; c += 32) {
      // B[mm][col] = src[m0 + c + mm][c0 + 32 wave + 16 h + col]: lane (col = l15) holds mm = 8 lg + [0, 8)
      bf16x8_t fb[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) fb[h] = *(const bf16x8_t*)(s_src + (wave * 32 + h * 16 + l15) * LS_LDS_LD + c + 8 * lg);
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        // A[row = j][mm] = T^T[16 t + row][m0 + c + mm] (U^T in role DOWN): lane (row = l15) holds the same 8 mm, hi and lo
        const int64_t at = (int64_t)(t * 16 + l15) * a.Mp + m0 + c + 8 * lg;
        const bf16x8_t fh = *(const bf16x8_t*)(r.hi + at);
        const bf16x8_t fl = *(const bf16x8_t*)(r.lo + at);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          acc[t][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fh, fb[h], acc[t][h], 0, 0, 0);
          acc[t][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fl, fb[h], acc[t][h], 0, 0, 0);
        }
      }
    }
  }
  // D[row][col]: row = 4 lg + reg -> j, col = l15 -> the output column (n in role UP: d_up[n][j]; k in role DOWN: d_down[j][k])
  const bool final_ = r.splits == 1;
  float* out = r.out + (final_ ? 0 : (int64_t)sp * r.L * rank);
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int32_t col = c0 + wave * 32 + h * 16 + l15;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = 16 * t + 4 * lg + e;
        if (j < rank && col < r.L) {
          const int64_t at = is_up ? (int64_t)col * rank + j : (int64_t)j * r.L + col;
          float v = final_ ? a.scale * acc[t][h][e] : acc[t][h][e];
          if (final_ && a.accumulate) v += out[at];
          out[at] = v;
        }
      }
    }
}

// out[i] = scale * (p[0][i] + p[1][i] + ...) (+ out[i] when accumulate), splits ascending; elements [0, n_up) are d_up's, the
// next n_dn are d_down's
__global__ __launch_bounds__(LS_THREADS) void lora_side_reduce_kernel(const float* p_up, int splits_up, int64_t n_up, float* d_up,
                                                                      const float* p_dn, int splits_dn, int64_t n_dn, float* d_down,
                                                                      float scale, int accumulate) {
  int64_t i = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x;
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
Span span_of(const void* p, int64_t bs, int64_t B, int64_t ld, int64_t rows, int64_t cols, size_t elem) {
  const uintptr_t lo = (uintptr_t)p;
  return Span{lo, lo + (uintptr_t)((B - 1) * bs + (rows - 1) * ld + cols) * elem};
}
bool overlap(const Span& x, const Span& y) { return x.lo < y.hi && y.lo < x.hi; }

int64_t rank_pad(int64_t rank) { return (rank + 31) / 32 * 32; }
int64_t part_up_of(const Plan& p, int64_t N, int64_t rank) { return p.splits_up > 1 ? p.splits_up * N * rank : 0; }
int64_t part_dn_of(const Plan& p, int64_t K, int64_t rank) { return p.splits_dn > 1 ? p.splits_dn * rank * K : 0; }
// partials + 3 floats of slack to reach a 16-byte boundary + 4 bf16 matrices [r_pad][Mp]
int64_t ws_floats_of(const Plan& p, int64_t N, int64_t K, int64_t rank) {
  return part_up_of(p, N, rank) + part_dn_of(p, K, rank) + 3 + 2 * rank_pad(rank) * p.Mp;
}

constexpr int64_t LS_MAX_DIM = 0x7fffffffLL - 1024;    // M, N, K as int32 with room for a padded step

bool dims_ok(int64_t B, int64_t R, int64_t N, int64_t K) {
  return B >= 1 && R >= 1 && N >= 1 && K >= 1 && B <= LS_MAX_DIM && R <= LS_MAX_DIM && B * R <= LS_MAX_DIM && N <= LS_MAX_DIM &&
         K <= LS_MAX_DIM;
}

}  // namespace

extern "C" int64_t fk_lora_side_grad_ws_floats(int64_t B, int64_t R, int64_t N, int64_t K, int64_t rank) {
  if (!dims_ok(B, R, N, K) || rank < 1 || rank > FK_LORA_MAX_RANK) return 0;
  return ws_floats_of(plan_of(B * R, N, K), N, K, rank);
}

extern "C" int fk_lora_side_grad_bf16(const void* x, int64_t ld_x, int64_t bs_x, const void* dy, int64_t ld_dy, int64_t bs_dy, int64_t B,
                                      int64_t R, int64_t N, int64_t K, const void* up, int64_t ld_up, const void* down, int64_t ld_down,
                                      int64_t rank, float scale, float* d_up, float* d_down, int accumulate, float* ws,
                                      int64_t ws_floats, fk_stream_t stream) {
  const char* fn = "fk_lora_side_grad_bf16";
  FK_CHECK_ARG(x && dy && up && down && d_up && d_down && ws, "%s: NULL pointer", fn);
  FK_CHECK_ARG(B >= 1 && R >= 1 && N >= 1 && K >= 1, "%s: needs B, R, N, K >= 1 (B = %lld, R = %lld, N = %lld, K = %lld)", fn,
               (long long)B, (long long)R, (long long)N, (long long)K);
  if (!dims_ok(B, R, N, K)) {
    fk_set_error("%s: B * R = %lld x %lld rows, N = %lld or K = %lld exceed 32-bit indices", fn, (long long)B, (long long)R,
                 (long long)N, (long long)K);
    return FK_EUNSUPPORTED;
  }
  if (rank < 1 || rank > FK_LORA_MAX_RANK) {
    fk_set_error("%s: rank %lld, supported 1 to %d", fn, (long long)rank, FK_LORA_MAX_RANK);
    return FK_EUNSUPPORTED;
  }
  FK_CHECK_ARG(ld_x >= K && ld_dy >= N && ld_up >= rank && ld_down >= K, "%s: a row stride below the row length (ld_x = %lld, "
               "ld_down = %lld, K = %lld, ld_dy = %lld, N = %lld, ld_up = %lld, rank = %lld)", fn, (long long)ld_x, (long long)ld_down,
               (long long)K, (long long)ld_dy, (long long)N, (long long)ld_up, (long long)rank);
  FK_CHECK_ARG(bs_x >= 0 && bs_dy >= 0, "%s: a negative batch stride (bs_x = %lld, bs_dy = %lld)", fn, (long long)bs_x, (long long)bs_dy);
  FK_CHECK_ARG(scale == scale && scale - scale == 0.0f, "%s: the scale is not finite", fn);
  FK_CHECK_ARG(accumulate == 0 || accumulate == 1, "%s: accumulate is %d, it must be 0 (overwrite) or 1 (add)", fn, accumulate);
  FK_CHECK_ARG((uintptr_t)ws % 4 == 0 && (uintptr_t)d_up % 4 == 0 && (uintptr_t)d_down % 4 == 0, "%s: an fp32 pointer is not 4-byte "
               "aligned", fn);
  const int64_t M = B * R;
  const Plan p = plan_of(M, N, K);
  const int64_t need = ws_floats_of(p, N, K, rank);
  FK_CHECK_ARG(ws_floats >= need, "%s: the workspace holds %lld floats, [%lld x %lld, %lld, %lld] at rank %lld needs %lld "
               "(fk_lora_side_grad_ws_floats)", fn, (long long)ws_floats, (long long)B, (long long)R, (long long)N, (long long)K,
               (long long)rank, (long long)need);
  const Span in[4] = {span_of(x, bs_x, B, ld_x, R, K, 2), span_of(dy, bs_dy, B, ld_dy, R, N, 2), span_of(up, 0, 1, ld_up, N, rank, 2),
                      span_of(down, 0, 1, ld_down, rank, K, 2)};
  const Span o_up = span_of(d_up, 0, 1, rank, N, rank, 4), o_dn = span_of(d_down, 0, 1, K, rank, K, 4);
  const Span o_ws = span_of(ws, 0, 1, need, 1, need, 4);
  FK_CHECK_ARG(!overlap(o_up, o_dn), "%s: d_up overlaps d_down", fn);
  for (int i = 0; i < 4; ++i)
    FK_CHECK_ARG(!overlap(o_up, in[i]) && !overlap(o_dn, in[i]) && !overlap(o_ws, in[i]), "%s: an output or the workspace overlaps an "
                 "input", fn);
  FK_CHECK_ARG(!overlap(o_ws, o_up) && !overlap(o_ws, o_dn), "%s: the workspace overlaps an output", fn);
  const int64_t up_blocks = p.strips_up * p.splits_up, dn_blocks = p.strips_dn * p.splits_dn;
  if (up_blocks + dn_blocks > 0x7fffffffLL || 2 * p.strips1 > 0x7fffffffLL) {
    fk_set_error("%s: %lld + %lld workgroups exceed one grid", fn, (long long)up_blocks, (long long)dn_blocks);
    return FK_EUNSUPPORTED;
  }
  const int64_t rp = rank_pad(rank);
  float* part_up = ws;
  float* part_dn = ws + part_up_of(p, N, rank);
  bf16_t* pairs = (bf16_t*)(((uintptr_t)(part_dn + part_dn_of(p, K, rank)) + 15) & ~(uintptr_t)15);
  Stage1Args s1;
  s1.x = View{(const bf16_t*)x, ld_x, bs_x, (uintptr_t)x % 16 == 0 && ld_x % 8 == 0 && (B == 1 || bs_x % 8 == 0)};
  s1.dy = View{(const bf16_t*)dy, ld_dy, bs_dy, (uintptr_t)dy % 16 == 0 && ld_dy % 8 == 0 && (B == 1 || bs_dy % 8 == 0)};
  s1.up = (const bf16_t*)up, s1.ld_up = ld_up, s1.down = (const bf16_t*)down, s1.ld_down = ld_down;
  s1.M = (int32_t)M, s1.R = (int32_t)R, s1.N = (int32_t)N, s1.K = (int32_t)K, s1.rank = (int32_t)rank;
  s1.vec_up = (uintptr_t)up % 16 == 0 && ld_up % 8 == 0;
  s1.vec_down = (uintptr_t)down % 16 == 0 && ld_down % 8 == 0;
  s1.Mp = p.Mp;
  s1.t_hi = pairs, s1.t_lo = pairs + rp * p.Mp, s1.u_hi = pairs + 2 * rp * p.Mp, s1.u_lo = pairs + 3 * rp * p.Mp;
  s1.strips = (int32_t)p.strips1;
  Stage2Args s2;
  s2.up = Role2{s1.dy, s1.t_hi, s1.t_lo, p.splits_up > 1 ? part_up : d_up, (int32_t)N, (int32_t)p.splits_up, (int32_t)p.chunk_up};
  s2.dn = Role2{s1.x, s1.u_hi, s1.u_lo, p.splits_dn > 1 ? part_dn : d_down, (int32_t)K, (int32_t)p.splits_dn, (int32_t)p.chunk_dn};
  s2.M = (int32_t)M, s2.R = (int32_t)R, s2.rank = (int32_t)rank, s2.Mp = p.Mp;
  s2.up_blocks = (int32_t)up_blocks, s2.scale = scale, s2.accumulate = accumulate;
  const dim3 grid1((unsigned)(2 * p.strips1)), grid2((unsigned)(up_blocks + dn_blocks)), block(LS_THREADS);
  switch (rp / 32) {
    case 1: hipLaunchKernelGGL(lora_side_stage1_kernel<2>, grid1, block, 0, (hipStream_t)stream, s1); break;
    case 2: hipLaunchKernelGGL(lora_side_stage1_kernel<4>, grid1, block, 0, (hipStream_t)stream, s1); break;
    case 3: hipLaunchKernelGGL(lora_side_stage1_kernel<6>, grid1, block, 0, (hipStream_t)stream, s1); break;
    default: hipLaunchKernelGGL(lora_side_stage1_kernel<8>, grid1, block, 0, (hipStream_t)stream, s1); break;
  }
  FK_CHECK_LAUNCH(fn);
  switch (rp / 32) {
    case 1: hipLaunchKernelGGL(lora_side_stage2_kernel<2>, grid2, block, 0, (hipStream_t)stream, s2); break;
    case 2: hipLaunchKernelGGL(lora_side_stage2_kernel<4>, grid2, block, 0, (hipStream_t)stream, s2); break;
    case 3: hipLaunchKernelGGL(lora_side_stage2_kernel<6>, grid2, block, 0, (hipStream_t)stream, s2); break;
    default: hipLaunchKernelGGL(lora_side_stage2_kernel<8>, grid2, block, 0, (hipStream_t)stream, s2); break;
  }
  FK_CHECK_LAUNCH(fn);
  const int64_t n_up = p.splits_up > 1 ? N * rank : 0, n_dn = p.splits_dn > 1 ? rank * K : 0;
  if (n_up + n_dn > 0) {
    const int64_t blocks = (n_up + n_dn + LS_THREADS - 1) / LS_THREADS;
    hipLaunchKernelGGL(lora_side_reduce_kernel, dim3((unsigned)blocks), block, 0, (hipStream_t)stream, part_up, (int)p.splits_up, n_up,
                       d_up, part_dn, (int)p.splits_dn, n_dn, d_down, scale, accumulate);
    FK_CHECK_LAUNCH(fn);
  }
  return FK_OK;
}
