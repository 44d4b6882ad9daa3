// LoRA merge (transformer.py: load_lora_adapter / set_adapters / set_lora_scale): the adapters become part of a bf16 weight.
//   out[n, k] = bf16_rne( float(base[n, k]) + sum_t scale_t * acc_t[n, k] ),   acc_t[n, k] = sum_j up_t[n, j] * down_t[j, k]
// over base / out [N, K], up_t [N, rank_t] (lora_B), down_t [rank_t, K] (lora_A), all bf16 with contiguous rows and a row
// stride of their own.  HBM-bound by construction: 2 B read + 2 B written per weight element, the adapters are small.
//
// One workgroup (4 waves) per 64 x 128 (n x k) tile of the weight, wave w on rows [16w, 16w + 16) and all 128 columns.  Per term:
//   stage   up's 64 rows as they are, [n][j], and down's 128 columns TRANSPOSED, [k][j], into LDS, j zero-padded to
//           r_pad = 32 * ceil(rank / 32); rows / columns beyond N / K are zeros.  Both images have the reduction index
//           contiguous, which is what an MFMA operand fragment wants (8 consecutive j per lane = one 16-byte LDS read).
//   product the tile as down^T . up^T on v_mfma_f32_16x16x32_bf16: the operand rows are 16 of the tile's k, the columns the
//           wave's 16 n, so a lane's four accumulators are four consecutive k of ONE weight row.  A wave issues eight such
//           products per 32 ranks (k sub-tiles s = 0..7); sub-tile s holds k = 32 (s / 2) + 8 (row / 4) + 4 (s % 2) + row % 4,
//           so sub-tiles 2p and 2p + 1 together give a lane 8 consecutive k: one 16-byte load of base, one 16-byte store.
//   add     v = fmaf(scale_t, acc_t, v) in fp32, terms in ascending t, starting from v = float(base).
// The accumulation order INSIDE acc_t is the MFMA's (fp32, r_pad products); tests/lora_ref.py bounds it, not emulates it.
// Every element is read (base) and written (out) by the same lane, so out may be base itself.  Terms whose scale is 0 are
// dropped on the host: with none left the kernel copies base's bits (and an in-place call launches nothing).
// Views that are not 16-byte aligned (pointer or row stride) take the same kernel with element-wise global accesses.
#include "fk_common.h"

namespace {

constexpr int LM_THREADS = 256;
constexpr int LM_TILE_N = 64;                        // rows (n) of a workgroup's tile: 16 per wave
constexpr int LM_TILE_K = 128;                       // columns (k): 8 MFMA sub-tiles of 16
constexpr int LM_LDS_LD = FK_LORA_MAX_RANK + 8;      // elements per LDS row: 272 B, rows 16-byte aligned, 4 banks apart

struct LoraArgs {
  fk_lora_term t[FK_LORA_MAX_TERMS];                 // by value: the device never follows a pointer into host memory
  int32_t n_terms;
};

// column (0 .. 127) of the tile that row `row` (0 .. 15) of MFMA sub-tile s (0 .. 7) stands for
FK_DEV int tile_k_of(int s, int row) { return 32 * (s >> 1) + 8 * (row >> 2) + 4 * (s & 1) + (row & 3); }

// rows [r0, r0 + LM_TILE_N) x columns [0, r_pad) of a [rows_total, cols] matrix -> lds[row][col]; zeros outside the matrix
FK_DEV void stage_rows(bf16_t* lds, const bf16_t* src, int64_t ld, int64_t r0, int64_t rows_total, int cols, int r_pad) {
  const bool al = (uintptr_t)src % 16 == 0 && ld % 8 == 0;
  const int cpr = r_pad / 8;
  for (int i = threadIdx.x; i < LM_TILE_N * cpr; i += LM_THREADS) {
    const int r = i / cpr, c = (i - r * cpr) * 8;
    const int64_t row = r0 + r;
    u32x4_t w = {0u, 0u, 0u, 0u};
    if (row < rows_total) {
      const bf16_t* p = src + row * ld + c;
      if (al && c + 8 <= cols) {
        w = *(const u32x4_t*)p;
      } else {
        uint32_t e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = c + j < cols ? (uint32_t)p[j] : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = e[2 * j] | (e[2 * j + 1] << 16);
      }
    }
    *(u32x4_t*)(lds + r * LM_LDS_LD + c) = w;
  }
}

// rows [0, r_pad) x columns [c0, c0 + LM_TILE_K) of a [rows_total, cols_total] matrix -> lds[col][row] (transposed); zeros outside
FK_DEV void stage_cols_transposed(bf16_t* lds, const bf16_t* src, int64_t ld, int64_t c0, int64_t cols_total, int rows_total,
                                  int r_pad) {
  const bool al = (uintptr_t)src % 16 == 0 && ld % 8 == 0;
  // 32 consecutive lanes take 32 consecutive j of one 8-column chunk: their 2-byte LDS writes fall into 16 consecutive banks
  static_assert(LM_TILE_K / 8 == 16, "the item map below: 32 j x 16 chunks per 512 items");
  for (int i = threadIdx.x; i < r_pad * (LM_TILE_K / 8); i += LM_THREADS) {
    const int j = (i >> 9) * 32 + (i & 31), c = ((i >> 5) & 15) * 8;
    const int64_t col = c0 + c;
    uint32_t e[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) e[q] = 0u;
    if (j < rows_total) {
      const bf16_t* p = src + (int64_t)j * ld + col;
      if (al && col + 8 <= cols_total) {
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
    for (int q = 0; q < 8; ++q) lds[(c + q) * LM_LDS_LD + j] = (bf16_t)e[q];
  }
}

__global__ __launch_bounds__(LM_THREADS) void lora_merge_kernel(const bf16_t* base, int64_t ld_base, bf16_t* out,
                                                                int64_t ld_out, int N, int K, int tiles_k, int vec16,
                                                                LoraArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t s_up[LM_TILE_N * LM_LDS_LD];
  __shared__ __attribute__((aligned(16))) bf16_t s_dn[LM_TILE_K * LM_LDS_LD];
  const int tile = blockIdx.x;
  const int tn = tile / tiles_k, tk = tile - tn * tiles_k;
  const int64_t n0 = (int64_t)tn * LM_TILE_N, k0 = (int64_t)tk * LM_TILE_K;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int64_t n = n0 + wave * 16 + l15;             // the weight row of this lane's 32 elements
  const bool row_ok = n < N;

  // v[p][0..7]: elements k0 + 32 p + 8 lg + [0, 8) of row n
  float v[4][8];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int64_t k = k0 + 32 * p + 8 * lg;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[p][e] = 0.0f;
    if (row_ok && k < K) {                            // K % 8 == 0: a chunk of 8 lies inside the row or outside it
      const bf16_t* bp = base + n * ld_base + k;
      if (vec16) {
        const u32x4_t w = *(const u32x4_t*)bp;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[p][2 * e] = bf_lo(w[e]);
          v[p][2 * e + 1] = bf_hi(w[e]);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[p][e] = bf2f(bp[e]);
      }
    }
  }

  for (int t = 0; t < a.n_terms; ++t) {
    const fk_lora_term tm = a.t[t];
    const int r_pad = (tm.rank + 31) & ~31;
    __syncthreads();                                  // the previous term's fragments have been read
    stage_rows(s_up, (const bf16_t*)tm.up, tm.ld_up, n0, N, tm.rank, r_pad);
    stage_cols_transposed(s_dn, (const bf16_t*)tm.down, tm.ld_down, k0, K, tm.rank, r_pad);
    __syncthreads();
    f32x4_t acc[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) acc[s] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = 0; c < r_pad; c += 32) {
      // B operand: up^T, B[j][col] = up[n0 + 16 wave + col][j]; lane (col = l15) holds j = c + 8 lg + [0, 8)
      const bf16x8_t fb = *(const bf16x8_t*)(s_up + (wave * 16 + l15) * LM_LDS_LD + c + 8 * lg);
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        // A operand: down^T, A[row][j] = down[j][k0 + tile_k_of(s, row)]; lane (row = l15) holds the same 8 j
        const bf16x8_t fa = *(const bf16x8_t*)(s_dn + tile_k_of(s, l15) * LM_LDS_LD + c + 8 * lg);
        acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc[s], 0, 0, 0);
      }
    }
    // D[row][col]: col = l15 (the lane's n), row = 4 lg + reg -> k = 32 (s / 2) + 8 lg + 4 (s % 2) + reg = v[s / 2][4 (s % 2) + reg]
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[s >> 1][4 * (s & 1) + e] = fmaf(tm.scale, acc[s][e], v[s >> 1][4 * (s & 1) + e]);
  }

#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int64_t k = k0 + 32 * p + 8 * lg;
    if (row_ok && k < K) {
      bf16_t* op = out + n * ld_out + k;
      if (vec16) {
        u32x4_t w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = pack_bf2(v[p][2 * e], v[p][2 * e + 1]);
        *(u32x4_t*)op = w;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) op[e] = f2bf(v[p][e]);
      }
    }
  }
}

struct Span { uintptr_t lo, hi; };                     // [lo, hi): first element to the end of the last row
Span span_of(const void* p, int64_t ld, int64_t rows, int64_t cols) {
  const uintptr_t lo = (uintptr_t)p;
  return Span{lo, lo + (uintptr_t)((rows - 1) * ld + cols) * sizeof(bf16_t)};
}
bool overlap(const Span& x, const Span& y) { return x.lo < y.hi && y.lo < x.hi; }

}  // namespace

extern "C" int fk_lora_merge_bf16(const void* base, int64_t ld_base, void* out, int64_t ld_out, int32_t N, int32_t K,
                                  const fk_lora_term* terms, int32_t n_terms, fk_stream_t stream) {
  FK_CHECK_ARG(base && out && terms, "fk_lora_merge_bf16: NULL pointer");
  FK_CHECK_ARG(N >= 1 && K >= 8 && K % 8 == 0, "fk_lora_merge_bf16: needs N >= 1 and K >= 8, K %% 8 == 0 (N = %d, K = %d)", N, K);
  FK_CHECK_ARG(ld_base >= K && ld_out >= K, "fk_lora_merge_bf16: a row stride below K = %d (ld_base = %lld, ld_out = %lld)", K,
               (long long)ld_base, (long long)ld_out);
  if (n_terms < 1 || n_terms > FK_LORA_MAX_TERMS) {
    fk_set_error("fk_lora_merge_bf16: 1 to %d terms per launch, got %d", FK_LORA_MAX_TERMS, n_terms);
    return FK_EUNSUPPORTED;
  }
  const Span so = span_of(out, ld_out, N, K), sb = span_of(base, ld_base, N, K);
  const bool in_place = base == out && ld_base == ld_out;
  FK_CHECK_ARG(in_place || !overlap(so, sb), "fk_lora_merge_bf16: out overlaps base (it may only BE base, same row stride)");
  LoraArgs a;
  a.n_terms = 0;
  for (int t = 0; t < n_terms; ++t) {
    const fk_lora_term& tm = terms[t];
    FK_CHECK_ARG(tm.up && tm.down, "fk_lora_merge_bf16: term %d: NULL pointer", t);
    if (tm.rank < 1 || tm.rank > FK_LORA_MAX_RANK) {
      fk_set_error("fk_lora_merge_bf16: term %d: rank %d, supported 1 to %d", t, tm.rank, FK_LORA_MAX_RANK);
      return FK_EUNSUPPORTED;
    }
    FK_CHECK_ARG(tm.ld_up >= tm.rank && tm.ld_down >= K, "fk_lora_merge_bf16: term %d: a row stride below the row length "
                 "(ld_up = %lld, rank = %d, ld_down = %lld, K = %d)", t, (long long)tm.ld_up, tm.rank, (long long)tm.ld_down, K);
    FK_CHECK_ARG(tm.scale == tm.scale && tm.scale - tm.scale == 0.0f, "fk_lora_merge_bf16: term %d: the scale is not finite", t);
    FK_CHECK_ARG(!overlap(so, span_of(tm.up, tm.ld_up, N, tm.rank)) && !overlap(so, span_of(tm.down, tm.ld_down, tm.rank, K)),
                 "fk_lora_merge_bf16: term %d: out overlaps the adapter", t);
    if (tm.scale != 0.0f) a.t[a.n_terms++] = tm;     // a zero term adds nothing (and must not turn a -0 of base into +0)
  }
  if (a.n_terms == 0 && in_place) return FK_OK;      // base's bits are already there
  const int64_t tiles_n = ((int64_t)N + LM_TILE_N - 1) / LM_TILE_N, tiles_k = ((int64_t)K + LM_TILE_K - 1) / LM_TILE_K;
  if (tiles_n * tiles_k > 0x7fffffffLL) {
    fk_set_error("fk_lora_merge_bf16: %lld x %lld tiles exceed one grid", (long long)tiles_n, (long long)tiles_k);
    return FK_EUNSUPPORTED;
  }
  const int vec16 = (uintptr_t)base % 16 == 0 && (uintptr_t)out % 16 == 0 && ld_base % 8 == 0 && ld_out % 8 == 0;
  hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)(tiles_n * tiles_k)), dim3(LM_THREADS), 0, (hipStream_t)stream,
                     (const bf16_t*)base, ld_base, (bf16_t*)out, ld_out, (int)N, (int)K, (int)tiles_k, vec16, a);
  FK_CHECK_LAUNCH("fk_lora_merge_bf16");
  return FK_OK;
}
