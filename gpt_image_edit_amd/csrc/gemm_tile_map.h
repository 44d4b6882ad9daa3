// Tile order of the large-tile GEMMs as launch constants: what a workgroup needs to find its (problem, m0, n0) without a
// division and without reading anything but the first cache lines of its kernel arguments.  No HIP dependency: the host
// fills the records (fk_gemm2_launch), the kernels read them, and a plain C++ program can compile this file on the CPU
// (tests/test_gemm_tile_map.py).  A translation unit may define FK_TM_FN (function qualifiers) before including it.
//
// Order (unchanged since round 1): workgroup b runs on XCD b % 8, so the grid is cut into 8 chunks of consecutive tile
// indices; a tile index walks the problems one after the other, and inside a problem groups of `group_m` row tiles,
// row tile fastest inside a group, so that consecutive tiles share W columns and a group's A rows stay in one XCD's L2.
#pragma once
#include <stdint.h>

#ifndef FK_TM_FN
#define FK_TM_FN inline
#endif
#if defined(__clang__)
#define TM_UNROLL _Pragma("unroll")
#else
#define TM_UNROLL
#endif

constexpr int TM_MAX_GROUP = 4;   // == FK_MAX_GROUP (include/fk.h)
constexpr int TM_BM = 256;        // rows of every large tile

// ---- division by a launch constant -------------------------------------------------------------------------------------
// floor(t / d) = floor(2 t m / 2^32) with m = ceil(2^31 / d): m d = 2^31 + e, 0 <= e < d, so 2 t m / 2^32 = t / d + t e / (d 2^31),
// and the second term stays below the 1 / d that separates t / d's fraction from the next integer whenever t e < 2^31.
// Exact for t d <= 2^31 (tm_div_domain), in particular for every d <= 4096 and t < 65536; d = 1 gives m = 2^31 and the
// identity.  On the device: one shift and one s_mul_hi_u32.
FK_TM_FN uint32_t tm_magic(uint32_t d) { return (uint32_t)(((1ull << 31) + d - 1) / d); }
FK_TM_FN uint32_t tm_div(uint32_t t, uint32_t magic) { return (uint32_t)(((uint64_t)(t << 1) * magic) >> 32); }
FK_TM_FN bool tm_div_domain(uint64_t t_max, uint64_t d) { return d >= 1 && t_max < (1ull << 31) && t_max * d <= (1ull << 31); }

// ---- one class of tiles: TM_BM x bn tiles over the column tiles [col0 / bn, col0 / bn + nbn) of every problem ------------
struct TmClass {
  int32_t before[TM_MAX_GROUP + 1];   // prefix sums of the problems' tile counts
  int32_t per_group, col0;            // group_m * (column tiles of the class); first column of the class
  uint32_t per_group_mul, group_m_mul;
  int32_t nbm[TM_MAX_GROUP];          // row tiles of problem i
  uint32_t last_mul[TM_MAX_GROUP];    // tm_magic of the depth of problem i's last (partial) group
};

// ---- the entry record: the front of the kernel arguments ------------------------------------------------------------------
struct TileEntry {
  uint32_t grid, xq, xr;   // workgroups of the launch, grid >> 3, grid & 7 (the XCD chunks)
  int32_t n, group_m, nk;  // problems; depth of a group in row tiles (clamped to the deepest problem); K / 64
  TmClass cls[2];          // [0] the launch's tiles (mixed grid: the 256 x 256 ones), [1] the mixed grid's 256 x 128 ones
  // mixed grid, per XCD (workgroup index % 8): the chunk of each class it works off, one 16-byte row per XCD (one fetch)
  struct Xcd { int32_t big_start, big_cnt, small_start, pad_; } xcd[8];
};

// ---- what the seven prologue requests of a tile need from its problem -------------------------------------------------------
enum { TM_A_FLAT = 1, TM_C_FLAT = 2, TM_R_FLAT = 4, TM_G_FLAT = 8 };
struct ProbEntry {
  const void* A;
  const void* W;
  int32_t lda, ldw;   // elements; the launcher guarantees 256 rows of either fit 31 bits of byte offset
  int32_t M, N, K;
  int32_t flags;      // TM_*_FLAT: row m of A / C / the residual lies at m * ld; the gate row of every m is row 0
};

// rows addressed as base + (m / rows_per_batch) * batch_stride + (m % rows_per_batch) * ld (include/fk.h: fk_rows) lie at
// m * ld for every m < M when there is one batch, when the problem ends inside the first batch, or when the batches follow
// each other without a gap
FK_TM_FN bool tm_rows_flat(int64_t ld, int64_t rows_per_batch, int64_t batch_stride, int64_t M) {
  return rows_per_batch <= 0 || M <= rows_per_batch || batch_stride == rows_per_batch * ld;
}

// ---- device and host: which tile ----------------------------------------------------------------------------------------
// position of workgroup `bid` in the launch's tile list
FK_TM_FN int tm_xcd_chunk(uint32_t xq, uint32_t xr, uint32_t bid) {
  const uint32_t xcd = bid & 7, idx = bid >> 3;
  return (int)((xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + idx);
}
FK_TM_FN int tm_xcd_chunk(const TileEntry& e, uint32_t bid) { return tm_xcd_chunk(e.xq, e.xr, bid); }

// what tm_tile_hot reads of the entry record and one of its classes, as plain values: a kernel fetches exactly these in one
// go before it computes anything (gemm_pingpong_bf16.hip: load_hot)
struct TmHot {
  int32_t n, group_m;
  int32_t before[TM_MAX_GROUP - 1];   // of problems 1 ..: problem 0 starts at tile 0
  int32_t nbm[TM_MAX_GROUP];
  uint32_t last_mul[TM_MAX_GROUP];
  int32_t per_group, col0;
  uint32_t per_group_mul, group_m_mul;
};
FK_TM_FN TmHot tm_hot(const TileEntry& e, const TmClass& c) {
  TmHot h;
  h.n = e.n;
  h.group_m = e.group_m;
  TM_UNROLL
  for (int i = 0; i < TM_MAX_GROUP; ++i) {
    if (i > 0) h.before[i - 1] = c.before[i];
    h.nbm[i] = c.nbm[i];
    h.last_mul[i] = c.last_mul[i];
  }
  h.per_group = c.per_group;
  h.col0 = c.col0;
  h.per_group_mul = c.per_group_mul;
  h.group_m_mul = c.group_m_mul;
  return h;
}

// tile t of a class: problem pi, first row m0, first column n0 (bn: the class's tile width)
FK_TM_FN void tm_tile_hot(const TmHot& h, int bn, int t, int& pi, int& m0, int& n0) {
  pi = 0;
  int base = 0, nbm = h.nbm[0];
  uint32_t lmul = h.last_mul[0];
  TM_UNROLL
  for (int i = 1; i < TM_MAX_GROUP; ++i) {
    const bool here = i < h.n && t >= h.before[i - 1];
    pi = here ? i : pi;
    base = here ? h.before[i - 1] : base;
    nbm = here ? h.nbm[i] : nbm;
    lmul = here ? h.last_mul[i] : lmul;
  }
  const uint32_t u = (uint32_t)(t - base);
  const uint32_t g = tm_div(u, h.per_group_mul);
  const int first_m = (int)g * h.group_m;
  const bool full = nbm - first_m >= h.group_m;          // every group but a problem's last is group_m deep
  const int gm = full ? h.group_m : nbm - first_m;
  const uint32_t rem = u - g * (uint32_t)h.per_group;
  const uint32_t col = tm_div(rem, full ? h.group_m_mul : lmul);
  m0 = (first_m + (int)(rem - col * (uint32_t)gm)) * TM_BM;
  n0 = h.col0 + (int)col * bn;
}
FK_TM_FN void tm_tile(const TileEntry& e, const TmClass& c, int bn, int t, int& pi, int& m0, int& n0) {
  tm_tile_hot(tm_hot(e, c), bn, t, pi, m0, n0);
}

// ---- tile walk: G workgroups (one per CU) instead of one workgroup per tile -----------------------------------------------------
// The launch keeps its `grid` PLACES (e.grid / xq / xr: a place is what the workgroup index is to the one-workgroup-per-tile launch) and workgroup
// g takes the places g, g + G, g + 2 G, ... in turn.  The dispatcher hands place b to the CU that becomes free first, which on
// a grid of equal tiles is the CU that ran place b - G: a CU sees the same tiles in the same order either way (and, G being a
// multiple of 8 on the device, the same XCD chunk).
FK_TM_FN int tm_walk_count(uint32_t places, uint32_t G, uint32_t g) { return g < places ? (int)((places - 1 - g) / G) + 1 : 0; }
FK_TM_FN uint32_t tm_walk_place(uint32_t G, uint32_t g, uint32_t i) { return g + i * G; }
// mixed grid: place b of the launch is tile `t` of class 0 (256 x 256; returns false) or of class 1 (256 x 128; true) -- every
// XCD's chunk of the big tiles first, then its chunk of the small ones
FK_TM_FN bool tm_mix_place(int32_t big_start, int32_t big_cnt, int32_t small_start, uint32_t b, int& t) {
  const int idx = (int)(b >> 3);
  const bool small = idx >= big_cnt;
  t = small ? small_start + idx - big_cnt : big_start + idx;
  return small;
}
FK_TM_FN bool tm_mix_place(const TileEntry& e, uint32_t b, int& t) {
  return tm_mix_place(e.xcd[b & 7].big_start, e.xcd[b & 7].big_cnt, e.xcd[b & 7].small_start, b, t);
}
// the per-XCD table of a mixed grid of tb big and ts small tiles; false: an XCD would get fewer places than big tiles
FK_TM_FN bool tm_fill_mix(TileEntry& e, int tb, int ts) {
  const int W = tb + ts;
  int bs = 0, ss = 0;
  for (int x = 0; x < 8; ++x) {
    const int wx = W / 8 + (x < W % 8 ? 1 : 0), bx = tb / 8 + (x < tb % 8 ? 1 : 0);
    if (wx < bx) return false;
    e.xcd[x] = {bs, bx, ss, 0};
    bs += bx;
    ss += wx - bx;
  }
  return true;
}

// ---- host: fill the records -----------------------------------------------------------------------------------------------
// group_m of the launch: a depth beyond the deepest problem changes nothing (one group per problem either way), so it is
// clamped there, which keeps every divisor of the order within the row-tile counts
FK_TM_FN int tm_group_m(const int32_t* M, int n, int group_m) {
  int deepest = 1;
  for (int i = 0; i < n; ++i) {
    const int nbm = (M[i] + TM_BM - 1) / TM_BM;
    if (nbm > deepest) deepest = nbm;
  }
  return group_m < deepest ? group_m : deepest;
}

// returns the class's tile count, or -1 when a quotient of the order would leave tm_div's exact range
FK_TM_FN int tm_fill_class(TmClass& c, const int32_t* M, int n, int nbn, int col0, int group_m) {
  int total = 0;
  for (int i = 0; i < TM_MAX_GROUP; ++i) {
    c.before[i] = total;
    const int nbm = i < n ? (M[i] + TM_BM - 1) / TM_BM : 0;
    c.nbm[i] = nbm;
    const int last = nbm > 0 ? nbm - ((nbm - 1) / group_m) * group_m : 1;   // 1 .. group_m
    c.last_mul[i] = tm_magic((uint32_t)last);
    total += nbm * nbn;
  }
  c.before[TM_MAX_GROUP] = total;
  c.col0 = col0;
  c.per_group = group_m * nbn;
  c.per_group_mul = tm_magic((uint32_t)c.per_group);
  c.group_m_mul = tm_magic((uint32_t)group_m);
  // t / per_group with t < total; rem / depth with rem < per_group and depth <= group_m
  if (!tm_div_domain((uint64_t)total, (uint64_t)c.per_group) || !tm_div_domain((uint64_t)c.per_group, (uint64_t)group_m)) return -1;
  return total;
}

FK_TM_FN void tm_fill_grid(TileEntry& e, uint32_t grid) {
  e.grid = grid;
  e.xq = grid >> 3;
  e.xr = grid & 7;
}
