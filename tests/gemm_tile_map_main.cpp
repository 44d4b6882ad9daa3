// Stand-alone check of csrc/gemm_tile_map.h on the CPU (built and run by tests/test_gemm_tile_map.py, with
// -fsanitize=address,undefined where the compiler has them).  The reference below is the device code the header replaced,
// kept verbatim: the tile order with its divisions, the XCD chunking from the grid size, and fk_row_offset.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../gpt_image_edit_amd/csrc/gemm_tile_map.h"

namespace ref {
constexpr int BM = 256, FK_MAX_GROUP = 4;
using std::min;
struct fk_rows { int64_t ld, rows_per_batch, batch_stride; };
struct Prob { int M, N; };
struct GroupArgs {
  Prob p[FK_MAX_GROUP];
  int tiles_before[FK_MAX_GROUP + 1];
  int n;
  int big_cols;
  int small_before[FK_MAX_GROUP + 1];
  int xcd_big_start[8], xcd_big_cnt[8], xcd_small_start[8];
  int group_m;
};
template <int BN>
void tile_of(const GroupArgs& ga, const int (&before)[FK_MAX_GROUP + 1], int t, int nbn, int col0, int& pi, int& m0, int& n0) {
  pi = 0;
  for (int i = 1; i < FK_MAX_GROUP; ++i)
    if (i < ga.n && t >= before[i]) pi = i;
  const Prob& p = ga.p[pi];
  t -= before[pi];
  const int nbm = (p.M + BM - 1) / BM;
  const int per_group = ga.group_m * nbn;
  const int g = t / per_group;
  const int first_m = g * ga.group_m;
  const int gm = min(nbm - first_m, ga.group_m);
  const int rem = t - g * per_group;
  m0 = (first_m + rem % gm) * BM;
  n0 = col0 + (rem / gm) * BN;
}
int xcd_chunk_index(int gridDim_x, int blockIdx_x) {
  const int nwg = gridDim_x;
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = blockIdx_x & 7, idx = blockIdx_x >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}
int64_t fk_row_offset(const fk_rows& r, int64_t m) {
  if (r.rows_per_batch <= 0) return m * r.ld;
  int64_t b = m / r.rows_per_batch;
  return b * r.batch_stride + (m - b * r.rows_per_batch) * r.ld;
}
}  // namespace ref

static long failures = 0, checked = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    ++checked;                                            \
    if (!(cond)) {                                        \
      if (++failures <= 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } \
    }                                                     \
  } while (0)

// one launch: n problems of Ms x N, tile width BN (0: mixed grid with big_cols), split: two workgroups per tile
static void check_grid(const std::vector<int>& Ms, int N, int group_m, int BN, int big_cols, bool split) {
  const int n = (int)Ms.size();
  ref::GroupArgs ra = {};
  ra.n = n;
  ra.group_m = group_m;
  for (int i = 0; i < ref::FK_MAX_GROUP; ++i) ra.p[i] = {Ms[i < n ? i : 0], N};
  TileEntry e = {};
  e.n = n;
  std::vector<int32_t> M32(Ms.begin(), Ms.end());
  e.group_m = tm_group_m(M32.data(), n, group_m);
  if (BN) {
    int total = 0;
    for (int i = 0; i < ref::FK_MAX_GROUP; ++i) {
      ra.tiles_before[i] = total;
      if (i < n) total += ((Ms[i] + 255) / 256) * ((N + BN - 1) / BN);
    }
    ra.tiles_before[ref::FK_MAX_GROUP] = total;
    const int got = tm_fill_class(e.cls[0], M32.data(), n, (N + BN - 1) / BN, 0, e.group_m);
    CHECK(got == total, "tile count %d != %d", got, total);
    const int grid = split ? 2 * total : total;
    tm_fill_grid(e, (uint32_t)grid);
    std::vector<char> seen(total, 0);
    for (int b = 0; b < grid; ++b) {
      int t = ref::xcd_chunk_index(grid, b), t2 = tm_xcd_chunk(e, (uint32_t)b);
      CHECK(t == t2, "chunk index of workgroup %d: %d != %d", b, t2, t);
      if (split) t >>= 1;
      int pi, m0, n0, qi, q0, r0;
      if (BN == 256) ref::tile_of<256>(ra, ra.tiles_before, t, (N + 255) / 256, 0, pi, m0, n0);
      else ref::tile_of<128>(ra, ra.tiles_before, t, (N + 127) / 128, 0, pi, m0, n0);
      tm_tile(e, e.cls[0], BN, t, qi, q0, r0);
      CHECK(pi == qi && m0 == q0 && n0 == r0, "M0 %d n %d N %d gm %d BN %d tile %d: (%d,%d,%d) != (%d,%d,%d)", Ms[0], n, N, group_m,
            BN, t, qi, q0, r0, pi, m0, n0);
      CHECK(m0 < Ms[pi] && n0 < N, "tile outside its problem");
      seen[t] = 1;
    }
    for (int t = 0; t < total; ++t) CHECK(seen[t], "tile %d not covered", t);
    return;
  }
  // mixed grid: the launcher's tables, then gemm_mix_kernel's selection
  const int ncols128 = (N - big_cols * 256 + 127) / 128;
  int tb = 0, ts = 0;
  for (int i = 0; i < ref::FK_MAX_GROUP; ++i) {
    ra.tiles_before[i] = tb;
    ra.small_before[i] = ts;
    if (i < n) {
      const int nbm = (Ms[i] + 255) / 256;
      tb += nbm * big_cols;
      ts += nbm * ncols128;
    }
  }
  ra.tiles_before[ref::FK_MAX_GROUP] = tb;
  ra.small_before[ref::FK_MAX_GROUP] = ts;
  ra.big_cols = big_cols;
  const int W = tb + ts;
  int bs = 0, ss = 0;
  for (int x = 0; x < 8; ++x) {
    const int wx = W / 8 + (x < W % 8 ? 1 : 0), bx = tb / 8 + (x < tb % 8 ? 1 : 0);
    if (wx < bx) return;   // the launcher refuses this split
    ra.xcd_big_start[x] = bs;
    ra.xcd_big_cnt[x] = bx;
    ra.xcd_small_start[x] = ss;
    e.xcd[x] = {bs, bx, ss, 0};
    bs += bx;
    ss += wx - bx;
  }
  CHECK(tm_fill_class(e.cls[0], M32.data(), n, big_cols, 0, e.group_m) == tb, "big tile count");
  CHECK(tm_fill_class(e.cls[1], M32.data(), n, ncols128, big_cols * 256, e.group_m) == ts, "small tile count");
  for (int b = 0; b < W; ++b) {
    const int xcd = b & 7, idx = b >> 3;
    const int nbig = ra.xcd_big_cnt[xcd];
    int pi, m0, n0, qi, q0, r0;
    if (idx < nbig) {
      ref::tile_of<256>(ra, ra.tiles_before, ra.xcd_big_start[xcd] + idx, ra.big_cols, 0, pi, m0, n0);
      tm_tile(e, e.cls[0], 256, e.xcd[xcd].big_start + idx, qi, q0, r0);
    } else {
      ref::tile_of<128>(ra, ra.small_before, ra.xcd_small_start[xcd] + idx - nbig, (ra.p[0].N - ra.big_cols * 256 + 127) / 128,
                        ra.big_cols * 256, pi, m0, n0);
      tm_tile(e, e.cls[1], 128, e.xcd[xcd].small_start + idx - e.xcd[xcd].big_cnt, qi, q0, r0);
    }
    CHECK(pi == qi && m0 == q0 && n0 == r0, "mixed M0 %d n %d N %d gm %d big %d workgroup %d: (%d,%d,%d) != (%d,%d,%d)", Ms[0], n, N,
          group_m, big_cols, b, qi, q0, r0, pi, m0, n0);
  }
}

static void check_all_forms(const std::vector<int>& Ms, int N, int group_m) {
  check_grid(Ms, N, group_m, 128, 0, false);
  if (N % 256 == 0) {
    check_grid(Ms, N, group_m, 256, 0, false);
    check_grid(Ms, N, group_m, 256, 0, true);    // split-K pairs
    for (int cb = 1; cb < N / 256; ++cb) check_grid(Ms, N, group_m, 0, cb, false);
  } else {
    check_grid(Ms, N, group_m, 256, 0, false);   // the order itself does not need N % 256 == 0
  }
}

static void check_rows(int64_t ld, int64_t rpb, int64_t bs, int64_t M, int expect_flat) {
  const ref::fk_rows r = {ld, rpb, bs};
  const bool flat = tm_rows_flat(ld, rpb, bs, M);
  if (expect_flat >= 0) CHECK(flat == (expect_flat != 0), "flat(ld %ld rpb %ld bs %ld M %ld) = %d", (long)ld, (long)rpb, (long)bs, (long)M, (int)flat);
  bool same = true;
  for (int64_t m = 0; m < M; ++m) same = same && ref::fk_row_offset(r, m) == m * ld;
  if (flat) CHECK(same, "rows marked flat are not: ld %ld rpb %ld bs %ld M %ld", (long)ld, (long)rpb, (long)bs, (long)M);
}

int main(int argc, char**) {
  if (argc > 1) return 0;   // any argument: "can this build start here?" (the test falls back to the plain build if not)
  // 1. the multiply-shift quotients
  for (uint32_t d = 1; d <= 4096; ++d) {
    const uint32_t m = tm_magic(d);
    uint32_t q = 0, r = 0;   // t = q d + r
    for (uint32_t t = 0; t < 65536; ++t) {
      if (tm_div(t, m) != q) { CHECK(false, "%u / %u: %u != %u", t, d, tm_div(t, m), q); break; }
      if (++r == d) { r = 0; ++q; }
    }
    ++checked;
  }
  // the domain test the launcher relies on, at its edge
  for (uint64_t d : {2ull, 3ull, 4097ull, 32768ull, 65535ull}) {
    const uint64_t tmax = (1ull << 31) / d;
    CHECK(tm_div_domain(tmax, d) && !tm_div_domain(tmax + 1, d), "domain edge d %lu", (unsigned long)d);
    const uint32_t m = tm_magic((uint32_t)d);
    for (uint64_t t = tmax > 70000 ? tmax - 70000 : 0; t < tmax; ++t)
      if (tm_div((uint32_t)t, m) != (uint32_t)(t / d)) { CHECK(false, "%lu / %lu", (unsigned long)t, (unsigned long)d); break; }
  }

  // 2. the tile of every workgroup: flagship grids ...
  for (int N : {3072, 9216, 12288})
    for (int gm : {1, 8, 64}) {
      check_all_forms({2560}, N, gm);
      check_all_forms({2048, 512}, N, gm);
    }
  // ... and ragged ones, 1 - 4 problems
  const int Mr[3] = {300, 520, 700};
  for (int N : {384, 1280})
    for (int gm : {1, 8, 64})
      for (int n = 1; n <= 4; ++n)
        for (int first = 0; first < 3; ++first) {
          std::vector<int> Ms;
          for (int i = 0; i < n; ++i) Ms.push_back(Mr[(first + i) % 3]);
          check_all_forms(Ms, N, gm);
        }
  check_all_forms({8704, 300}, 3072, 8);    // deeper than one group, last group partial (34 row tiles)
  check_all_forms({8704, 300}, 3072, 5);

  // 3. flat rows against fk_row_offset, row by row
  check_rows(3072, 0, 0, 2560, 1);                  // one batch
  check_rows(3072, -1, 12345, 700, 1);
  check_rows(3072, 2560, 2560 * 3072, 2560, 1);     // what the blocks pass at B = 1
  check_rows(3072, 2048, 2560 * 3072, 2048, 1);     // image slice of a joint buffer, B = 1
  check_rows(3072, 512, 2560 * 3072, 512, 1);       // text slice, B = 1
  check_rows(3072, 136, 160 * 3072, 136, 1);
  check_rows(3072, 24, 160 * 3072, 24, 1);
  check_rows(3072, 136, 160 * 3072, 272, 0);        // the same slices at B = 2: a gap between the batches
  check_rows(3072, 24, 160 * 3072, 48, 0);
  check_rows(3072, 160, 160 * 3072, 320, 1);        // B = 2 without a gap
  check_rows(3080, 160, 160 * 3080 + 8, 161, 0);
  for (int64_t ld : {64, 3072})
    for (int64_t rpb : {-1, 0, 1, 7, 24, 136, 160, 300})
      for (int64_t gap : {0, 8, 4096})
        for (int64_t M : {1, 7, 24, 25, 136, 160, 161, 300, 520})
          check_rows(ld, rpb, rpb > 0 ? rpb * ld + gap : gap, M, -1);

  printf("%ld checks, %ld failures\n", checked, failures);
  return failures ? 1 : 0;
}
