// Stand-alone check of the tile walk of csrc/gemm_tile_map.h on the CPU (built and run by tests/test_gemm_walk_map.py, with
// -fsanitize=address,undefined where the compiler has them).  G workgroups take the places g, g + G, ... of a launch that
// has one place per tile: over a sweep of (tiles, G) the workgroups' lists together hold every place -- and through the
// launch's tile order every tile -- exactly once; place b is entry b / G of workgroup b % G, which is the workgroup (CU)
// that list scheduling hands block b of the one-workgroup-per-tile launch to on a grid of equal tiles; and the tile a place
// names is the one blockIdx.x = place computes in that launch (tm_xcd_chunk + tm_tile; mixed grids: the per-XCD table).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../gpt_image_edit_amd/csrc/gemm_tile_map.h"

static long failures = 0, checked = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    ++checked;                                            \
    if (!(cond)) {                                        \
      if (++failures <= 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } \
    }                                                     \
  } while (0)

typedef std::tuple<int, int, int, int> Tile;   // class (0: 256 wide, 1: 128 wide), problem, m0, n0

// the tile of place b as the one-workgroup-per-tile kernels compute it from blockIdx.x = b
static Tile tile_of_place(const TileEntry& e, bool mixed, uint32_t b) {
  int pi, m0, n0;
  if (!mixed) {
    tm_tile(e, e.cls[0], 256, tm_xcd_chunk(e, b), pi, m0, n0);
    return Tile(0, pi, m0, n0);
  }
  const TileEntry::Xcd& x = e.xcd[b & 7];
  const int idx = (int)(b >> 3);
  if (idx < x.big_cnt) {
    tm_tile(e, e.cls[0], 256, x.big_start + idx, pi, m0, n0);
    return Tile(0, pi, m0, n0);
  }
  tm_tile(e, e.cls[1], 128, x.small_start + idx - x.big_cnt, pi, m0, n0);
  return Tile(1, pi, m0, n0);
}

// every tile of the launch, from the problems' shapes alone
static std::set<Tile> all_tiles(const std::vector<int32_t>& Ms, int N, int big_cols, bool mixed) {
  std::set<Tile> s;
  for (int pi = 0; pi < (int)Ms.size(); ++pi)
    for (int m0 = 0; m0 < Ms[pi]; m0 += 256) {
      const int wide = mixed ? big_cols : (N + 255) / 256;
      for (int c = 0; c < wide; ++c) s.insert(Tile(0, pi, m0, c * 256));
      if (mixed)
        for (int n0 = big_cols * 256; n0 < N; n0 += 128) s.insert(Tile(1, pi, m0, n0));
    }
  return s;
}

static void check_walk(const std::vector<int32_t>& Ms, int N, int group_m, int big_cols, const std::vector<int>& Gs) {
  const bool mixed = big_cols > 0;
  const int n = (int)Ms.size();
  TileEntry e = {};
  e.n = n;
  e.group_m = tm_group_m(Ms.data(), n, group_m);
  int places;
  if (mixed) {
    const int tb = tm_fill_class(e.cls[0], Ms.data(), n, big_cols, 0, e.group_m);
    const int ts = tm_fill_class(e.cls[1], Ms.data(), n, (N - big_cols * 256 + 127) / 128, big_cols * 256, e.group_m);
    CHECK(tb >= 0 && ts >= 0, "class fill N %d big_cols %d", N, big_cols);
    if (!tm_fill_mix(e, tb, ts)) return;   // the launcher falls back to a plain grid
    places = tb + ts;
  } else {
    places = tm_fill_class(e.cls[0], Ms.data(), n, (N + 255) / 256, 0, e.group_m);
    CHECK(places >= 0, "class fill N %d", N);
  }
  tm_fill_grid(e, (uint32_t)places);
  const std::set<Tile> want = all_tiles(Ms, N, big_cols, mixed);
  CHECK((int)want.size() == places, "N %d big_cols %d: %d places for %d tiles", N, big_cols, places, (int)want.size());
  // the place order of a mixed grid is big tiles first: no place behind a small tile names a big one.  A workgroup takes its
  // places in rising order whatever G is, so its list changes shape at most once, from big to small
  if (mixed) {
    int ti;
    for (int b = 0; b + 1 < places; ++b)
      CHECK(!(tm_mix_place(e, (uint32_t)b, ti) && !tm_mix_place(e, (uint32_t)(b + 1), ti)), "N %d big_cols %d: place %d is big behind a small one",
            N, big_cols, b + 1);
  }
  for (int G : Gs) {
    std::vector<int> seen(places, 0);
    std::set<Tile> got;
    long entries = 0;
    for (int g = 0; g < G; ++g) {
      const int cnt = tm_walk_count((uint32_t)places, (uint32_t)G, (uint32_t)g);
      CHECK(cnt == (g < places ? (places - g + G - 1) / G : 0), "tiles %d G %d workgroup %d: %d entries", places, G, g, cnt);
      bool small_before = false;
      for (int i = 0; i < cnt; ++i, ++entries) {
        const uint32_t b = tm_walk_place((uint32_t)G, (uint32_t)g, (uint32_t)i);
        CHECK(b < (uint32_t)places && (int)(b % G) == g && (int)(b / G) == i, "tiles %d G %d: entry %d of workgroup %d is place %u",
              places, G, i, g, b);
        if (b >= (uint32_t)places) continue;
        ++seen[b];
        const Tile t = tile_of_place(e, mixed, b);
        got.insert(t);
        if (mixed) {
          int ti;
          const bool small = tm_mix_place(e, b, ti);
          int pi, m0, n0;
          tm_tile(e, e.cls[small ? 1 : 0], small ? 128 : 256, ti, pi, m0, n0);
          CHECK(Tile(small ? 1 : 0, pi, m0, n0) == t, "tiles %d G %d place %u: tm_mix_place names another tile", places, G, b);
          // a workgroup whose places stay on one XCD (G % 8 == 0: the device's grids) never returns to a big tile
          if (G % 8 == 0) CHECK(!(small_before && !small), "tiles %d G %d workgroup %d: a big tile behind a small one", places, G, g);
          small_before = small_before || small;
        }
      }
    }
    CHECK(entries == places, "tiles %d G %d: %ld entries", places, G, entries);
    for (int b = 0; b < places; ++b) CHECK(seen[b] == 1, "tiles %d G %d: place %d taken %d times", places, G, b, seen[b]);
    CHECK(got == want, "tiles %d G %d: the places do not name every tile once (%d of %d)", places, G, (int)got.size(), (int)want.size());
  }
}

// --places N big_cols group_m M...: one line "small tile" per place of that mixed launch, from tm_fill_class / tm_fill_mix /
// tm_mix_place themselves (tests/test_gemm_large_host.py holds the restatement in tests/gemm_large_cases.py against it)
static int print_places(int argc, char** argv) {
  if (argc < 6) return 2;
  const int N = atoi(argv[2]), big_cols = atoi(argv[3]), group_m = atoi(argv[4]);
  std::vector<int32_t> Ms;
  for (int i = 5; i < argc; ++i) Ms.push_back(atoi(argv[i]));
  const int n = (int)Ms.size();
  if (n > TM_MAX_GROUP || big_cols < 1 || big_cols * 256 >= N) return 2;
  TileEntry e = {};
  e.n = n;
  e.group_m = tm_group_m(Ms.data(), n, group_m);
  const int tb = tm_fill_class(e.cls[0], Ms.data(), n, big_cols, 0, e.group_m);
  const int ts = tm_fill_class(e.cls[1], Ms.data(), n, (N - big_cols * 256 + 127) / 128, big_cols * 256, e.group_m);
  if (tb < 0 || ts < 0 || !tm_fill_mix(e, tb, ts)) return 3;
  printf("%d %d\n", tb, ts);
  for (int b = 0; b < tb + ts; ++b) {
    int ti;
    const bool small = tm_mix_place(e, (uint32_t)b, ti);
    printf("%d %d\n", small ? 1 : 0, ti);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "--places") return print_places(argc, argv);
  if (argc > 1) return 0;   // any other argument: "can this build start here?" (the test falls back to the plain build if not)
  const std::vector<int> Gs = {1, 2, 3, 4, 5, 7, 8, 16, 24, 31, 32, 64, 104, 256, 304, 1000};
  // pure 256 x 256 grids: the walk tests' own (9 tiles), the flagship MLP-up grid (480), ragged and grouped ones
  check_walk({768}, 768, 8, 0, Gs);
  check_walk({2560}, 12288, 8, 0, Gs);
  check_walk({700}, 1024, 8, 0, Gs);
  check_walk({512, 256}, 768, 8, 0, Gs);
  check_walk({2048, 512}, 12288, 8, 0, Gs);
  check_walk({300, 520, 700, 1}, 1280, 1, 0, Gs);
  check_walk({5632}, 3072, 64, 0, Gs);
  for (int rows = 1; rows <= 6; ++rows)
    for (int cols = 1; cols <= 7; ++cols) check_walk({rows * 256 - 5}, cols * 256, 3, 0, Gs);
  // mixed grids: the flagship fused QKV grid (256 big + 208 small at big_cols 26 .. every split), the walk tests' own, ragged N
  for (int cb = 1; cb < 36; ++cb) check_walk({2560}, 9216, 8, cb, Gs);
  for (int cb = 1; cb < 4; ++cb) {
    check_walk({768}, 1024, 8, cb, Gs);
    check_walk({700}, 1024 - 128 + 8, 8, cb, Gs);
    check_walk({2048, 512}, 1024, 2, cb, Gs);
  }
  printf("%ld checks, %ld failures\n", checked, failures);
  return failures ? 1 : 0;
}
