// Runs capital_amd/csrc/tri_thin_plan.h on the host (tests/test_tri_thin_plan.py).  One case per input line:
//   plan  shape trans m n slices      -> the slices' tile ranges walked tile by tile: counts, weights, coverage
//   cols  col0 count                  -> packed column starts and alignment classes of columns col0 .. col0 + count - 1
#include <stdio.h>
#include <string.h>
#include <vector>
#include "tri_thin_plan.h"

namespace tp = tri_thin_plan;

static int run_plan(int shape, int trans, long long m, long long n, int slices) {
  const tp::Plan P = tp::make_plan(shape, trans, m, n);
  std::vector<int64_t> pos(tp::MAX_SLICES + 1, -1);
  const int S = tp::make_slices(P, slices, pos.data());
  const int64_t T = tp::total_tiles(P);
  // every tile number 0 .. T - 1 is walked once, in order; locate() must agree with the walk
  const bool mark = m * n <= 4000000;          // small blocks: count how often every element is covered
  std::vector<unsigned char> hit(mark ? (size_t)(m * n) : 0, 0);
  int64_t walked = 0, elems = 0, max_slice = 0, max_tile = 0, bad = 0, g = 0, c = 0;
  for (int s = 0; s < S; ++s) {
    if (pos[s] != walked || pos[s + 1] < pos[s]) ++bad;
    int64_t in_slice = 0;
    if (pos[s] < pos[s + 1]) {
      int64_t lg, lc;
      tp::locate(P, pos[s], &lg, &lc);
      if (lg != g || lc != c) ++bad;
    }
    for (int64_t q = pos[s]; q < pos[s + 1]; ++q) {
      if (g >= P.ngroups || c < tp::first_tile(P, g) || c >= tp::first_tile(P, g) + tp::group_tiles(P, g)) { ++bad; break; }
      const int64_t w = tp::tile_elems(P, g, c);
      if (w <= 0) ++bad;
      if (w > max_tile) max_tile = w;
      in_slice += w;
      if (mark) {
        int64_t r0, r1, c0, c1;
        tp::tile_rect(P, g, c, &r0, &r1, &c0, &c1);
        for (int64_t j = c0; j < c1; ++j)
          for (int64_t i = r0; i < r1; ++i)
            if (!P.tri || i <= j) ++hit[(size_t)(i + j * m)];
      }
      ++walked;
      if (++c == tp::first_tile(P, g) + tp::group_tiles(P, g)) { ++g; c = g < P.ngroups ? tp::first_tile(P, g) : 0; }
    }
    elems += in_slice;
    if (in_slice > max_slice) max_slice = in_slice;
  }
  int64_t miss = 0;
  if (mark)
    for (int64_t j = 0; j < n; ++j)
      for (int64_t i = 0; i < m; ++i)
        if (hit[(size_t)(i + j * m)] != ((!P.tri || i <= j) ? 1 : 0)) ++miss;
  printf("S=%d tiles=%lld walked=%lld elems=%lld total=%lld max_slice=%lld max_tile=%lld tile_cap=%d bad=%lld marked=%d miss=%lld end_group=%lld groups=%lld\n", S,
         (long long)T, (long long)walked, (long long)elems, (long long)tp::total_elems(P), (long long)max_slice, (long long)max_tile, tp::GROUP * tp::DEPTH,
         (long long)bad, (int)mark, (long long)miss, (long long)g, (long long)P.ngroups);
  return 0;
}

int main() {
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    char what[16];
    long long a, b, c, d, e;
    const int k = sscanf(line, "%15s %lld %lld %lld %lld %lld", what, &a, &b, &c, &d, &e);
    if (k == 6 && !strcmp(what, "plan")) run_plan((int)a, (int)b, c, d, (int)e);
    else if (k == 3 && !strcmp(what, "cols")) {
      for (long long x = a; x < a + b; ++x)
        printf("col %lld start=%lld offset=%lld class=%d\n", x, (long long)tp::packed_col_start(x), (long long)tp::packed_col_offset(a, x - a),
               tp::align_class(tp::packed_col_start(x)));
    } else { fprintf(stderr, "bad line: %s", line); return 2; }
  }
  return 0;
}
