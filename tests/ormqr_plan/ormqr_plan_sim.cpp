// Walks the launch schedule of capi_dormqr's thin path (capital_amd/csrc/ormqr_plan.h) and checks it the way the kernels rely on it.  Commands on stdin:
//   consts                          -> "nb=<NB> tile=<TILE> waves=<WAVES> round=<ROUND>"
//   plan <m> <k> <trans> <cus> <rb> -> one line of key=value pairs:
//     panels, launches         what the schedule holds
//     refl_miss                reflectors that do not lie in exactly one panel
//     order_bad                panels out of order (ascending for trans = 1, descending for 0), empty, wider than NB, or with the wrong live rows
//     row_miss                 (panel, live row) pairs that the walk of the Gram kernel (slice z, its rounds, a tile per wave) does not visit exactly once,
//                              or that do not lie inside row_begin(z) .. row_begin(z + 1)
//     empty                    slices without a row
//     slabs                    the largest slab count of a panel (must not exceed cus)
//     ws                       workspace_doubles(m, rb, cus)
//     touched                  one past the last double of the workspace the walk reads or writes (Z and the slabs of every panel)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ormqr_plan.h"

namespace op = ormqr_plan;

static void plan(int64_t m, int64_t k, int trans, int cus, int rb) {
  std::vector<int> in_panel((size_t)k, 0);
  int64_t refl_miss = 0, order_bad = 0, row_miss = 0, empty = 0, slabs = 0, touched = op::Z_DOUBLES;
  const int64_t P = op::num_panels(k);
  int64_t last = trans ? -1 : k;
  for (int64_t step = 0; step < P; ++step) {
    const op::Panel pn = op::panel(m, k, trans != 0, step);
    if (pn.nb < 1 || pn.nb > op::NB || pn.j0 % op::NB != 0 || pn.j0 < 0 || pn.j0 + pn.nb > k || pn.rows != m - pn.j0) ++order_bad;
    if (trans ? pn.j0 <= last : pn.j0 >= last) ++order_bad;
    if (pn.j0 + op::NB < k && pn.nb != op::NB) ++order_bad;          // only the last panel may be short
    last = pn.j0;
    for (int64_t j = pn.j0; j < pn.j0 + pn.nb && j < k; ++j) ++in_panel[(size_t)j];
    const op::Slices sl = op::slices(pn.rows, cus);
    if (sl.S > slabs) slabs = sl.S;
    if (sl.S < 1 || sl.S > cus) ++order_bad;
    std::vector<int> hit((size_t)pn.rows, 0);
    for (int z = 0; z < sl.S; ++z) {
      const int64_t rd0 = op::round_begin(sl, z), rd1 = op::round_begin(sl, z + 1);
      const int64_t r0 = op::row_begin(sl, pn.rows, z), r1 = op::row_begin(sl, pn.rows, z + 1);
      if (r1 <= r0) ++empty;
      const int64_t tend = rd1 * op::WAVES < sl.tiles ? rd1 * op::WAVES : sl.tiles;
      for (int w = 0; w < op::WAVES; ++w)
        for (int64_t tile = rd0 * op::WAVES + w; tile < tend; tile += op::WAVES)
          for (int64_t i = tile * op::TILE; i < (tile + 1) * op::TILE && i < pn.rows; ++i) {
            ++hit[(size_t)i];
            if (i < r0 || i >= r1) ++row_miss;
          }
      const int64_t end = op::slab_offset(rb, z) + op::slab_doubles(rb);
      if (end > touched) touched = end;
    }
    if (op::round_begin(sl, 0) != 0 || op::round_begin(sl, sl.S) != sl.rounds) ++order_bad;
    for (int v : hit)
      if (v != 1) ++row_miss;
  }
  if (P > 0 && (trans ? last != (P - 1) * op::NB : last != 0)) ++order_bad;
  for (int v : in_panel)
    if (v != 1) ++refl_miss;
  printf("panels=%lld launches=%lld refl_miss=%lld order_bad=%lld row_miss=%lld empty=%lld slabs=%lld ws=%lld touched=%lld\n", (long long)P,
         (long long)op::num_launches(k), (long long)refl_miss, (long long)order_bad, (long long)row_miss, (long long)empty, (long long)slabs,
         (long long)op::workspace_doubles(m, rb, cus), (long long)touched);
}

int main() {
  char cmd[32];
  while (scanf("%31s", cmd) == 1) {
    long long m = 0, k = 0;
    int trans = 0, cus = 0, rb = 0;
    if (!strcmp(cmd, "consts")) printf("nb=%d tile=%d waves=%d round=%d\n", op::NB, op::TILE, op::WAVES, op::ROUND);
    else if (!strcmp(cmd, "plan") && scanf("%lld %lld %d %d %d", &m, &k, &trans, &cus, &rb) == 5) plan(m, k, trans, cus, rb);
    else return 2;
  }
  return 0;
}
