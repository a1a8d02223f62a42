// Walks the launch schedule of capi_dchud / capi_dchud_inv (capital_amd/csrc/chud_plan.h) and checks it the way the kernels rely on it.  Commands on stdin:
//   consts                -> "b=<B> cols=<COLS> rows=<ROWS> kchunk=<KCHUNK>"
//   plan <n>              -> one line of key=value pairs:
//     panels, launches, applies        what the schedule holds (applies: apply workgroups over all panels)
//     step_miss                        steps that do not lie in exactly one panel, or whose panel_of() is another one
//     col_miss                         (panel, trailing column) pairs that do not lie in exactly one apply workgroup of the panel
//     bad                              panels that are empty, longer than B or out of order; applies that are empty, wider than COLS, reach into
//                                      the panel's own columns or beyond n
//   inv <k0> <k1>         -> groups, row_miss (rows of [k0, k1) not owned by exactly one thread), bad (a workgroup whose first chunk starts behind its
//                            first row, or before k0, or whose chunks are not aligned to k0)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "chud_plan.h"

namespace cp = chud_plan;

static void plan(int64_t n) {
  std::vector<int> in_panel((size_t)n, 0);
  std::vector<int> hit((size_t)n, 0);
  int64_t applies = 0, step_miss = 0, col_miss = 0, bad = 0, last_end = 0;
  const int64_t P = cp::num_panels(n);
  for (int64_t p = 0; p < P; ++p) {
    const cp::Panel pn = cp::panel(n, p);
    if (pn.k0 != last_end || pn.k1 <= pn.k0 || pn.k1 - pn.k0 > cp::B || pn.k1 > n) ++bad;
    last_end = pn.k1;
    for (int64_t k = pn.k0; k < pn.k1; ++k) {
      ++in_panel[(size_t)k];
      if (cp::panel_of(k) != p) ++step_miss;
    }
    const int64_t na = cp::num_applies(n, pn);
    applies += na;
    std::fill(hit.begin(), hit.end(), 0);
    for (int64_t g = 0; g < na; ++g) {
      const cp::Apply a = cp::apply(n, pn, g);
      if (a.j1 <= a.j0 || a.j1 - a.j0 > cp::COLS || a.j0 < pn.k1 || a.j1 > n) { ++bad; continue; }
      for (int64_t j = a.j0; j < a.j1; ++j) ++hit[(size_t)j];
    }
    for (int64_t j = 0; j < n; ++j)
      if (hit[(size_t)j] != (j >= pn.k1 ? 1 : 0)) ++col_miss;
  }
  if (last_end != n) ++bad;
  for (int64_t k = 0; k < n; ++k)
    if (in_panel[(size_t)k] != 1) ++step_miss;
  printf("panels=%lld launches=%lld applies=%lld step_miss=%lld col_miss=%lld bad=%lld\n", (long long)P, (long long)cp::num_launches(n), (long long)applies,
         (long long)step_miss, (long long)col_miss, (long long)bad);
}

static void inv(int64_t k0, int64_t k1) {
  std::vector<int> own((size_t)(k1 - k0), 0);
  int64_t bad = 0, row_miss = 0;
  const int64_t G = cp::inv_groups(k0, k1);
  for (int64_t g = 0; g < G; ++g) {
    const int64_t c0 = k0 + g * cp::ROWS, ks = cp::inv_first_step(k0, g);
    if (ks > c0 || ks < k0 || (ks - k0) % cp::KCHUNK != 0 || c0 - ks >= cp::KCHUNK) ++bad;
    for (int64_t t = 0; t < cp::ROWS; ++t)
      if (c0 + t < k1) ++own[(size_t)(c0 + t - k0)];
  }
  for (int v : own)
    if (v != 1) ++row_miss;
  printf("groups=%lld row_miss=%lld bad=%lld\n", (long long)G, (long long)row_miss, (long long)bad);
}

int main() {
  char cmd[32];
  while (scanf("%31s", cmd) == 1) {
    long long a = 0, b = 0;
    if (!strcmp(cmd, "consts")) printf("b=%d cols=%d rows=%d kchunk=%d\n", cp::B, cp::COLS, cp::ROWS, cp::KCHUNK);
    else if (!strcmp(cmd, "plan") && scanf("%lld", &a) == 1) plan(a);
    else if (!strcmp(cmd, "inv") && scanf("%lld %lld", &a, &b) == 2) inv(a, b);
    else return 2;
  }
  return 0;
}
