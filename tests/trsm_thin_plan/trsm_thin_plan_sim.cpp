// Walks the step list of capi_dtrsm_thin (capital_amd/csrc/trsm_thin_plan.h) and checks it the way the kernels rely on it.  Commands on stdin:
//   leaf              -> "leaf=<LEAF>"
//   plan <trans> <n>  -> one line of key=value pairs:
//     steps, leaves, products, max_leaf, depth      what the list holds; depth = levels of the recursion above the leaves
//     elems, total                                  elements of the triangle covered by the steps (by sums) / n (n + 1) / 2
//     marked, miss                                  n^2 <= 4e6: counted element by element; miss = elements not covered exactly once
//     bad                                           steps that break a rule: a leaf larger than LEAF or off the diagonal, a product that reaches
//                                                   the diagonal or leaves the triangle, reads a row that no earlier leaf solved or updates a solved
//                                                   one, a leaf whose rows have not received all their products, a row solved twice or never
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "trsm_thin_plan.h"

namespace sp = trsm_thin_plan;

static int depth_of(int64_t n) {
  if (n <= sp::LEAF) return 0;
  const int64_t n1 = sp::split(n);
  const int a = depth_of(n1), b = depth_of(n - n1);
  return 1 + (a > b ? a : b);
}

static void plan(int trans, int64_t n) {
  const bool mark = n * n <= 4000000;
  std::vector<unsigned char> cover(mark ? (size_t)(n * n) : 0, 0);
  std::vector<unsigned char> solved((size_t)n, 0);
  std::vector<int64_t> got((size_t)n, 0);                // triangle elements applied to the row by products so far
  int64_t steps = 0, nleaves = 0, products = 0, max_leaf = 0, elems = 0, bad = 0;
  sp::for_each_step(trans, 0, n, [&](const sp::Step& s) {
    ++steps;
    if (s.kind == sp::STEP_LEAF) {
      ++nleaves;
      if (s.m > max_leaf) max_leaf = s.m;
      if (s.m != s.n || s.row0 != s.col0 || s.m < 1 || s.m > sp::LEAF || s.row0 < 0 || s.row0 + s.m > n) { ++bad; return 0; }
      elems += s.m * (s.m + 1) / 2;
      for (int64_t i = s.row0; i < s.row0 + s.m; ++i) {
        const int64_t want = trans ? s.row0 : n - (s.row0 + s.m);          // the column above the leaf / the row right of it
        if (solved[(size_t)i] || got[(size_t)i] != want) ++bad;
        solved[(size_t)i] = 1;
      }
      if (mark)
        for (int64_t j = s.col0; j < s.col0 + s.n; ++j)
          for (int64_t i = s.row0; i <= j; ++i) ++cover[(size_t)(i + j * n)];
    } else {
      ++products;
      if (s.m < 1 || s.n < 1 || s.row0 < 0 || s.row0 + s.m > s.col0 || s.col0 + s.n > n) { ++bad; return 0; }
      elems += s.m * s.n;
      const int64_t in0 = trans ? s.row0 : s.col0, inn = trans ? s.m : s.n, out0 = trans ? s.col0 : s.row0, outn = trans ? s.n : s.m;
      for (int64_t i = in0; i < in0 + inn; ++i) if (!solved[(size_t)i]) ++bad;
      for (int64_t i = out0; i < out0 + outn; ++i) { if (solved[(size_t)i]) ++bad; got[(size_t)i] += inn; }
      if (mark)
        for (int64_t j = s.col0; j < s.col0 + s.n; ++j)
          for (int64_t i = s.row0; i < s.row0 + s.m; ++i) ++cover[(size_t)(i + j * n)];
    }
    return 0;
  });
  for (int64_t i = 0; i < n; ++i) if (!solved[(size_t)i]) ++bad;
  int64_t miss = 0;
  if (mark)
    for (int64_t j = 0; j < n; ++j)
      for (int64_t i = 0; i < n; ++i) miss += cover[(size_t)(i + j * n)] != (i <= j ? 1 : 0);
  if (steps != sp::num_steps(n) || nleaves != sp::leaves(n)) ++bad;
  printf("steps=%lld leaves=%lld products=%lld max_leaf=%lld depth=%d elems=%lld total=%lld marked=%d miss=%lld bad=%lld\n", (long long)steps,
         (long long)nleaves, (long long)products, (long long)max_leaf, depth_of(n), (long long)elems, (long long)(n * (n + 1) / 2), (int)mark,
         (long long)miss, (long long)bad);
}

int main() {
  char line[256];
  while (fgets(line, sizeof(line), stdin)) {
    long long a, b;
    if (!strncmp(line, "leaf", 4)) printf("leaf=%d\n", sp::LEAF);
    else if (sscanf(line, "plan %lld %lld", &a, &b) == 2) plan((int)a, b);
    else { fprintf(stderr, "unknown command: %s", line); return 2; }
  }
  return 0;
}
