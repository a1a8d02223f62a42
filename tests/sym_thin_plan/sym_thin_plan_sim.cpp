// sym_thin_plan_sim.cpp -- walks the block triangle of capi_dresid_sym (capital_amd/csrc/sym_thin_plan.h) on the host.
// stdin: lines "plan <n> <cus>"; stdout: one line of key=value counts per plan (tests/test_sym_thin_plan.py reads them).
#include <cstdio>
#include <cstring>
#include <vector>
#include "sym_thin_plan.h"

namespace sp = sym_thin_plan;

int main() {
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    long long n_ = 0;
    int cus = 0;
    if (sscanf(line, "plan %lld %d", &n_, &cus) != 2) continue;
    const int64_t n = n_;
    const sp::Plan P = sp::make_plan(n, cus);
    const int nb = sp::num_blocks(P);
    int64_t bad = 0, elems = 0, max_block = 0, miss = 0;
    // the line blocks tile [0, n) in order
    int64_t at = 0;
    for (int L = 0; L < P.p; ++L) {
      if (sp::line0(P, L) != at || sp::line1(P, L) <= at) ++bad;
      at = sp::line1(P, L);
    }
    if (at != n) ++bad;
    // blocks: numbering, sizes
    for (int J = 0; J < P.p; ++J)
      for (int I = 0; I <= J; ++I) {
        int i2, j2;
        sp::block_of(sp::block_id(I, J), &i2, &j2);
        if (i2 != I || j2 != J || sp::block_id(I, J) < 0 || sp::block_id(I, J) >= nb) ++bad;
        const int64_t e = sp::block_elems(P, I, J);
        elems += e;
        if (e > max_block) max_block = e;
      }
    // element by element where the matrix is small: every element of the upper triangle lies in the ranges of the block that owns it, and the
    // blocks hold what block_elems says
    const bool marked = n * n <= 4000000;
    if (marked) {
      std::vector<int64_t> cnt((size_t)nb, 0);
      for (int64_t c = 0; c < n; ++c)
        for (int64_t r = 0; r <= c; ++r) {
          const int id = sp::owner(P, r, c);
          int I, J;
          if (id < 0 || id >= nb) { ++miss; continue; }
          sp::block_of(id, &I, &J);
          if (r < sp::line0(P, I) || r >= sp::line1(P, I) || c < sp::line0(P, J) || c >= sp::line1(P, J)) ++miss;
          ++cnt[(size_t)id];
        }
      for (int J = 0; J < P.p; ++J)
        for (int I = 0; I <= J; ++I)
          if (cnt[(size_t)sp::block_id(I, J)] != sp::block_elems(P, I, J)) ++miss;
    }
    // slots: what the blocks write (slot -> the line block it holds), what the combine reads
    std::vector<int> holds((size_t)(2 * nb), -1), reads((size_t)(2 * nb), 0);
    int64_t written = 0, read = 0, stray = 0;
    for (int J = 0; J < P.p; ++J)
      for (int I = 0; I <= J; ++I)
        for (int which = 0; which < 2; ++which) {
          const int s = sp::slot_of(I, J, which);
          if (s < 0 || s >= 2 * nb || holds[(size_t)s] != -1) { ++bad; continue; }
          holds[(size_t)s] = which ? J : I;
          ++written;
        }
    for (int L = 0; L < P.p; ++L)
      for (int k = 0; k <= P.p; ++k) {
        const int s = sp::contribution(P, L, k);
        ++read;
        if (s < 0 || s >= 2 * nb || holds[(size_t)s] != L) { ++stray; continue; }     // a slot that nothing wrote, or another line block's
        ++reads[(size_t)s];
      }
    int64_t unread = 0;
    for (int s = 0; s < 2 * nb; ++s)
      if (holds[(size_t)s] != -1 && reads[(size_t)s] != 1) ++unread;
    if (sp::slab_doubles(P) != 2 * (int64_t)nb * sp::RPAD * P.bs) ++bad;
    printf("p=%d bs=%lld blocks=%d q=%d elems=%lld max_block=%lld marked=%d miss=%lld written=%lld read=%lld stray=%lld unread=%lld bad=%lld\n", P.p,
           (long long)P.bs, nb, sp::max_blocks_edge(cus), (long long)elems, (long long)max_block, (int)marked, (long long)miss, (long long)written,
           (long long)read, (long long)stray, (long long)unread, (long long)bad);
  }
  return 0;
}
