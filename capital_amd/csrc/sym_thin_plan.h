// sym_thin_plan.h -- how capi_dresid_sym (sym_apply_f64.hip) cuts Rout <- B - S X, S symmetric and stored as A's upper triangle, into workgroup
// blocks.  Pure arithmetic in the manner of tri_thin_plan.h: no HIP, compiled by a host compiler too (tests/sym_thin_plan), and by hipcc for both sides.
//
// The n lines are cut into p LINE BLOCKS of bs lines (bs a multiple of 32, the last block ragged), and the upper triangle into the p (p + 1) / 2
// BLOCKS (I, J), I <= J: rows of line block I x columns of line block J, for I == J the part on and above the diagonal.  One workgroup owns one
// block, reads it once and writes exactly two ranges of partial sums:
//   slot 2 id + 0, lines of I:  U_IJ X_J                          (for I == J: the upper triangle incl. the diagonal)
//   slot 2 id + 1, lines of J:  U_IJ^T X_I                        (for I == J: the STRICTLY upper triangle: the diagonal counts once)
// id = J (J + 1) / 2 + I.  A slot is [16 columns][bs lines].  Line block L receives p + 1 contributions, which the combine kernel adds in the order
// k = 0 .. p: the row slots of (L, L), (L, L + 1), .., (L, p - 1), then the column slots of (0, L), (1, L), .., (L, L).
//
// BALANCE RULE: p is the largest count with p (p + 1) / 2 <= the CUs (and bs >= 32), so every workgroup runs beside every other and the call
// lasts as long as its largest block: no block holds more than bs x bs elements, and bs < n / p + 32.  The p diagonal blocks hold half as much;
// pairing them would free p / 2 CUs, which admits no larger p at 256 CUs (22: 253 blocks; 23 would need 276 - 11), so they are left alone.
#pragma once
#include "thin_plan_common.h"

namespace sym_thin_plan {
using namespace thin_plan;

constexpr int STRIP = 32;         // lines per wave strip: bs is a multiple
constexpr int SUPER = 256;        // lines per super-tile edge (8 strips)
constexpr int RPAD = 16;          // columns per slot

struct Plan {
  int64_t n, bs;                  // order, lines per line block
  int p;                          // line blocks
};

// the largest q with q (q + 1) / 2 <= cus (at least 1)
THIN_HD inline int max_blocks_edge(int cus) {
  int q = 1;
  while ((q + 1) * (q + 2) / 2 <= cus) ++q;
  return q;
}
THIN_HD inline Plan make_plan(int64_t n, int cus) {
  Plan P;
  P.n = n;
  const int q = max_blocks_edge(cus);
  P.bs = n > 0 ? cdiv64(cdiv64(n, q), STRIP) * STRIP : STRIP;
  P.p = (int)cdiv64(n, P.bs);
  return P;
}
THIN_HD inline int num_blocks(const Plan& P) { return P.p * (P.p + 1) / 2; }
THIN_HD inline int block_id(int I, int J) { return J * (J + 1) / 2 + I; }
THIN_HD inline void block_of(int id, int* I, int* J) {
  int j = 0;
  while ((j + 1) * (j + 2) / 2 <= id) ++j;
  *J = j;
  *I = id - j * (j + 1) / 2;
}
// lines [l0, l1) of line block L
THIN_HD inline int64_t line0(const Plan& P, int L) { return (int64_t)L * P.bs; }
THIN_HD inline int64_t line1(const Plan& P, int L) { return min64(P.n, (int64_t)(L + 1) * P.bs); }
// the two slots a block writes: which = 0 the lines of I, which = 1 the lines of J
THIN_HD inline int slot_of(int I, int J, int which) { return 2 * block_id(I, J) + which; }
THIN_HD inline int64_t slot_doubles(const Plan& P) { return (int64_t)RPAD * P.bs; }
THIN_HD inline int64_t slab_doubles(const Plan& P) { return 2 * (int64_t)num_blocks(P) * slot_doubles(P); }
// contribution k = 0 .. p of line block L, in the order the combine adds them
THIN_HD inline int contribution(const Plan& P, int L, int k) {
  const int nrow = P.p - L;                                   // row slots of (L, L .. p - 1)
  return k < nrow ? slot_of(L, L + k, 0) : slot_of(k - nrow, L, 1);
}
// elements of A that block (I, J) reads
THIN_HD inline int64_t block_elems(const Plan& P, int I, int J) {
  const int64_t a = line1(P, I) - line0(P, I), b = line1(P, J) - line0(P, J);
  return I == J ? a * (a + 1) / 2 : a * b;
}
// the block that owns element (row, col), row <= col
THIN_HD inline int owner(const Plan& P, int64_t row, int64_t col) { return block_id((int)(row / P.bs), (int)(col / P.bs)); }

}  // namespace sym_thin_plan
