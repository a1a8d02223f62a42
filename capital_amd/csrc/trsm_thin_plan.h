// trsm_thin_plan.h -- the call sequence of capi_dtrsm_thin (tri_solve_f64.hip): B <- op(T)^-1 B for an upper triangular T of order n and a thin B,
// by substitution.  Pure arithmetic in the manner of tri_thin_plan.h: no HIP, compiled by a host compiler too (tests/trsm_thin_plan).
//
// The triangle is cut recursively into LEAVES (diagonal sub-triangles of order <= LEAF, each solved by one launch of the leaf kernel) and
// RECTANGULAR PRODUCTS (capi_dtrmm_thin on a CAPI_RECT view, alpha = -1, beta = 1).  A triangle of order n > LEAF at offset a splits into
// T11 (order n1), T12 (n1 x n2) and T22 (order n2):
//   TRANS    (T^T y = b, forward):   solve T11^T y1 = b1;  b2 -= T12^T y1;  solve T22^T y2 = b2
//   NOTRANS  (T x = y, backward):    solve T22 x2 = y2;    y1 -= T12 x2;    solve T11 x1 = y1
// SPLIT RULE: n1 = LEAF * ceil(ceil(n / LEAF) / 2) -- a multiple of LEAF, so every leaf but the last of the triangle has order LEAF, and the
// recursion is ceil(log2(ceil(n / LEAF))) deep: 2 ceil(n / LEAF) - 1 steps.  Every element of the triangle lies in exactly one leaf or
// one product, so T is read once per call.  The steps run in the order listed, one after the other on one stream: a product reads rows of B
// that earlier steps finished and updates rows that no earlier leaf has solved.
#pragma once
#include <stdint.h>

namespace trsm_thin_plan {

// order of the largest leaf.  Measured at n = 32768 against 256 (profiles/cholinv_solve_subst.txt): 256 is 8-14 % faster at r = 1, 512 up to 9 %
// faster at r = 8 and 15-17 % at r = 32.  1024 is not buildable: the leaf kernel keeps the solved rows of a leaf in LDS, (LEAF - 32) x 32
// doubles at r > 16
// (-DCAPI_TRSM_THIN_LEAF=256 builds the other candidate, for an A/B measurement through CAPITAL_HIP_LIB)
#ifndef CAPI_TRSM_THIN_LEAF
#define CAPI_TRSM_THIN_LEAF 512
#endif
constexpr int LEAF = CAPI_TRSM_THIN_LEAF;
static_assert(LEAF == 256 || LEAF == 512, "LEAF: a multiple of 32 whose solved rows fit LDS");

enum { STEP_LEAF = 0, STEP_PRODUCT = 1 };
// a leaf: the triangle's rows and columns [row0, row0 + n) (row0 == col0, m == n).  A product: the block T(row0 .. row0 + m - 1, col0 .. col0 + n - 1),
// strictly above the diagonal.  TRANS: B(col0 .. + n) -= block^T B(row0 .. + m).  NOTRANS: B(row0 .. + m) -= block B(col0 .. + n)
struct Step { int kind; int64_t row0, col0, m, n; };

inline int64_t leaves(int64_t n) { return (n + LEAF - 1) / LEAF; }
inline int64_t num_steps(int64_t n) { return n > 0 ? 2 * leaves(n) - 1 : 0; }
inline int64_t split(int64_t n) { return LEAF * ((leaves(n) + 1) / 2); }

// calls f(Step) for every step of the triangle of order n at offset a, in execution order; stops at, and returns, the first non-zero value of f
template <class F>
inline int for_each_step(int trans, int64_t a, int64_t n, F&& f) {
  if (n <= 0) return 0;
  if (n <= LEAF) return f(Step{STEP_LEAF, a, a, n, n});
  const int64_t n1 = split(n), n2 = n - n1;
  int rc;
  if (trans) {
    if ((rc = for_each_step(trans, a, n1, f))) return rc;
    if ((rc = f(Step{STEP_PRODUCT, a, a + n1, n1, n2}))) return rc;
    return for_each_step(trans, a + n1, n2, f);
  }
  if ((rc = for_each_step(trans, a + n1, n2, f))) return rc;
  if ((rc = f(Step{STEP_PRODUCT, a, a + n1, n1, n2}))) return rc;
  return for_each_step(trans, a, n1, f);
}

}  // namespace trsm_thin_plan
