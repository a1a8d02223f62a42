// jacobi_plan.h -- the pair schedule of capi_dgesvj (svd_f64.hip): which two columns a workgroup rotates.  Pure arithmetic in the manner of
// trsm_thin_plan.h: no HIP, usable from host and device, compiled by a host compiler too (tests/jacobi_plan).
//
// A cyclic sweep of one-sided Jacobi visits every unordered pair of the n columns once.  The ROUND-ROBIN (circle-method) order does it in
// N - 1 STEPS, N = n rounded up to even, of up to N / 2 disjoint pairs each, so that a step's pairs can be rotated side by side: one launch per
// step, one workgroup per SLOT.  The N players sit on a circle of N - 1 seats with player N - 1 in the middle:
//   slot 0      pairs the middle player N - 1 with player `step`
//   slot k > 0  pairs the players (step + k) mod (N - 1) and (step - k) mod (N - 1),  k = 1 .. N / 2 - 1
// For an odd n the middle player is a phantom: slot 0 SITS OUT, and column `step` rests in that step.  n == 1 has no steps.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JACOBI_PLAN_HD __host__ __device__
#else
#define JACOBI_PLAN_HD
#endif

namespace jacobi_plan {

constexpr int MAX_N = 2048;                      // capi_dgesvj's largest order
constexpr int MAX_SWEEPS = 30;

JACOBI_PLAN_HD inline int players(int n) { return n + (n & 1); }
JACOBI_PLAN_HD inline int steps(int n) { return n > 1 ? players(n) - 1 : 0; }
JACOBI_PLAN_HD inline int slots(int n) { return n > 1 ? players(n) / 2 : 0; }

// the pair p < q < n of (step, slot), 0 <= step < steps(n), 0 <= slot < slots(n); false: the slot sits out (p and q are not written)
JACOBI_PLAN_HD inline bool pair_of(int n, int step, int slot, int* p, int* q) {
  const int N = players(n), ring = N - 1;
  int a, b;
  if (slot == 0) {
    a = N - 1;
    b = step;
  } else {
    a = step + slot;
    if (a >= ring) a -= ring;
    b = step - slot;
    if (b < 0) b += ring;
  }
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  if (hi >= n) return false;
  *p = lo;
  *q = hi;
  return true;
}

}  // namespace jacobi_plan
