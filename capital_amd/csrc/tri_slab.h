// tri_slab.h -- what stands around tri_thin_plan.h in every call that streams a triangle or rectangle by that plan (capi_dtrmm_thin of
// tri_apply_f64.hip, capi_dtri_rownorm2 of tri_reduce_f64.hip): the host prologue, the slabs of partial sums and the launch that adds them.
//
// A workgroup walks its slice's consecutive tiles and leaves, for every group of 256 output lines that it touches, [width][256] doubles in a slab of
// its own; a second launch (tri_combine_kernel) adds the slabs of a group in slice order: no floating-point atomics, the same bits on every run.
// SLOT RULE: slice s keeps its sums for group g in slot s + g.  The slices' tile ranges are consecutive and the tiles are numbered group by group, so
// from one (slice, group) pair to the next either s or g grows and neither shrinks: no two pairs share a slot, and S + ngroups slots hold them all.
#pragma once
#include "capi_internal.h"
#include "tri_thin_plan.h"

namespace tri_slab {
namespace tp = tri_thin_plan;

THIN_HD inline int64_t slot(int64_t s, int64_t g) { return s + g; }
// first double of the slab of slice s for group g
THIN_HD inline int64_t slab_offset(int64_t s, int64_t g, int width) { return slot(s, g) * (tp::GROUP * width); }

// Local to the including file (the anonymous namespace), the kernel a template, as thin_tile.h's colnorms_kernel: every file holds its own copy
namespace {

struct CombineArgs {
  const double* slab; double* C;
  int64_t ldc;
  double alpha, beta;
  int r, width, S;
  tp::Plan P;
  int64_t pos[tp::MAX_SLICES + 1];
};

// C(l, j) = alpha (the slabs of l's group, in slice order) + beta C(l, j) for j < r; beta == 0 does not read C
template <class = void>
__global__ __launch_bounds__(tp::GROUP) void tri_combine_kernel(const CombineArgs p) {
  const int64_t g = blockIdx.x, l = g * tp::GROUP + threadIdx.x;
  if (l >= p.P.lines) return;
  int sa = 0, sb = -1;
  if (p.S > 0) {
    const int64_t t0 = tp::tiles_before(p.P, g), t1 = tp::tiles_before(p.P, g + 1);
    while (p.pos[sa + 1] <= t0) ++sa;                                    // the slice that holds the group's first tile
    sb = sa;
    while (sb + 1 < p.S && p.pos[sb + 1] < t1) ++sb;                     // .. and its last
  }
  for (int j = 0; j < p.r; ++j) {
    double sum = 0.0;
    for (int s = sa; s <= sb; ++s)
      if (p.pos[s] < p.pos[s + 1]) sum += p.slab[(slot(s, g) * p.width + j) * tp::GROUP + threadIdx.x];
    double v = p.alpha * sum;
    if (p.beta != 0.0) v += p.beta * p.C[l + (int64_t)j * p.ldc];
    p.C[l + (int64_t)j * p.ldc] = v;
  }
}

// The prologue: plan, slices, and the slabs in the handle's workspace, into both argument structs.  cp->S == 0: nothing to stream, the combine still runs
template <class StreamArgs>
inline int plan_slabs(capi_handle_t h, int shape, int trans, int64_t m, int64_t n, int width, CombineArgs* cp, StreamArgs* p) {
  cp->P = tp::make_plan(shape == CAPI_UPPERTRI ? tp::UPPERTRI : tp::RECT, trans, m, n);
  cp->S = tp::make_slices(cp->P, capi_stream_cus(h), cp->pos);
  cp->slab = nullptr; cp->width = width;
  if (cp->S == 0) return CAPI_OK;
  void* pv = nullptr;
  const int rc = capi_ws_get(h, sizeof(double) * (size_t)slab_offset(cp->S, cp->P.ngroups, width), &pv);
  if (rc != CAPI_OK) return rc;
  cp->slab = p->slab = (double*)pv;
  p->S = cp->S; p->P = cp->P;
  memcpy(p->pos, cp->pos, sizeof(int64_t) * (size_t)(cp->S + 1));
  return CAPI_OK;
}

inline void combine(capi_handle_t h, CombineArgs& cp, int r, double alpha, double beta, double* C, int64_t ldc) {
  cp.C = C; cp.ldc = ldc; cp.alpha = alpha; cp.beta = beta; cp.r = r;
  hipLaunchKernelGGL(tri_combine_kernel<>, dim3((unsigned)cp.P.ngroups), dim3(tp::GROUP), 0, h->stream, cp);
}

}  // namespace
}  // namespace tri_slab
