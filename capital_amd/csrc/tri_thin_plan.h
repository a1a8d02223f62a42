// tri_thin_plan.h -- how capi_dtrmm_thin (tri_apply_f64.hip) cuts C <- alpha op(T) B + beta C into workgroup slices, and tri_view, the way every
// kernel on the cholinv factors addresses its triangle.  Pure arithmetic in the manner of gemm_plan.h: no HIP, compiled by a host compiler too
// (tests/tri_thin_plan), and by hipcc for both sides.  What a call does around the plan (workspace, slabs, the combine launch) is in tri_slab.h.
//
// The m x n block T (all of it, or the upper triangle incl. the diagonal) is cut into TILES.  A tile belongs to a GROUP of 256 output lines
// (rows of T for NOTRANS, columns for TRANS: one workgroup of 8 waves x 32 lines) and is 32 deep along the contraction index (columns for
// NOTRANS, rows for TRANS): 256 x 32 elements, 64 KiB, fewer at the block's edges and on the diagonal.  Tiles that hold no element of
// the triangle are not enumerated.  The tiles are numbered group by group, inside a group along the contraction index, and slice s takes the
// consecutive tiles [pos[s], pos[s + 1]).
//
// BALANCE RULE (by bytes, not by tile or column counts): pos[s] is the first tile at whose END the running element count reaches
// s / S of the block's elements, so no slice holds more than the mean share plus ONE TILE's worth (256 x 32 elements); a slice may be
// empty when a single tile outweighs the mean share.
#pragma once
#include "thin_plan_common.h"

namespace tri_thin_plan {
using namespace thin_plan;

constexpr int GROUP = 256;        // output lines per group
constexpr int DEPTH = 32;         // contraction indices per tile
constexpr int CPG = GROUP / DEPTH;
constexpr int MAX_SLICES = 256;
enum { RECT = 0, UPPERTRI = 1 };

struct Plan {
  int tri, trans;
  int64_t m, n;
  int64_t lines, depth;           // output lines, contraction length
  int64_t ngroups, kc;            // groups of lines; tiles along the whole contraction length
};

// first element of column x of a packed upper triangle (structure.h uppertri).  The even factor is halved first: exact up to x ~ 4e9
THIN_HD inline int64_t packed_col_start(int64_t x) { return (x & 1) ? x * ((x + 1) / 2) : (x / 2) * (x + 1); }
// block column j of a view whose first column is the triangle's column col0, relative to the view's first element
THIN_HD inline int64_t packed_col_offset(int64_t col0, int64_t j) { return packed_col_start(col0 + j) - packed_col_start(col0); }
// alignment class of a column that starts `start` doubles behind a 16-byte boundary: 0 = 16-byte aligned, 1 = 8-byte aligned only
THIN_HD inline int align_class(int64_t start) { return (int)(start & 1); }

// THE VIEW that the kernels on the cholinv factors take (capi_dtrmm_thin, capi_dtri_*, capi_dtrsm_thin, capi_dchud*): a block whose first element is T,
// column-major with the leading dimension ldt > 0, or, ldt == 0, a view into a packed upper triangle whose first column is the triangle's column col0
// (not read when ldt > 0).  Checked by CAPI_REQUIRE_TRI_VIEW (capi_internal.h); cholinv.h's image::at is the host's twin of sub()
template <class D>
struct tri_view_t {
  D* T;
  int64_t ldt, col0;
  THIN_HD bool packed() const { return ldt == 0; }
  THIN_HD D* col(int64_t j) const { return ldt > 0 ? T + j * ldt : T + packed_col_offset(col0, j); }     // first element of column j
  THIN_HD D* at(int64_t i, int64_t j) const { return col(j) + i; }
  THIN_HD tri_view_t sub(int64_t i0, int64_t j0) const { return tri_view_t{at(i0, j0), ldt, ldt > 0 ? 0 : col0 + j0}; }   // first element (i0, j0)
};
using tri_view = tri_view_t<const double>;
using tri_view_rw = tri_view_t<double>;         // chud_f64.hip rewrites the triangle in place

THIN_HD inline Plan make_plan(int shape, int trans, int64_t m, int64_t n) {
  Plan P;
  P.tri = shape == UPPERTRI; P.trans = trans != 0; P.m = m; P.n = n;
  P.lines = trans ? n : m; P.depth = trans ? m : n;
  P.ngroups = cdiv64(P.lines, GROUP); P.kc = cdiv64(P.depth, DEPTH);
  return P;
}
// contraction index (in tiles) of the first tile of group g: the triangle's rows 256 g.. start at column 256 g
THIN_HD inline int64_t first_tile(const Plan& P, int64_t g) { return (P.tri && !P.trans) ? CPG * g : 0; }
THIN_HD inline int64_t group_tiles(const Plan& P, int64_t g) {
  if (!P.tri) return P.kc;
  return P.trans ? min64(P.kc, CPG * (g + 1)) : P.kc - CPG * g;
}
// tiles of the groups before g (0 <= g <= ngroups)
THIN_HD inline int64_t tiles_before(const Plan& P, int64_t g) {
  if (!P.tri) return g * P.kc;
  if (!P.trans) return g * P.kc - (CPG / 2) * g * (g - 1);
  return g < P.ngroups ? (CPG / 2) * g * (g + 1) : (P.ngroups > 0 ? (CPG / 2) * (P.ngroups - 1) * P.ngroups + P.kc : 0);
}
THIN_HD inline int64_t total_tiles(const Plan& P) { return (P.lines > 0 && P.depth > 0) ? tiles_before(P, P.ngroups) : 0; }
// tile number pos -> (group, contraction index in tiles)
THIN_HD inline void locate(const Plan& P, int64_t pos, int64_t* g, int64_t* c) {
  int64_t lo = 0, hi = P.ngroups - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) / 2;
    if (tiles_before(P, mid) <= pos) lo = mid; else hi = mid - 1;
  }
  *g = lo;
  *c = first_tile(P, lo) + (pos - tiles_before(P, lo));
}
// the tile's rows [r0, r1) and columns [c0, c1) of the block
THIN_HD inline void tile_rect(const Plan& P, int64_t g, int64_t c, int64_t* r0, int64_t* r1, int64_t* c0, int64_t* c1) {
  if (!P.trans) { *r0 = GROUP * g; *r1 = min64(P.m, *r0 + GROUP); *c0 = DEPTH * c; *c1 = min64(P.n, *c0 + DEPTH); }
  else { *c0 = GROUP * g; *c1 = min64(P.n, *c0 + GROUP); *r0 = DEPTH * c; *r1 = min64(P.m, *r0 + DEPTH); }
}
// elements of the block inside the tile
THIN_HD inline int64_t tile_elems(const Plan& P, int64_t g, int64_t c) {
  int64_t r0, r1, c0, c1;
  tile_rect(P, g, c, &r0, &r1, &c0, &c1);
  if (!P.tri || r1 - 1 <= c0) return (r1 - r0) * (c1 - c0);
  int64_t e = 0;
  for (int64_t j = c0; j < c1; ++j) e += max64(0, min64(j + 1, r1) - r0);
  return e;
}
// how many consecutive tiles of group g, from c on, are known to weigh the same as tile c (>= 1): the interior of a group
THIN_HD inline int64_t run_length(const Plan& P, int64_t g, int64_t c) {
  const int64_t last = first_tile(P, g) + group_tiles(P, g) - 1;        // may be ragged along the contraction index
  int64_t end = last;                                                  // first tile that may weigh differently
  if (P.tri && !P.trans && c < CPG * (g + 1)) return 1;                // tiles that the diagonal crosses
  if (P.tri && P.trans) end = min64(last, CPG * g);
  return end > c ? end - c : 1;
}
inline int64_t total_elems(const Plan& P) { return P.tri ? P.n * (P.n + 1) / 2 : P.m * P.n; }

// pos[0..S]: the slices' tile ranges (see the balance rule above).  Returns S = min(max_slices, MAX_SLICES, tiles)
inline int make_slices(const Plan& P, int max_slices, int64_t* pos) {
  const int64_t T = total_tiles(P), E = total_elems(P);
  int S = (int)min64(min64(max_slices, MAX_SLICES), T);
  if (S < 1) { pos[0] = 0; return 0; }
  pos[0] = 0;
  int s = 1;
  int64_t cum = 0, p = 0;
  for (int64_t g = 0; g < P.ngroups && s < S; ++g) {
    const int64_t c_end = first_tile(P, g) + group_tiles(P, g);
    for (int64_t c = first_tile(P, g); c < c_end && s < S;) {
      const int64_t w = tile_elems(P, g, c), q = run_length(P, g, c);
      // cut s falls behind the k-th tile of this run when cum + k w >= E s / S first holds
      while (s < S && (__int128)(cum + q * w) * S >= (__int128)E * s) {
        const __int128 need = (__int128)E * s - (__int128)cum * S;
        const int64_t k = need <= 0 ? 0 : (int64_t)((need + (__int128)w * S - 1) / ((__int128)w * S));
        pos[s++] = p + k;
      }
      cum += q * w; p += q; c += q;
    }
  }
  while (s < S) pos[s++] = T;
  pos[S] = T;
  return S;
}

}  // namespace tri_thin_plan
