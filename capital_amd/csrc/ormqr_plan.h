// ormqr_plan.h -- the launch schedule of capi_dormqr's thin path (qr_apply_f64.hip): C (m x r, r <= 32) <- Q^T C or Q C with Q = H_1 .. H_k from a
// capi_dgeqrf image.  Pure arithmetic in the manner of chud_plan.h: no HIP, compiled by a host compiler too (tests/ormqr_plan).
//
// The k reflectors are cut into PANELS of NB = 32 (larft_kernel's width), applied in ascending order for Q^T and in descending order for Q.  The
// panel at j0 works on the rows j0 .. m - 1 ("live rows").  Its Gram pass cuts them into TILES of 32 rows, a ROUND is one tile for each of the 8
// waves of a workgroup, and workgroup z of S takes the consecutive rounds [round_begin(z), round_begin(z + 1)): a row slice.  S <= the CUs and
// S <= the rounds, so no slice is empty.  Workgroup z writes slab z; the slabs are added in the order z = 0, 1, ..
#pragma once
#include "thin_plan_common.h"

namespace ormqr_plan {

constexpr int NB = 32;              // reflectors per panel
constexpr int TILE = 32;            // rows of a wave's tile
constexpr int WAVES = 8;            // waves of a Gram workgroup
constexpr int ROUND = TILE * WAVES; // rows of a round

struct Panel { int64_t j0; int nb; int64_t rows; };   // reflectors [j0, j0 + nb), live rows j0 .. m - 1

THIN_HD inline int64_t num_panels(int64_t k) { return k > 0 ? thin_plan::cdiv64(k, NB) : 0; }
// the step-th panel in the order of application: trans (Q^T = H_k .. H_1 applied H_1 first) ascending, else descending
THIN_HD inline Panel panel(int64_t m, int64_t k, bool trans, int64_t step) {
  const int64_t p = trans ? step : num_panels(k) - 1 - step, j0 = p * NB;
  return Panel{j0, (int)thin_plan::min64(NB, k - j0), m - j0};
}

struct Slices { int64_t tiles, rounds; int S; };
THIN_HD inline Slices slices(int64_t rows, int cus) {
  const int64_t tiles = thin_plan::cdiv64(rows, TILE), rounds = thin_plan::cdiv64(tiles, WAVES);
  return Slices{tiles, rounds, (int)thin_plan::min64(rounds, cus > 0 ? cus : 1)};
}
// first round of slice z (z == S: the end).  Slices differ by at most one round
THIN_HD inline int64_t round_begin(const Slices& s, int64_t z) { return z * s.rounds / s.S; }
// live rows [r0, r1) of slice z, relative to the panel's first row
THIN_HD inline int64_t row_begin(const Slices& s, int64_t rows, int64_t z) { return thin_plan::min64(round_begin(s, z) * ROUND, rows); }

// a slab: the upper 16 x 16 blocks (0,0), (0,1), (1,1) of G = P^T P, then W = P^T C as rb planes of 32 x 16 -- every block [16 rows][16 columns]
THIN_HD inline int slab_doubles(int rb) { return 3 * 256 + 2 * rb * 256; }
// the workspace of a call, in doubles: Z (32 x 32, ld 32), then the slabs of the panel with the most live rows (the one at j0 = 0)
constexpr int64_t Z_DOUBLES = NB * NB;
THIN_HD inline int64_t slab_offset(int rb, int64_t z) { return Z_DOUBLES + z * slab_doubles(rb); }
THIN_HD inline int64_t workspace_doubles(int64_t m, int rb, int cus) { return slab_offset(rb, slices(m, cus).S); }
THIN_HD inline int64_t num_launches(int64_t k) { return 3 * num_panels(k); }

}  // namespace ormqr_plan
