// chud_plan.h -- the launch schedule of capi_dchud / capi_dchud_inv (chud_f64.hip): the rank-r update or downdate of an upper triangular factor T of
// order n, T'^T T' = T^T T + sign V V^T, and of its inverse.  Pure arithmetic in the manner of trsm_thin_plan.h: no HIP, compiled by a host compiler
// too (tests/chud_plan).
//
// The n steps (one per row of T) are cut into PANELS of B consecutive rows.  Per panel two launches follow each other on one stream:
//   the DIAGONAL kernel, one workgroup: the panel's B dependent steps on the B x B diagonal block and the panel's rows of V; it writes the log;
//   the APPLY kernel, one workgroup per COLS trailing columns j >= the panel's end: a thread owns one column, walks the panel's steps from the log.
// Every step lies in exactly one panel, and every column behind a panel in exactly one apply workgroup of that panel: 2 ceil(n / B) - 1 launches.
// The inverse needs no chain: one launch, a thread owns one ROW c of the inverse's sub-triangle [k0, k1) and walks the steps k = c .. k1 - 1.
#pragma once
#include "thin_plan_common.h"

namespace chud_plan {

// rows of a panel.  (-DCAPI_CHUD_PANEL=64 builds the other candidate, for an A/B measurement through CAPITAL_HIP_LIB)
#ifndef CAPI_CHUD_PANEL
#define CAPI_CHUD_PANEL 32
#endif
constexpr int B = CAPI_CHUD_PANEL;
static_assert(B == 32 || B == 64, "B: the diagonal kernel is one wave, a lane per column of the diagonal block");
constexpr int COLS = 4096 / B;  // trailing columns (threads) of an apply workgroup: its B x COLS tile of T is 32 KiB of LDS
constexpr int ROWS = 64;        // rows of the inverse (threads) of a workgroup of capi_dchud_inv
constexpr int KCHUNK = 16;      // steps whose log a workgroup of capi_dchud_inv stages at a time

// one record of the log per step: x_k (r doubles), alpha_k, beta_k
inline int64_t log_stride(int64_t r) { return r + 2; }
inline int64_t log_doubles(int64_t n, int64_t r) { return n * log_stride(r); }

struct Panel { int64_t k0, k1; };            // the steps [k0, k1)
struct Apply { int64_t j0, j1; };            // the trailing columns [j0, j1) of one apply workgroup

inline int64_t num_panels(int64_t n) { return n > 0 ? (n + B - 1) / B : 0; }
inline Panel panel(int64_t n, int64_t p) { return Panel{p * B, (p + 1) * B < n ? (p + 1) * B : n}; }
inline int64_t panel_of(int64_t k) { return k / B; }
// apply workgroups behind the panel (0: the panel reaches the last column)
inline int64_t num_applies(int64_t n, const Panel& P) { return (n - P.k1 + COLS - 1) / COLS; }
inline Apply apply(int64_t n, const Panel& P, int64_t g) { return Apply{P.k1 + g * COLS, P.k1 + (g + 1) * COLS < n ? P.k1 + (g + 1) * COLS : n}; }
inline int64_t num_launches(int64_t n) { return n > 0 ? 2 * num_panels(n) - 1 : 0; }      // (the last panel has no column behind it)

// capi_dchud_inv on the steps [k0, k1): workgroup g owns the rows [k0 + g ROWS, ..) and walks the chunks of KCHUNK steps from the one that holds its
// first row (chunks are aligned to k0)
inline int64_t inv_groups(int64_t k0, int64_t k1) { return k1 > k0 ? (k1 - k0 + ROWS - 1) / ROWS : 0; }
THIN_HD inline int64_t inv_first_step(int64_t k0, int64_t g) { return k0 + g * ROWS / KCHUNK * KCHUNK; }
static_assert(ROWS % KCHUNK == 0, "a workgroup's first row starts a chunk");

}  // namespace chud_plan
