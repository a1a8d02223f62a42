// tri_solve_f64.hip -- B <- op(T)^-1 B for an upper triangular T (column-major, or a view into a packed triangle) and a THIN B (r <= 32 columns),
// by SUBSTITUTION: solves on the cholinv factor R itself (cholesky::cholinv::solve with info::solve_by_substitution).  Not in the reference: its
// cholinv stops at R and R^-1.
//
//   capi_dtrsm_thin   B <- op(T)^-1 B      no inverse of T or of a block of it is formed; reciprocals of diagonal ENTRIES only
//
// The call runs the step list of trsm_thin_plan.h on the handle's stream: leaves (diagonal sub-triangles of order <= LEAF, the kernel below, one
// workgroup each) and rectangular products (capi_dtrmm_thin, alpha = -1, beta = 1, between disjoint rows of B), each on a sub-view of T
// (tri_thin_plan.h: tri_view::sub).  Every element of T belongs to one
// step, so T is read from HBM once.  Ordering is by kernel boundaries alone: no flag is waited on, no cooperative launch, no atomics, and every sum
// has a fixed order -- the same bits on every run.
//
// THE LEAF KERNEL marches over the leaf's 32-row blocks, first to last for TRANS (T^T is lower triangular), last to first for NOTRANS.  Wave 0 is
// the SOLVER, the other waves are TILE waves.  In slot s the solver substitutes the 32 x 32 diagonal block of block s from LDS while the tile waves
// multiply, for block s + 1, the 32 x 32 blocks beside its diagonal block by the rows solved before slot s (thin_tile.h: column dots for TRANS, row
// dots for NOTRANS; the solved rows are the stationary operand in LDS, r padded to 16 or 32).  Only the block next to the diagonal one waits for
// slot s's result: it is multiplied at the start of slot s + 1, from registers loaded a slot ahead.  T's pieces are staged one tile ahead in
// registers along a wave's whole sequence of tiles, and the next diagonal block is fetched while the current one is substituted.
// The chain: one step per row -- the row's value times the reciprocal of its diagonal entry (taken when the block is staged, off the chain), one
// cross-lane broadcast, one multiply-add per remaining row of the lane.  The rows are dealt to the lanes as well as the columns: a lane owns one
// column and every G-th row, G = 64 / CW for CW = 4, 16 or 32 column lanes (r <= 4, <= 16, <= 32), so that a step at small r costs 2 multiply-adds.
// Edges: the diagonal blocks and the ragged last block are loaded from clamped addresses and selected afterwards; nothing below the diagonal or
// outside the leaf takes part, whatever it holds.  Packed columns are 8-byte aligned only every other pair: the tiles load 16 bytes through d2u_t.
#include "capi_internal.h"
#include "thin_tile.h"
#include "tri_thin_plan.h"
#include "trsm_thin_plan.h"

namespace {

namespace tp = tri_thin_plan;
namespace sp = trsm_thin_plan;
namespace tt = thin_tile;
using tt::d2_t;
using tt::d2u_t;
using tt::d4_t;

constexpr int TS_BS = 32;                        // rows per block
constexpr int TS_DP = TS_BS + 1;                 // pitch of the diagonal block in LDS
constexpr int TS_XR = sp::LEAF - TS_BS;          // solved rows that a later block of the leaf still multiplies
constexpr int TS_NT = 3;                         // tile waves beside the solver
// doubles of LDS: the solved rows [RB][TS_XR][16], the tile waves' partial sums [NT][16 RB][32], the diagonal block and its reciprocals
constexpr size_t ts_lds_doubles(int RB) { return (size_t)RB * TS_XR * 16 + (size_t)TS_NT * 16 * RB * TS_BS + TS_BS * TS_DP + TS_BS; }

struct SolveArgs {
  tp::tri_view T;
  double* B;
  int64_t ldb;
  int n, r;
};

template <int RB, int CW, bool TR>
__global__ __launch_bounds__(64 * (TS_NT + 1)) void trsm_thin_leaf_kernel(const SolveArgs p) {
  constexpr int NT = TS_NT, RPAD = 16 * RB, PLANE = TS_XR * 16;
  constexpr int G = 64 / CW, RPL = TS_BS / G;      // row groups of the solver's lanes; rows per lane
  extern __shared__ __attribute__((aligned(16))) double Ls[];
  double* const X = Ls;                            // [RB][TS_XR][16]
  double* const P = X + RB * PLANE;                // [NT][RPAD][32]
  double* const D = P + NT * RPAD * TS_BS;         // [32 columns][TS_DP]: the diagonal block, zero below the diagonal, identity beyond the leaf
  double* const Dinv = D + TS_BS * TS_DP;          // [32]
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = p.n, nb = (n + TS_BS - 1) / TS_BS;
  auto blk = [&](int s) { return TR ? s : nb - 1 - s; };                  // the block solved in slot s
  auto xrow = [&](int b) { return TR ? TS_BS * b : TS_BS * (b - 1); };    // its first row in X (the block solved last is never stored)

  if (w == 0) {
    // ---------------- the solver: lane = (column c, row group g), rows g + G t of the block ----------------
    const int c = lane % CW, g = lane / CW;
    const bool cin = c < p.r;
    double* const Bc = p.B + (int64_t)(cin ? c : 0) * p.ldb;
    double bv[RPL];
    auto bload = [&](int b) {
#pragma unroll
      for (int t = 0; t < RPL; ++t) {
        const int row = TS_BS * b + g + G * t;
        const bool in = cin && row < n;
        const double v = *(in ? Bc + row : p.B);
        bv[t] = in ? v : 0.0;
      }
    };
    bload(blk(0));
    for (int s = 0; s < nb; ++s) {
      const int b = blk(s);
      __syncthreads();                             // #1: X of slot s - 1 is written
      __syncthreads();                             // #2: P, D and Dinv of block b are written
      double v[RPL], res[RPL];
#pragma unroll
      for (int t = 0; t < RPL; ++t) {
        double sum = 0.0;
#pragma unroll
        for (int u = 0; u < NT; ++u) sum += P[(u * RPAD + c) * TS_BS + g + G * t];
        v[t] = bv[t] - sum;
        res[t] = 0.0;
      }
      if (s + 1 < nb) bload(blk(s + 1));           // (rows that no step of this launch has written)
      if (TR) {
#pragma unroll
        for (int j = 0; j < TS_BS; ++j) {
          const int tj = j / G;
          const double y = __shfl(v[tj] * Dinv[j], (j % G) * CW + c);
          if (g == j % G) res[tj] = y;
#pragma unroll
          for (int t = tj; t < RPL; ++t) {
            const int i = g + G * t;
            const double l = D[i * TS_DP + j];     // T(j, i)
            v[t] -= (i > j ? l : 0.0) * y;
          }
        }
      } else {
#pragma unroll
        for (int j = TS_BS - 1; j >= 0; --j) {
          const int tj = j / G;
          const double y = __shfl(v[tj] * Dinv[j], (j % G) * CW + c);
          if (g == j % G) res[tj] = y;
#pragma unroll
          for (int t = 0; t <= tj; ++t) {
            const int i = g + G * t;
            const double u = D[j * TS_DP + i];     // T(i, j)
            v[t] -= (i < j ? u : 0.0) * y;
          }
        }
      }
      const bool keep = s + 1 < nb;
#pragma unroll
      for (int t = 0; t < RPL; ++t) {
        const int i = g + G * t, row = TS_BS * b + i;
        if (keep) X[(c >> 4) * PLANE + (xrow(b) + i) * 16 + (c & 15)] = res[t];
        if (cin && row < n) Bc[row] = res[t];
      }
    }
    return;
  }

  // ---------------- the tile waves ----------------
  const int tw = w - 1, l16 = lane & 15, g4 = lane >> 4, u0 = tid - 64;
  constexpr int NDQ = (TS_BS * TS_BS + 64 * NT - 1) / (64 * NT);
  double dreg[NDQ];
  // the diagonal block b, selected after the load: the upper triangle inside the leaf, the identity beyond it
  auto dload = [&](int b) {
    const int nr = min(TS_BS, n - TS_BS * b);
#pragma unroll
    for (int q = 0; q < NDQ; ++q) {
      const int e = u0 + 64 * NT * q, row = e & 31, col = (e >> 5) & 31;
      const bool in = row <= col && col < nr;
      const double x = *(in ? p.T.col(TS_BS * b + col) + TS_BS * b + row : p.T.T);
      dreg[q] = in ? x : (row == col ? 1.0 : 0.0);
    }
  };
  auto dstore = [&]() {
#pragma unroll
    for (int q = 0; q < NDQ; ++q) {
      const int e = u0 + 64 * NT * q, row = e & 31, col = e >> 5;
      if (e < TS_BS * TS_BS) {
        D[col * TS_DP + row] = dreg[q];
        if (row == col) Dinv[col] = 1.0 / dreg[q];
      }
    }
  };
  // this wave's tiles, in order: for target slot t = 1, 2, ..: the blocks solved in slots i = tw, tw + NT, .. < t
  int it = 1, ii = tw;
  auto settle = [&](int* t, int* i) { while (*t < nb && *i >= *t) { ++*t; *i = tw; } };
  settle(&it, &ii);
  // piece q of the tile (block solved in slot i) x (block of slot t): its rows are whole, its last columns may lie beyond the leaf
  auto tload = [&](int t, int i, d2_t (&st)[8]) {
    const int rb0 = TS_BS * (TR ? blk(i) : blk(t)), cb0 = TS_BS * (TR ? blk(t) : blk(i));
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int row = rb0 + (TR ? 8 * (q & 3) + 2 * g4 : 2 * l16), col = cb0 + (TR ? 16 * (q >> 2) + l16 : 4 * q + g4);
      const bool in = col < n;
      const d2_t x = __builtin_nontemporal_load((const d2u_t*)(p.T.col(in ? col : n - 1) + row));
      st[q] = in ? x : (d2_t){0.0, 0.0};
    }
  };
  d4_t acc[2][RB];
  auto zero_acc = [&]() {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) acc[h][rb] = (d4_t){0.0, 0.0, 0.0, 0.0};
  };
  d2_t cur[8], nxt[8];
  // multiply the tile in `cur`, with the following tile of the sequence on its way
  auto consume = [&]() {
    int nt = it, ni = ii + NT;
    settle(&nt, &ni);
    if (nt < nb) tload(nt, ni, nxt);
    const double* lx = X + xrow(blk(ii)) * 16;
    if (!TR) tt::mfma_row_dots<RB>(acc, lx + g4 * 16 + l16, PLANE, cur);
    else tt::mfma_col_dots<RB>(acc, lx + 2 * g4 * 16 + l16, PLANE, cur);
#pragma unroll
    for (int q = 0; q < 8; ++q) cur[q] = nxt[q];
    it = nt; ii = ni;
  };
  auto pstore = [&]() {
    double* pw = P + tw * RPAD * TS_BS;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        if (!TR) {
          *(d2_t*)(pw + (16 * rb + g4 + 4 * reg) * TS_BS + 2 * l16) = (d2_t){acc[0][rb][reg], acc[1][rb][reg]};
        } else {
#pragma unroll
          for (int t = 0; t < 2; ++t) pw[(16 * rb + l16) * TS_BS + 16 * t + g4 + 4 * reg] = acc[t][rb][reg];
        }
      }
  };

  zero_acc();
  dload(blk(0));
  if (it < nb) tload(it, ii, cur);
  for (int s = 0; s < nb; ++s) {
    __syncthreads();                               // #1
    if (it == s && ii == s - 1) consume();         // the block next to the diagonal one: it needed slot s - 1's rows
    pstore();
    zero_acc();
    dstore();
    __syncthreads();                               // #2
    if (s + 1 < nb) dload(blk(s + 1));
    while (it == s + 1 && ii < s) consume();       // block s + 1's tiles over the rows solved before this slot
  }
}

}  // namespace

extern "C" {

int capi_dtrsm_thin(capi_handle_t h, int trans, int64_t n, int64_t r, const double* T, int64_t ldt, int64_t col0, double* B, int64_t ldb) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE_THIN_R(h, r);
  CAPI_REQUIRE(h, trans == CAPI_NOTRANS || trans == CAPI_TRANS, "trans");
  CAPI_REQUIRE(h, n >= 0 && n < (1LL << 31), "n");
  CAPI_REQUIRE_TRI_VIEW(h, n, n, ldt, col0);
  CAPI_REQUIRE(h, ldb >= (n > 1 ? n : 1), "ldb");
  CAPI_REQUIRE(h, n == 0 || (T && B), "T / B");
  if (n == 0) return CAPI_OK;
  const int rb = capi_thin_rb(r), cw = r <= 4 ? 4 : (r <= 16 ? 16 : 32);
  const int v = (cw == 4 ? 0 : (cw == 16 ? 2 : 4)) + (trans ? 1 : 0);
  const tp::tri_view V{T, ldt, col0};
  const int rc = sp::for_each_step(trans, 0, n, [&](const sp::Step& s) -> int {
    if (s.kind == sp::STEP_PRODUCT) {
      const int64_t in0 = trans ? s.row0 : s.col0, out0 = trans ? s.col0 : s.row0;
      const tp::tri_view blk = V.sub(s.row0, s.col0);
      return capi_dtrmm_thin(h, CAPI_RECT, trans, s.m, s.n, r, -1.0, blk.T, blk.ldt, blk.col0, B + in0, ldb, 1.0, B + out0, ldb);
    }
    SolveArgs p;
    p.T = V.sub(s.row0, s.col0); p.B = B + s.row0;
    p.ldb = ldb;
    p.n = (int)s.n; p.r = (int)r;
    const size_t lds = sizeof(double) * ts_lds_doubles(rb);
#define TS_LAUNCH(RB, CW, TR)                                                                                                        \
    do {                                                                                                                             \
      CAPI_RAISE_LDS_LIMIT(h, CAPI_ATTR_TRSM_THIN0 + v, (trsm_thin_leaf_kernel<RB, CW, TR>), lds);                                    \
      hipLaunchKernelGGL((trsm_thin_leaf_kernel<RB, CW, TR>), dim3(1), dim3(64 * (TS_NT + 1)), lds, h->stream, p);        \
    } while (0)
    switch (v) {
      case 0: TS_LAUNCH(1, 4, false); break;
      case 1: TS_LAUNCH(1, 4, true); break;
      case 2: TS_LAUNCH(1, 16, false); break;
      case 3: TS_LAUNCH(1, 16, true); break;
      case 4: TS_LAUNCH(2, 32, false); break;
      default: TS_LAUNCH(2, 32, true); break;
    }
#undef TS_LAUNCH
    return CAPI_OK;
  });
  if (rc != CAPI_OK) return rc;
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

}  // extern "C"
