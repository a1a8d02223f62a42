// tri_apply_f64.hip -- a (packed) triangle or rectangle times a THIN block (r <= 32 columns), for solves on the cholinv factors
// (cholesky::cholinv::solve).  Not in the reference: its cholinv stops at R and R^-1.
//
//   capi_dtrmm_thin   C <- alpha op(T) B + beta C      T m x n (all of it, or its upper triangle), column-major or a view into a packed triangle
//
// T is read from HBM once and the call is bound by that stream; the arithmetic goes to v_mfma_f64_16x16x4_f64 with the r columns padded to 16 or 32.
// The work is cut into tiles of 256 output lines x 32 contraction indices and dealt to one workgroup per CU by equal BYTES (tri_thin_plan.h): the
// lines of a triangle have lengths 1..n.  A workgroup walks its consecutive tiles; the 256 x rpad partial sums of every group of lines it
// touches go to a slab of its own and are added by a second launch (tri_slab.h: the prologue, the slot rule, the combine).
// The thin operand is stationary in LDS, 256 contraction indices at a time in two halves: the next block is fetched while the last tile of the
// current one is multiplied, one barrier per block.  T's pieces are double-buffered in registers, one tile (8 x 16 bytes per lane) ahead.  A wave's
// 32 x 32 part of a tile is multiplied in the row-dot form of thin_tile.h for NOTRANS and in its column-dot form for TRANS.
// Alignment: a packed column starts at x (x + 1) / 2, so every other pair of columns is 8-byte aligned only; the steady loop loads 16 bytes from
// such a column all the same (d2u_t of thin_tile.h); no column falls back to scalar loads.
// Measured (profiles/cholinv_solve.txt, n = 32768): packed against full storage costs 1.2 x for NOTRANS and 1.4 x for TRANS, misaligned loads and
// the 64-bit column address together; a peeled head element with aligned loads behind it is not built.
// Offsets into the packed triangle are 64-bit throughout: column 65536 starts beyond 2^31 doubles.
// Edges (ragged tiles, the tiles the diagonal crosses): a generic step that loads every element from a clamped address and selects afterwards;
// nothing below the diagonal or outside the block takes part, whatever it holds.
#include <type_traits>
#include "capi_internal.h"
#include "thin_tile.h"
#include "tri_slab.h"
#include "tri_thin_plan.h"

namespace {

namespace tp = tri_thin_plan;
namespace tt = thin_tile;
namespace ts = tri_slab;
using tt::d2_t;
using tt::d2u_t;
using tt::d4_t;

constexpr int TT_THREADS = 512;                 // 8 waves, one workgroup per CU
constexpr int TT_BLK = tp::GROUP;               // contraction indices of the thin operand per LDS half (8 tiles)
constexpr int TT_NP = 8;                        // 16-byte pieces of T per lane and tile

struct ThinArgs {
  const double* T; const double* B; double* slab;
  int64_t ldt, col0, ldb;
  int r, S;
  tp::Plan P;
  int64_t pos[tp::MAX_SLICES + 1];
};

template <int RB, bool TR>
__global__ __launch_bounds__(TT_THREADS) void trmm_thin_kernel(const ThinArgs p) {
  extern __shared__ __attribute__((aligned(16))) double Lb[];   // [2][RB][TT_BLK][16]: B(256 blk + k, 16 rb + jj)
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15, g4 = lane >> 4;
  const int s = blockIdx.x;
  const int64_t p0 = p.pos[s], p1 = p.pos[s + 1];
  if (p0 >= p1) return;
  const bool tri = p.P.tri;
  const int64_t m = p.P.m, n = p.P.n;
  // tp::tri_view::col on the fields where they lie: held as a tri_view they load in another order and the kernels come out in another schedule
  auto colptr = [&](int64_t j) { return p.ldt > 0 ? p.T + j * p.ldt : p.T + tp::packed_col_offset(p.col0, j); };
  auto valid = [&](int64_t row, int64_t col) { return row < m && col < n && (!tri || row <= col); };

  // ---- the thin operand: thread t fetches contraction indices t & 255 of columns (t >> 8) + 2 q ----
  const int fk = tid & (TT_BLK - 1), fj = tid >> 8;
  double bst[8 * RB];
  auto bload = [&](int64_t blk) {
    const int64_t k = blk * TT_BLK + fk;
#pragma unroll
    for (int q = 0; q < 8 * RB; ++q) {
      const int j = fj + 2 * q;
      const bool in = k < p.P.depth && j < p.r;
      bst[q] = *(in ? p.B + k + (int64_t)j * p.ldb : p.B);
    }
  };
  auto bstore = [&](double* L, int64_t blk) {
    const int64_t k = blk * TT_BLK + fk;
#pragma unroll
    for (int q = 0; q < 8 * RB; ++q) {
      const int j = fj + 2 * q;
      L[((j >> 4) * TT_BLK + fk) * 16 + (j & 15)] = (k < p.P.depth && j < p.r) ? bst[q] : 0.0;
    }
  };

  // ---- T's piece q of tile (g, c) for this lane: wave w's 32 lines of group g x the tile's 32 contraction indices ----
  auto piece = [&](int64_t g, int64_t c, int q, int64_t* row, int64_t* col) {
    if (!TR) { *row = tp::GROUP * g + 32 * w + 2 * l16; *col = tp::DEPTH * c + 4 * q + g4; }
    else { *row = tp::DEPTH * c + 8 * (q & 3) + 2 * g4; *col = tp::GROUP * g + 32 * w + 16 * (q >> 2) + l16; }
  };
  // wave-uniform: the wave's 32 x 32 part of the tile holds something / is whole and inside the triangle
  auto live = [&](int64_t g, int64_t c) {
    const int64_t l0 = tp::GROUP * g + 32 * w, k0 = tp::DEPTH * c;       // first line, first contraction index
    if (l0 >= p.P.lines) return false;
    if (!tri) return true;
    return TR ? k0 <= l0 + 31 : l0 <= k0 + 31;
  };
  auto steady = [&](int64_t g, int64_t c) {
    const int64_t l0 = tp::GROUP * g + 32 * w, k0 = tp::DEPTH * c;
    if (l0 + 32 > p.P.lines || k0 + 32 > p.P.depth) return false;
    if (!tri) return true;
    return TR ? k0 + 31 <= l0 : l0 + 31 <= k0;
  };
  auto tload_steady = [&](int64_t g, int64_t c, d2_t (&st)[TT_NP]) {
#pragma unroll
    for (int q = 0; q < TT_NP; ++q) {
      int64_t row, col;
      piece(g, c, q, &row, &col);
      st[q] = __builtin_nontemporal_load((const d2u_t*)(colptr(col) + row));
    }
  };
  auto tload_edge = [&](int64_t g, int64_t c, d2_t (&st)[TT_NP]) {
#pragma unroll
    for (int q = 0; q < TT_NP; ++q) {
      int64_t row, col;
      piece(g, c, q, &row, &col);
      const bool v0 = valid(row, col), v1 = valid(row + 1, col);
      const double* cp = colptr(col < n ? col : 0);
      const double x = *(v0 ? cp + row : p.T), y = *(v1 ? cp + row + 1 : p.T);
      st[q] = (d2_t){v0 ? x : 0.0, v1 ? y : 0.0};
    }
  };

  d4_t acc[2][RB];
  auto zero_acc = [&]() {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) acc[h][rb] = (d4_t){0.0, 0.0, 0.0, 0.0};
  };
  auto multiply = [&](const double* L, int64_t c, const d2_t (&cur)[TT_NP]) {
    const int kb = (int)(c & (tp::CPG - 1)) * tp::DEPTH;                  // the tile's place inside the LDS block
    __builtin_amdgcn_s_setprio(1);
    if (!TR) tt::mfma_row_dots<RB>(acc, L + (kb + g4) * 16 + l16, TT_BLK * 16, cur);
    else tt::mfma_col_dots<RB>(acc, L + (kb + 2 * g4) * 16 + l16, TT_BLK * 16, cur);
    __builtin_amdgcn_s_setprio(0);
  };
  // the group's partial sums, to this slice's slab for it: [16 RB columns][256 lines]
  auto flush = [&](int64_t g) {
    double* sl = p.slab + ts::slab_offset(s, g, 16 * RB);
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        if (!TR) {
          *(d2_t*)(sl + (16 * rb + g4 + 4 * reg) * tp::GROUP + 32 * w + 2 * l16) = (d2_t){acc[0][rb][reg], acc[1][rb][reg]};
        } else {
#pragma unroll
          for (int t = 0; t < 2; ++t) sl[(16 * rb + l16) * tp::GROUP + 32 * w + 16 * t + g4 + 4 * reg] = acc[t][rb][reg];
        }
      }
  };

  // one tile: prefetch the following tile's piece (and, at a block change, the thin operand's next block), multiply this one
  int par = 0;
  auto step = [&](int64_t g, int64_t c, d2_t (&cur)[TT_NP], d2_t (&nxt)[TT_NP], int64_t ng, int64_t nc, bool has_next, auto steady_tag) {
    constexpr bool STEADY = decltype(steady_tag)::value;
    if (STEADY) tload_steady(ng, nc, nxt);
    else if (has_next && live(ng, nc)) tload_edge(ng, nc, nxt);
    const bool refill = has_next && (nc >> 3) != (c >> 3);               // workgroup-uniform
    if (live(g, c)) multiply(Lb + par * (RB * TT_BLK * 16), c, cur);
    if (!has_next || ng != g) { flush(g); zero_acc(); }
    if (refill) {
      // the other half was last read before the previous block change's barrier.  (The block is fetched here, not ahead of the multiply:
      // its 16 values per thread across the MFMA phase cost spills at r > 16; it comes from L2 once per 8 tiles, beside the other waves' work)
      bload(nc >> 3);
      bstore(Lb + (par ^ 1) * (RB * TT_BLK * 16), nc >> 3);
      __syncthreads();
      par ^= 1;
    }
  };

  int64_t g, c;
  tp::locate(p.P, p0, &g, &c);
  int64_t gend = tp::first_tile(p.P, g) + tp::group_tiles(p.P, g);       // one past the group's last tile
  zero_acc();
  bload(c >> 3);
  d2_t pa[TT_NP], pb[TT_NP];
  if (live(g, c)) { if (steady(g, c)) tload_steady(g, c, pa); else tload_edge(g, c, pa); }
  bstore(Lb, c >> 3);
  __syncthreads();
  for (int64_t q = p0; q < p1; ++q) {
    int64_t ng = g, nc = c + 1, ngend = gend;
    if (nc == gend) { ng = g + 1; nc = tp::first_tile(p.P, ng); ngend = nc + tp::group_tiles(p.P, ng); }
    const bool has_next = q + 1 < p1, st = has_next && live(ng, nc) && steady(ng, nc);
    if ((q - p0) & 1) {
      if (st) step(g, c, pb, pa, ng, nc, has_next, std::true_type{}); else step(g, c, pb, pa, ng, nc, has_next, std::false_type{});
    } else {
      if (st) step(g, c, pa, pb, ng, nc, has_next, std::true_type{}); else step(g, c, pa, pb, ng, nc, has_next, std::false_type{});
    }
    g = ng; c = nc; gend = ngend;
  }
}

}  // namespace

extern "C" {

int capi_dtrmm_thin(capi_handle_t h, int shape, int trans, int64_t m, int64_t n, int64_t r, double alpha, const double* T, int64_t ldt, int64_t col0,
                    const double* B, int64_t ldb, double beta, double* C, int64_t ldc) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE_THIN_R(h, r);
  CAPI_REQUIRE(h, shape == CAPI_RECT || shape == CAPI_UPPERTRI, "shape: CAPI_RECT or CAPI_UPPERTRI");
  CAPI_REQUIRE(h, trans == CAPI_NOTRANS || trans == CAPI_TRANS, "trans");
  CAPI_REQUIRE(h, m >= 0 && n >= 0 && m < (1LL << 31) && n < (1LL << 31), "m / n");
  CAPI_REQUIRE(h, shape != CAPI_UPPERTRI || m == n, "CAPI_UPPERTRI: m == n");
  CAPI_REQUIRE_TRI_VIEW(h, m, n, ldt, col0);
  const int64_t lines = trans ? n : m, depth = trans ? m : n;
  CAPI_REQUIRE(h, ldb >= (depth > 1 ? depth : 1) && ldc >= (lines > 1 ? lines : 1), "ldb / ldc");
  CAPI_REQUIRE(h, lines == 0 || C, "C");
  CAPI_REQUIRE(h, lines == 0 || depth == 0 || (T && B && B != C), "T / B (C must not alias B)");
  if (lines == 0) return CAPI_OK;
  const int rb = capi_thin_rb(r);
  ts::CombineArgs cp;
  ThinArgs p;
  const int rc = ts::plan_slabs(h, shape, trans, m, n, 16 * rb, &cp, &p);
  if (rc != CAPI_OK) return rc;
  if (cp.S > 0) {
    p.T = T; p.B = B;
    p.ldt = ldt; p.col0 = col0; p.ldb = ldb;
    p.r = (int)r;
    const size_t lds = sizeof(double) * 2 * (size_t)rb * TT_BLK * 16;
    const int v = 2 * (rb - 1) + (trans ? 1 : 0);
#define TT_LAUNCH(RB, TR)                                                                                                  \
    do {                                                                                                                   \
      CAPI_RAISE_LDS_LIMIT(h, CAPI_ATTR_TRMM_THIN0 + v, (trmm_thin_kernel<RB, TR>), lds);                                   \
      hipLaunchKernelGGL((trmm_thin_kernel<RB, TR>), dim3((unsigned)cp.S), dim3(TT_THREADS), lds, h->stream, p);            \
    } while (0)
    if (v == 0) TT_LAUNCH(1, false); else if (v == 1) TT_LAUNCH(1, true); else if (v == 2) TT_LAUNCH(2, false); else TT_LAUNCH(2, true);
#undef TT_LAUNCH
  }
  ts::combine(h, cp, (int)r, alpha, beta, C, ldc);
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

}  // extern "C"
