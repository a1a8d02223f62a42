// tri_reduce_f64.hip -- reductions over a (packed) triangle or rectangle that lies as capi_dtrmm_thin takes it: what a caller needs of the cholinv
// factors themselves (cholesky::cholinv::inverse_diagonal, log_determinant).  Not in the reference: its cholinv stops at R and R^-1.
//
//   capi_dtri_rownorm2   out[i] <- beta out[i] + sum_j T(i, j)^2      the diagonal of A^-1 from the rows of R^-1
//   capi_dtri_logdiag    out[0] <- sum_i log T(i, i)                  half the log-determinant of A from R
//
// capi_dtri_rownorm2 is the NOTRANS thin product of tri_apply_f64.hip with T's own entries standing in for the thin operand: its plan and slices
// (tri_thin_plan.h), its prologue, slabs and combine (tri_slab.h, one column), its pieces per lane (rows 2 l16, + 1 of column 4 q + g4 of the wave's
// 32 x 32 part), double-buffered in registers one tile ahead.  T is read from HBM once and the call is bound by that stream; there is no LDS, no barrier
// and no MFMA, so the waves of a workgroup need not keep step: each walks the whole tiles of its own 32 lines in a loop of its own (the diagonal meets
// every wave at another tile).  A lane squares its 16 elements into two sums, and where its workgroup leaves a group of lines the four lanes of a row
// pair meet in a fixed butterfly.
// Edges (ragged tiles, the tiles the diagonal crosses): every element is loaded from a clamped address and SELECTED afterwards, as in the product;
// nothing below the diagonal or outside the block is read into a sum, whatever it holds.
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

constexpr int TR_THREADS = 512;                 // 8 waves x 32 lines: one group
constexpr int TR_NP = 8;                        // 16-byte pieces of T per lane and tile

struct RowNormArgs {
  const double* T; double* slab;
  int64_t ldt, col0;
  int S;
  tp::Plan P;
  int64_t pos[tp::MAX_SLICES + 1];
};

__global__ __launch_bounds__(TR_THREADS) void tri_rownorm2_kernel(const RowNormArgs p) {
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15, g4 = lane >> 4;
  const int s = blockIdx.x;
  const int64_t p0 = p.pos[s], p1 = p.pos[s + 1];
  if (p0 >= p1) return;
  const bool tri = p.P.tri, packed = p.ldt == 0;
  const int64_t m = p.P.m, n = p.P.n;
  auto colptr = [&](int64_t j) { return packed ? p.T + tp::packed_col_offset(p.col0, j) : p.T + j * p.ldt; };   // tp::tri_view::col, as in trmm_thin_kernel
  auto valid = [&](int64_t row, int64_t col) { return row < m && col < n && (!tri || row <= col); };

  d2_t acc = (d2_t){0.0, 0.0};                   // rows 2 l16, + 1 of the wave's 32 lines, over this lane's columns
  auto square = [&](const d2_t (&cur)[TR_NP]) {
#pragma unroll
    for (int q = 0; q < TR_NP; ++q) acc += cur[q] * cur[q];
  };
  // An edge tile (ragged, or crossed by the diagonal), not pipelined: every element from a clamped address, selected afterwards
  auto edge_tile = [&](int64_t g, int64_t c) {
    const int64_t l0 = tp::GROUP * g + 32 * w, k0 = tp::DEPTH * c;
    if (l0 >= m || (tri && l0 > k0 + 31)) return;                         // wave-uniform: the wave's 32 x 32 part holds nothing
    d2_t st[TR_NP];
#pragma unroll
    for (int q = 0; q < TR_NP; ++q) {
      const int64_t row = l0 + 2 * l16, col = k0 + 4 * q + g4;
      const bool v0 = valid(row, col), v1 = valid(row + 1, col);
      const double* cp = colptr(col < n ? col : 0);
      const double x = *(v0 ? cp + row : p.T), y = *(v1 ? cp + row + 1 : p.T);    // p.T: the block's first element, always inside it
      st[q] = (d2_t){v0 ? x : 0.0, v1 ? y : 0.0};
    }
    square(st);
  };
  // The tiles c0 .. c1 - 1 of group g, each whole and inside the triangle for this wave: two register sets, the next tile's eight loads issued before
  // the current tile is squared, two tiles a round so that each set keeps its registers.  The eight column pointers advance by increments: from tile to
  // tile a column of the packed triangle moves by 32 x + 528 doubles (x its index in the triangle), 32 ldt in column-major storage; no multiplication and
  // no branch between the loads
  auto steady_run = [&](int64_t g, int64_t c0, int64_t c1) {
    const int64_t row = tp::GROUP * g + 32 * w + 2 * l16, col = tp::DEPTH * c0 + g4;
    const d2u_t* src[TR_NP];
#pragma unroll
    for (int q = 0; q < TR_NP; ++q) src[q] = (const d2u_t*)(colptr(col + 4 * q) + row);
    int64_t inc = packed ? 32 * (p.col0 + col) + 528 : 32 * p.ldt;        // piece 0's way to the next tile, in doubles; piece q: + 128 q when packed
    const int64_t dq = packed ? 128 : 0, dinc = packed ? 1024 : 0;
    // loads the tile that src points at and moves src on.  Between the two scheduling barriers nothing but the eight loads: left alone, the compiler
    // dealt the squares of the tile before among them, each behind a wait for its piece, and a wave had little more than one tile in flight
    auto tload = [&](d2_t (&st)[TR_NP]) {
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < TR_NP; ++q) st[q] = __builtin_nontemporal_load(src[q]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < TR_NP; ++q) src[q] = (const d2u_t*)((const double*)src[q] + (inc + q * dq));
      inc += dinc;
    };
    d2_t pa[TR_NP], pb[TR_NP];
    tload(pa);
    int64_t c = c0;
    for (; c + 2 < c1; c += 2) {                                          // pa holds tile c
      tload(pb);
      square(pa);
      tload(pa);
      square(pb);
    }
    if (c + 1 < c1) { tload(pb); square(pa); square(pb); }
    else square(pa);
  };
  // the group's partial sums, to this slice's slab for it: 256 lines
  auto flush = [&](int64_t g) {
    d2_t v = acc;
    v.x += __shfl_xor(v.x, 16); v.y += __shfl_xor(v.y, 16);
    v.x += __shfl_xor(v.x, 32); v.y += __shfl_xor(v.y, 32);
    if (g4 == 0) *(d2_t*)(p.slab + ts::slab_offset(s, g, 1) + 32 * w + 2 * l16) = v;
    acc = (d2_t){0.0, 0.0};
  };

  int64_t g, c;
  tp::locate(p.P, p0, &g, &c);
  for (int64_t q = p0; q < p1;) {
    // the slice's tiles of this group: c .. cE - 1; of them cs .. ce - 1 are whole and inside the triangle for this wave (wave-uniform)
    const int64_t cE = tp::min64(tp::first_tile(p.P, g) + tp::group_tiles(p.P, g), c + (p1 - q));
    const int64_t l0 = tp::GROUP * g + 32 * w;
    const bool whole = l0 + 32 <= m;
    const int64_t cs = whole ? (tri ? l0 / 32 + 1 : 0) : cE, ce = whole ? n / tp::DEPTH : cE;
    const int64_t s0 = tp::min64(tp::max64(c, cs), cE), s1 = tp::max64(s0, tp::min64(cE, ce));
    for (int64_t cc = c; cc < s0; ++cc) edge_tile(g, cc);
    if (s1 > s0) steady_run(g, s0, s1);
    for (int64_t cc = s1; cc < cE; ++cc) edge_tile(g, cc);
    flush(g);
    q += cE - c;
    ++g;
    c = tp::first_tile(p.P, g);
  }
}

constexpr int LD_THREADS = 256;

// One workgroup.  A thread adds the logarithms of the entries tid, tid + 256, ..; the 256 sums meet pairwise: a butterfly inside the wave, then the
// four waves as (0 + 1) + (2 + 3)
__global__ __launch_bounds__(LD_THREADS) void tri_logdiag_kernel(int64_t n, const tp::tri_view T, double* __restrict__ out) {
  __shared__ double red[4];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += LD_THREADS) s += log(*T.at(i, i));
  s = tt::butterfly_sum<64>(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace

extern "C" {

int capi_dtri_rownorm2(capi_handle_t h, int shape, int64_t m, int64_t n, const double* T, int64_t ldt, int64_t col0, double beta, double* out) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE(h, shape == CAPI_RECT || shape == CAPI_UPPERTRI, "shape: CAPI_RECT or CAPI_UPPERTRI");
  CAPI_REQUIRE(h, m >= 0 && n >= 0 && m < (1LL << 31) && n < (1LL << 31), "m / n");
  CAPI_REQUIRE(h, shape != CAPI_UPPERTRI || m == n, "CAPI_UPPERTRI: m == n");
  CAPI_REQUIRE_TRI_VIEW(h, m, n, ldt, col0);
  CAPI_REQUIRE(h, m == 0 || out, "out");
  CAPI_REQUIRE(h, m == 0 || n == 0 || T, "T");
  if (m == 0) return CAPI_OK;
  ts::CombineArgs cp;
  RowNormArgs p;
  const int rc = ts::plan_slabs(h, shape, CAPI_NOTRANS, m, n, 1, &cp, &p);
  if (rc != CAPI_OK) return rc;
  if (cp.S > 0) {
    p.T = T; p.ldt = ldt; p.col0 = col0;
    hipLaunchKernelGGL(tri_rownorm2_kernel, dim3((unsigned)cp.S), dim3(TR_THREADS), 0, h->stream, p);
  }
  ts::combine(h, cp, 1, 1.0, beta, out, m);                               // one column of m lines; 1.0 * sum is sum
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

int capi_dtri_logdiag(capi_handle_t h, int64_t n, const double* T, int64_t ldt, int64_t col0, double* out) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE(h, n >= 0 && n < (1LL << 31) && out && (n == 0 || T), "n / T / out");
  CAPI_REQUIRE_TRI_VIEW(h, n, n, ldt, col0);
  hipLaunchKernelGGL(tri_logdiag_kernel, dim3(1), dim3(LD_THREADS), 0, h->stream, n, tp::tri_view{T, ldt, col0}, out);
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

}  // extern "C"
