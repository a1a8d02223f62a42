// qr_apply_f64.hip -- capi_dormqr, capi_dgels and capi_dgelsy for gfx950: Q or Q^T of a capi_dgeqrf image applied to a block without forming Q, the
// Householder least-squares solve built on it, and the rank-revealing one (capi_dgeqp3 of qrcp_f64.hip on the n x n triangle).  Not in the reference: lapack/interface.h declares _geqrf and _orgqr only.
//
// THIN PATH (r <= CAPI_TS_MAX_RHS): panels of 32 reflectors (csrc/ormqr_plan.h), three launches per panel at j0, P = the unit lower trapezoid of
// A[j0:m, j0:j0+nb] and Cp = C[j0:m, :]:
//   1. ormqr_gram_kernel    P^T [P | Cp] in ONE pass: G = P^T P and W = P^T Cp from the same loaded registers.  The 8 waves of a workgroup split
//                           ROWS: a wave owns 32-row tiles and holds its tile of P in thin_tile.h's column-dot arrangement (lane (l16, g4): row
//                           pairs 8 q + 2 g4, + 1 of its own column l16 of a 16-column strip).  That arrangement is at once the MFMA's A operand
//                           (P^T) and its B operand (P), and the wave's rows of Cp load in the same arrangement as further strips: with the rows
//                           dealt to waves no operand is shared between waves, so nothing is staged through LDS.  Only the upper blocks (0,0),
//                           (0,1), (1,1) of G are formed (dlarft reads G above the diagonal).  Workgroup z takes a row slice and writes slab z.
//   2. ormqr_small_kernel   one workgroup: adds the slabs in the order z = 0, 1, .., forms T from G and tau by larft_kernel's recurrence, Z = T^T W
//                           (Q^T) or T W (Q), and updates the panel's top 32 rows of Cp, where P carries its mask, in place.
//   3. capi_dresid_ts       Cp[32:, :] -= P[32:, :] Z in place (Rout == B, X = Z): the row-dot kernel that is shaped for a 32-column A.
// Nothing on or above A's diagonal is ever loaded into a product: the unit diagonal and the zeros above it are selected, not multiplied in.
// The panel is read from HBM twice, the live rows of C twice and written once; no m-long temporary, no copy of V.  Every sum has a fixed order.
// WIDE PATH (r > 32): capi_qr_apply_wide of qr_f64.hip, the block-reflector loop of capi_dorgqr on the tile kernel.
#include "capi_internal.h"
#include "ormqr_plan.h"
#include "thin_tile.h"

namespace {

namespace tt = thin_tile;
namespace op = ormqr_plan;
using tt::d2_t;
using tt::d4_t;

constexpr int GR_THREADS = 64 * op::WAVES;
constexpr int SM_THREADS = 1024;
constexpr int MAXE = 7 * 256;            // doubles of a slab at rb = 2

struct GramArgs {
  const double* P; const double* C; double* slab;      // P = &A[j0][j0], C = &C[j0][0]
  int64_t rows, lda, ldc;
  int nb, r, vec;
  op::Slices sl;
};

#define RC(x) do { int rc__ = (x); if (rc__ != CAPI_OK) return rc__; } while (0)

template <int RB>
__global__ __launch_bounds__(GR_THREADS) void ormqr_gram_kernel(const GramArgs p) {
  constexpr int NBLK = 3 + 2 * RB;
  __shared__ double red[NBLK * 256];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15, g4 = lane >> 4;
  const int z = blockIdx.x;
  const int64_t rd0 = op::round_begin(p.sl, z), rd1 = op::round_begin(p.sl, z + 1);
  d4_t g00 = {0.0, 0.0, 0.0, 0.0}, g01 = g00, g11 = g00;
  d4_t wacc[2][RB];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) wacc[t][rb] = g00;

  // the lane's pieces of tile `tile`: pa[4 t + q] = rows 8 q + 2 g4, + 1 of column 16 t + l16 of P, ca[rb][q] the same rows of column 16 rb + l16 of C
  auto load_steady = [&](int64_t tile, d2_t (&pa)[8], d2_t (&ca)[RB][4]) {      // whole tile below the panel's top block, nb == 32, 16-byte aligned
    const int64_t row = tile * op::TILE + 2 * g4;
    const double* ps = p.P + row + (int64_t)l16 * p.lda;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) pa[4 * t + q] = __builtin_nontemporal_load((const d2_t*)(ps + (int64_t)(16 * t) * p.lda + 8 * q));
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const int col = 16 * rb + l16;
      const bool in = col < p.r;
      const double* cs = p.C + row + (int64_t)(in ? col : 0) * p.ldc;           // a clamped address; the select follows the load
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const d2_t v = *(const d2_t*)(cs + 8 * q);
        ca[rb][q] = in ? v : (d2_t){0.0, 0.0};
      }
    }
  };
  // P's element (i, c) of the panel: nothing on or above the diagonal is loaded
  auto p_at = [&](int64_t i, int c) -> double {
    if (c >= p.nb || i >= p.rows || i < c) return 0.0;
    if (i == c) return 1.0;
    return p.P[i + (int64_t)c * p.lda];
  };
  auto c_at = [&](int64_t i, int c) -> double { return (c < p.r && i < p.rows) ? p.C[i + (int64_t)c * p.ldc] : 0.0; };
  auto load_edge = [&](int64_t tile, d2_t (&pa)[8], d2_t (&ca)[RB][4]) {        // the masked top tile, a ragged tile, a short panel, unaligned operands
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t row = tile * op::TILE + 8 * q + 2 * g4;
#pragma unroll
      for (int t = 0; t < 2; ++t) pa[4 * t + q] = (d2_t){p_at(row, 16 * t + l16), p_at(row + 1, 16 * t + l16)};
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) ca[rb][q] = (d2_t){c_at(row, 16 * rb + l16), c_at(row + 1, 16 * rb + l16)};
    }
  };
  auto steady = [&](int64_t tile) { return p.vec && p.nb == op::NB && tile > 0 && (tile + 1) * op::TILE <= p.rows; };
  auto load = [&](int64_t tile, d2_t (&pa)[8], d2_t (&ca)[RB][4]) {
    if (steady(tile)) load_steady(tile, pa, ca); else load_edge(tile, pa, ca);
  };
  auto multiply = [&](const d2_t (&pa)[8], const d2_t (&ca)[RB][4]) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const double a0 = hh ? pa[q].y : pa[q].x, a1 = hh ? pa[4 + q].y : pa[4 + q].x;
        g00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a0, g00, 0, 0, 0);
        g01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a1, g01, 0, 0, 0);
        g11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, a1, g11, 0, 0, 0);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          const double cv = hh ? ca[rb][q].y : ca[rb][q].x;
          wacc[0][rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, cv, wacc[0][rb], 0, 0, 0);
          wacc[1][rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, cv, wacc[1][rb], 0, 0, 0);
        }
      }
    __builtin_amdgcn_s_setprio(0);
  };
  // wave w takes tile 8 rd + w of every round rd of the slice; the next tile's loads are in flight during a tile's products
  d2_t pa[8], ca[RB][4], pn[8], cn[RB][4];
  int64_t tile = rd0 * op::WAVES + w;
  const int64_t tend = rd1 * op::WAVES < p.sl.tiles ? rd1 * op::WAVES : p.sl.tiles;
  if (tile < tend) load(tile, pa, ca);
  while (tile < tend) {
    const int64_t next = tile + op::WAVES;
    if (next < tend) load(next, pn, cn);
    multiply(pa, ca);
    tile = next;
    if (tile >= tend) break;
    if (tile + op::WAVES < tend) load(tile + op::WAVES, pa, ca);
    multiply(pn, cn);
    tile += op::WAVES;
  }
  // lane (l16, g4) holds element (g4 + 4 reg, l16) of each 16 x 16 block: the waves add theirs in the order 0 .. 7
  for (int ww = 0; ww < op::WAVES; ++ww) {
    if (w == ww) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int e = (g4 + 4 * reg) * 16 + l16;
        if (ww == 0) {
          red[e] = g00[reg]; red[256 + e] = g01[reg]; red[512 + e] = g11[reg];
#pragma unroll
          for (int rb = 0; rb < RB; ++rb) { red[(3 + 2 * rb) * 256 + e] = wacc[0][rb][reg]; red[(4 + 2 * rb) * 256 + e] = wacc[1][rb][reg]; }
        } else {
          red[e] += g00[reg]; red[256 + e] += g01[reg]; red[512 + e] += g11[reg];
#pragma unroll
          for (int rb = 0; rb < RB; ++rb) { red[(3 + 2 * rb) * 256 + e] += wacc[0][rb][reg]; red[(4 + 2 * rb) * 256 + e] += wacc[1][rb][reg]; }
        }
      }
    }
    __syncthreads();
  }
  double* sl = p.slab + (int64_t)z * (NBLK * 256);
  for (int e = tid; e < NBLK * 256; e += GR_THREADS) sl[e] = red[e];
}

struct SmallArgs {
  const double* slab; const double* tau; const double* P; double* C; double* Z;   // tau = &tau[j0]; Z: 32 x 32, ld 32
  int64_t rows, lda, ldc;
  int S, rb, nb, r, trans;
};

// block b of a slab holds [16 rows][16 columns]; G(l, i) for l <= i, W(l, c)
__device__ __forceinline__ int g_index(int l, int i) { return ((l >> 4) + (i >> 4)) * 256 + (l & 15) * 16 + (i & 15); }
__device__ __forceinline__ int w_index(int l, int c) { return (3 + 2 * (c >> 4) + (l >> 4)) * 256 + (l & 15) * 16 + (c & 15); }

__global__ __launch_bounds__(SM_THREADS) void ormqr_small_kernel(const SmallArgs p) {
  __shared__ double sum[MAXE];
  __shared__ double t[op::NB][op::NB + 1];
  __shared__ double zs[op::NB][op::NB + 1];
  __shared__ double ptop[op::NB][op::NB + 1];
  const int tid = threadIdx.x, E = op::slab_doubles(p.rb);
  // 1. the slabs, in slab order.  Columns of W beyond r hold zeros and are not read
  for (int e = tid; e < E; e += SM_THREADS) {
    double s = 0.0;
    if (e < 3 * 256 || 16 * ((e / 256 - 3) >> 1) + (e & 15) < p.r) {
      const double* src = p.slab + e;
#pragma unroll 16
      for (int z = 0; z < p.S; ++z) s += src[(int64_t)z * E];
    }
    sum[e] = s;
  }
  // the panel's top block with its mask: ptop[i][k] = P(i, k) strictly below the diagonal, 1 on it, 0 above (selected, never loaded)
  const int i0 = tid & 31, c0 = tid >> 5;
  {
    const int i = i0, k = c0;
    double v = 0.0;
    if (k < p.nb && i < p.rows) v = i > k ? p.P[i + (int64_t)k * p.lda] : (i == k ? 1.0 : 0.0);
    ptop[i][k] = v;
    t[i][k] = 0.0;
  }
  __syncthreads();
  // 2. dlarft (forward, columnwise) as larft_kernel runs it: T(0:i, i) = -tau_i T(0:i, 0:i) G(0:i, i)
  for (int i = 0; i < p.nb; ++i) {
    const double ti = p.tau[i];
    double s = 0.0;
    if (tid < i)
      for (int l = tid; l < i; ++l) s += t[tid][l] * sum[g_index(l, i)];
    __syncthreads();
    if (tid < i) t[tid][i] = -ti * s;
    if (tid == i) t[i][i] = ti;
    __syncthreads();
  }
  // 3. Z = T^T W (Q^T) or T W (Q): thread (i0, c0) owns Z(i0, c0)
  {
    double s = 0.0;
    if (i0 < p.nb && c0 < p.r) {
      if (p.trans) { for (int l = 0; l <= i0; ++l) s += t[l][i0] * sum[w_index(l, c0)]; }
      else { for (int l = i0; l < p.nb; ++l) s += t[i0][l] * sum[w_index(l, c0)]; }
      p.Z[i0 + op::NB * c0] = s;
    }
    zs[i0][c0] = s;
  }
  __syncthreads();
  // 4. the top rows of the panel: C(i, c) -= sum_k P(i, k) Z(k, c)
  if (i0 < p.rows && c0 < p.r) {
    double s = 0.0;
    for (int k = 0; k < p.nb; ++k) s += ptop[i0][k] * zs[k][c0];
    p.C[i0 + (int64_t)c0 * p.ldc] -= s;
  }
}

// info[0] <- the 1-based index of the first diagonal entry of R (order n, in A) that is zero or not finite, or 0
__global__ __launch_bounds__(256) void gels_diag_scan_kernel(const double* __restrict__ A, int64_t lda, int n, int* __restrict__ info) {
  __shared__ int first[256];
  int f = 0x7fffffff;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double d = A[i + (int64_t)i * lda];
    if (!(d != 0.0 && fabs(d) <= 1.7976931348623157e308) && i + 1 < f) f = i + 1;
  }
  first[threadIdx.x] = f;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o && first[threadIdx.x + o] < first[threadIdx.x]) first[threadIdx.x] = first[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *info = first[0] == 0x7fffffff ? 0 : first[0];
}

// Z (n x k, ldz) <- [R11 R12]^T from the upper trapezoid of capi_dgeqp3's image F: Z(i, l) = F(l, i) for i >= l, an exact zero above (what lies below
// F's diagonal, the reflectors, is not read).  32 x 32 tiles through LDS: reads run down F's columns, writes down Z's
__global__ __launch_bounds__(256) void gelsy_transpose_kernel(int n, int k, const double* __restrict__ F, int64_t ldf, double* __restrict__ Z, int64_t ldz) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int i0 = blockIdx.x * 32, l0 = blockIdx.y * 32;                     // tile: rows l0 .. of F (columns of Z), columns i0 .. of F (rows of Z)
  for (int q = ty; q < 32; q += 8) {
    const int l = l0 + tx, i = i0 + q;
    tile[q][tx] = (l < k && i < n && i >= l) ? F[l + (int64_t)i * ldf] : 0.0;
  }
  __syncthreads();
  for (int q = ty; q < 32; q += 8) {
    const int i = i0 + tx, l = l0 + q;
    if (i < n && l < k) Z[i + (int64_t)l * ldz] = tile[tx][q];
  }
}

// rows r0 .. r1 - 1 of B (ldb, ncols columns) <- 0
__global__ __launch_bounds__(256) void gelsy_zero_rows_kernel(int64_t r0, int64_t r1, int64_t ncols, double* __restrict__ B, int64_t ldb) {
  const int64_t i = r0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= r1) return;
  for (int64_t j = blockIdx.y; j < ncols; j += gridDim.y) B[i + j * ldb] = 0.0;
}

bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int ormqr_thin(capi_handle_t h, int trans, int64_t m, int64_t r, int64_t k, const double* A, int64_t lda, const double* tau, double* C, int64_t ldc) {
  const int rb = capi_thin_rb(r), cus = capi_stream_cus(h);
  void* pv = nullptr;
  RC(capi_ws3_get(h, sizeof(double) * (size_t)op::workspace_doubles(m, rb, cus), &pv));
  double* ws = (double*)pv;
  const int vec = aligned16(A) && aligned16(C) && (lda & 1) == 0 && (ldc & 1) == 0;
  const int64_t steps = op::num_panels(k);
  for (int64_t step = 0; step < steps; ++step) {
    const op::Panel pn = op::panel(m, k, trans == CAPI_TRANS, step);
    const double* P = A + pn.j0 + pn.j0 * lda;
    double* Cp = C + pn.j0;
    GramArgs g;
    g.P = P; g.C = Cp; g.slab = ws + op::slab_offset(rb, 0);
    g.rows = pn.rows; g.lda = lda; g.ldc = ldc;
    g.nb = pn.nb; g.r = (int)r; g.vec = vec;
    g.sl = op::slices(pn.rows, cus);
    if (rb == 1) hipLaunchKernelGGL(ormqr_gram_kernel<1>, dim3((unsigned)g.sl.S), dim3(GR_THREADS), 0, h->stream, g);
    else hipLaunchKernelGGL(ormqr_gram_kernel<2>, dim3((unsigned)g.sl.S), dim3(GR_THREADS), 0, h->stream, g);
    SmallArgs s;
    s.slab = g.slab; s.tau = tau + pn.j0; s.P = P; s.C = Cp; s.Z = ws;
    s.rows = pn.rows; s.lda = lda; s.ldc = ldc;
    s.S = g.sl.S; s.rb = rb; s.nb = pn.nb; s.r = (int)r; s.trans = trans == CAPI_TRANS;
    hipLaunchKernelGGL(ormqr_small_kernel, dim3(1), dim3(SM_THREADS), 0, h->stream, s);
    CAPI_HIP_CHECK(h, hipGetLastError());
    if (pn.rows > op::NB)
      RC(capi_dresid_ts(h, pn.rows - op::NB, pn.nb, r, P + op::NB, lda, ws, op::NB, Cp + op::NB, ldc, Cp + op::NB, ldc, nullptr));
  }
  return CAPI_OK;
}

}  // namespace

extern "C" {

int capi_dormqr(capi_handle_t h, int side, int trans, int64_t m, int64_t r, int64_t k, const double* A, int64_t lda, const double* tau, double* C,
                int64_t ldc) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE(h, side == CAPI_LEFT, "side: CAPI_LEFT only (C Q and C Q^T are not served)");
  CAPI_REQUIRE(h, trans == CAPI_NOTRANS || trans == CAPI_TRANS, "trans");
  CAPI_REQUIRE(h, m >= 0 && r >= 0 && k >= 0 && k <= m && m < (1LL << 31) && r < (1LL << 31), "dims (m >= k >= 0, r >= 0)");
  if (m == 0 || r == 0 || k == 0) return CAPI_OK;
  CAPI_REQUIRE(h, A && tau && C && lda >= m && ldc >= m, "operands");
  if (r > CAPI_TS_MAX_RHS) return capi_qr_apply_wide(h, trans, m, r, k, A, lda, tau, C, ldc);
  return ormqr_thin(h, trans, m, r, k, A, lda, tau, C, ldc);
}

int capi_dgels(capi_handle_t h, int64_t m, int64_t n, int64_t r, double* A, int64_t lda, double* tau, double* B, int64_t ldb, double* colnorm2,
               int* info_host) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE(h, n >= 1 && m >= n && r >= 1 && m < (1LL << 31) && r < (1LL << 31), "dims (m >= n >= 1, r >= 1: minimum-norm solutions are not served)");
  CAPI_REQUIRE(h, A && tau && B && info_host && lda >= m && ldb >= m, "operands");
  RC(capi_dgeqrf(h, m, n, A, lda, tau));
  RC(capi_dormqr(h, CAPI_LEFT, CAPI_TRANS, m, r, n, A, lda, tau, B, ldb));
  void* pv = nullptr;
  RC(capi_ws3_get(h, 64, &pv));
  hipLaunchKernelGGL(gels_diag_scan_kernel, dim3(1), dim3(256), 0, h->stream, (const double*)A, lda, (int)n, (int*)pv);
  CAPI_HIP_CHECK(h, hipGetLastError());
  int info = 0;
  RC(capi_memcpy_d2h(h, &info, pv, sizeof(int)));            // the call's own synchronisation
  *info_host = info;
  if (info != 0) return CAPI_OK;                             // B stays Q^T B: no solve, no norms
  for (int64_t j = 0; j < r; j += CAPI_TS_MAX_RHS) {
    const int64_t rb = r - j < CAPI_TS_MAX_RHS ? r - j : CAPI_TS_MAX_RHS;
    RC(capi_dtrsm_thin(h, CAPI_NOTRANS, n, rb, A, lda, 0, B + j * ldb, ldb));
    if (colnorm2) RC(capi_dcolnorm2(h, m - n, rb, B + n + j * ldb, ldb, colnorm2 + j));
  }
  return CAPI_OK;
}

int capi_dgelsy(capi_handle_t h, int64_t m, int64_t n, int64_t r, double* A, int64_t lda, double* tau, double* F, int64_t ldf, double* tauf, int* jpvt,
                double* Z, int64_t ldz, double* tauz, double* B, int64_t ldb, double rcond, int min_norm, double* colnorm2, int* rank_host) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE(h, n >= 1 && m >= n && n <= CAPI_GEQP3_MAX && r >= 1 && m < (1LL << 31) && r < (1LL << 31), "dims (m >= n >= 1, n <= CAPI_GEQP3_MAX, r >= 1)");
  CAPI_REQUIRE(h, A && tau && F && tauf && jpvt && B && rank_host && lda >= m && ldf >= n && ldb >= m, "operands");
  CAPI_REQUIRE(h, min_norm == 0 || (Z && tauz && ldz >= n), "Z / tauz / ldz >= n (they may be NULL only with min_norm == 0)");
  CAPI_REQUIRE(h, rcond == rcond, "rcond is not a number");
  CAPI_REQUIRE(h, aligned8(A) && aligned8(tau) && aligned8(F) && aligned8(tauf) && aligned8(B) && aligned8(Z) && aligned8(tauz) && aligned8(colnorm2) &&
                      ((uintptr_t)jpvt & 3) == 0, "pointers aligned to 8 bytes (jpvt to 4)");
  RC(capi_dgeqrf(h, m, n, A, lda, tau));
  RC(capi_dormqr(h, CAPI_LEFT, CAPI_TRANS, m, r, n, A, lda, tau, B, ldb));
  RC(capi_dlacpy(h, 1, n, n, A, lda, F, ldf));
  RC(capi_dtrizero(h, CAPI_UPPER, n, F, ldf));
  int k = 0;
  RC(capi_dgeqp3(h, n, n, F, ldf, jpvt, tauf, rcond < 0.0 ? (double)m * 0x1p-52 : rcond, &k));   // the call's synchronisation
  *rank_host = k;
  RC(capi_dormqr(h, CAPI_LEFT, CAPI_TRANS, n, r, k, F, ldf, tauf, B, ldb));
  const bool mn = min_norm != 0 && k < n && k > 0;
  if (mn) {
    hipLaunchKernelGGL(gelsy_transpose_kernel, dim3((unsigned)cdiv(n, 32), (unsigned)cdiv(k, 32)), dim3(256), 0, h->stream, (int)n, k, (const double*)F, ldf, Z, ldz);
    CAPI_HIP_CHECK(h, hipGetLastError());
    RC(capi_dgeqrf(h, n, k, Z, ldz, tauz));
  }
  for (int64_t j = 0; j < r; j += CAPI_TS_MAX_RHS) {
    const int64_t rb = r - j < CAPI_TS_MAX_RHS ? r - j : CAPI_TS_MAX_RHS;
    double* Bj = B + j * ldb;
    if (colnorm2) RC(capi_dcolnorm2(h, m - k, rb, Bj + k, ldb, colnorm2 + j));
    if (k > 0) RC(capi_dtrsm_thin(h, mn ? CAPI_TRANS : CAPI_NOTRANS, k, rb, mn ? Z : F, mn ? ldz : ldf, 0, Bj, ldb));
  }
  if (mn) {
    const unsigned gy = (unsigned)(r < 65535 ? r : 65535);
    hipLaunchKernelGGL(gelsy_zero_rows_kernel, dim3((unsigned)cdiv(n - k, 256), gy), dim3(256), 0, h->stream, (int64_t)k, n, r, B, ldb);
    CAPI_HIP_CHECK(h, hipGetLastError());
    RC(capi_dormqr(h, CAPI_LEFT, CAPI_NOTRANS, n, r, k, Z, ldz, tauz, B, ldb));
  }
  // X = P Y: the scatter must not run in place
  void* pv = nullptr;
  RC(capi_ws_get(h, sizeof(double) * (size_t)n * (size_t)r, &pv));
  RC(capi_drow_scatter(h, 0, mn ? n : k, r, n, B, ldb, jpvt, (double*)pv, n));
  return capi_dlacpy(h, 0, n, r, (const double*)pv, n, B, ldb);
}

}  // extern "C"
