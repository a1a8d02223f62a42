// pstrf_f64.hip -- Cholesky with complete (diagonal) pivoting of a Gram matrix of order n <= 2048 on the device, P^T G P = R^T R + diag-block(0, S): the
// rank-revealing step of a column-pivoted CholeskyQR (qr::cacqr::factor_pivoted).  Not in the reference: cacqr.hpp stops at Q and R.
//
//   capi_dpstrf         LAPACK's dpstrf (upper), stopping where the largest remaining diagonal entry is <= tol * trace(G)
//   capi_drow_scatter   D <- 0, D(piv[i], :) <- S(i, :): the permutation applied to the rows of a (triangular) block
//
// dpstrf's blocked, lazy scheme with panels of 32 columns: ONE WORKGROUP PER PANEL (up to 1024 threads, a thread owns the same <= 2 columns through
// the whole panel) and one trailing update per panel through capi_dsyrk (UPPER, TRANS, k = 32: G22 -= R_strip^T R_strip, the two regions disjoint).
// Per step j the panel workgroup
//   - takes the updated diagonal d_i = g_ii - dots_i of the remaining columns (g_ii as the last trailing update left it, dots_i the squares of this
//     panel's rows of R, both in LDS) and the FIRST index p of its maximum (a NaN counts as -inf): a butterfly inside the wave, the waves in order,
//     under a total order on (value, index) so that the result does not depend on how the candidates meet;
//   - stops unless d_p > thresh (a NaN compares false and stops): the rank j goes to a device word with a flag, the unfinished rows of the strip are
//     zeroed so that the trailing update subtracts nothing for them, and every later panel kernel reads the flag at entry and returns;
//   - swaps j and p in upper storage: the column parts above, the row parts to the right, the transposed middle piece, the diagonal, dots and piv --
//     the column parts include the rows of R that earlier panels computed;
//   - computes row j of R: r_ji = (g_ji - sum_l r_lj r_li) / sqrt(d_p) over this panel's rows l < j, l ascending.
// All ceil(n / 32) rounds are enqueued without a host round trip; steps are ordered by kernel boundaries on the handle's stream and by workgroup
// barriers inside a panel alone: no cooperative launch, no device-side waiting, no flag that anyone spins on, no atomics.  Sums have a fixed order,
// so every result is bit-identical from run to run and on every device that holds the same G.  Every loop has a trip count fixed by n: non-finite
// input ends the call like any other, with 0 <= rank <= n and piv a permutation (piv only ever changes by swaps).
#include <math.h>

#include "capi_internal.h"
#include "thin_tile.h"

namespace {

namespace tt = thin_tile;

constexpr int PS_NB = 32;            // columns of a panel
constexpr int PS_MAX_N = 2048;
constexpr int PS_MAX_THREADS = 1024;
constexpr int PS_INIT_THREADS = 256;

struct PsState {
  double thresh;    // tol * trace(G)
  int stopped;      // a panel met a pivot <= thresh
  int rank;
};

// piv <- identity, state <- (tol * trace(G), not stopped, rank n).  One workgroup: a thread's diagonal entries in order, a butterfly inside the wave,
// the four waves in order
__global__ __launch_bounds__(PS_INIT_THREADS) void pstrf_init_kernel(int n, const double* __restrict__ G, int64_t ldg, double tol, int* __restrict__ piv,
                                                                     PsState* __restrict__ st) {
  __shared__ double red[4];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += PS_INIT_THREADS) {
    piv[i] = i;
    a += G[i + (int64_t)i * ldg];
  }
  a = tt::butterfly_sum<64>(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    st->thresh = tol * (((red[0] + red[1]) + red[2]) + red[3]);
    st->stopped = 0;
    st->rank = n;
  }
}

// (av, ai) before (bv, bi): the larger value, ties to the smaller index -- a strict total order (no NaN reaches it)
__device__ __forceinline__ bool pivots_before(double av, int ai, double bv, int bi) { return av > bv || (av == bv && ai < bi); }

// columns k0 .. min(k0 + 32, n) - 1: see the file comment.  blockDim.x is a multiple of 64, <= 1024
__global__ __launch_bounds__(PS_MAX_THREADS) void pstrf_panel_kernel(int n, int k0, double* __restrict__ G, int64_t ldg, int* __restrict__ piv,
                                                                     PsState* __restrict__ st) {
  __shared__ double dg[PS_MAX_N];      // g_ii of the trailing block as the last update left it, permuted with the columns
  __shared__ double dots[PS_MAX_N];    // what this panel's rows of R have taken from it
  __shared__ double cj[PS_NB];         // this panel's rows of column j
  __shared__ double redv[PS_MAX_THREADS / 64];
  __shared__ int redi[PS_MAX_THREADS / 64];
  __shared__ int stopped;
  const int tid = threadIdx.x, T = blockDim.x, nw = T >> 6;
  if (tid == 0) stopped = st->stopped;
  __syncthreads();
  if (stopped) return;                                                      // (the whole workgroup)
  const int kend = k0 + PS_NB < n ? k0 + PS_NB : n;
  const double thresh = st->thresh;
  for (int i = k0 + tid; i < n; i += T) {
    dg[i] = G[i + (int64_t)i * ldg];
    dots[i] = 0.0;
  }
  for (int j = k0; j < kend; ++j) {
    // the first maximum of the updated diagonal over j .. n - 1 (an entry is read by the thread that owns, and wrote, it)
    double bv = -INFINITY;
    int bi = n;
    for (int i = k0 + tid; i < n; i += T) {
      if (i < j) continue;
      double w = dg[i] - dots[i];
      w = w == w ? w : -INFINITY;
      if (pivots_before(w, i, bv, bi)) { bv = w; bi = i; }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double ov = __shfl_xor(bv, d);
      const int oi = __shfl_xor(bi, d);
      if (pivots_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if ((tid & 63) == 0) { redv[tid >> 6] = bv; redi[tid >> 6] = bi; }
    __syncthreads();
    bv = redv[0];
    bi = redi[0];
    for (int w = 1; w < nw; ++w)
      if (pivots_before(redv[w], redi[w], bv, bi)) { bv = redv[w]; bi = redi[w]; }
    // every thread holds the same (bv, bi), j <= bi < n (column j itself is a candidate): the decision is the workgroup's
    const int p = bi;
    if (!(bv > thresh) || p >= n) {
      for (int i = kend + tid; i < n; i += T)
        for (int l = j; l < kend; ++l) G[l + (int64_t)i * ldg] = 0.0;
      if (tid == 0) { st->rank = j; st->stopped = 1; }
      return;
    }
    if (p != j) {
      for (int l = tid; l < n; l += T) {
        if (l == j || l == p) continue;
        double *a, *b;
        if (l < j) { a = G + l + (int64_t)j * ldg; b = G + l + (int64_t)p * ldg; }            // the column parts above
        else if (l < p) { a = G + j + (int64_t)l * ldg; b = G + l + (int64_t)p * ldg; }       // the transposed middle piece
        else { a = G + j + (int64_t)l * ldg; b = G + p + (int64_t)l * ldg; }                  // the row parts to the right
        const double t = *a;
        *a = *b;
        *b = t;
      }
      if (tid == 0) {
        const int t = piv[j];
        piv[j] = piv[p];
        piv[p] = t;
        const double dj = dg[j], oj = dots[j];
        dg[p] = dj;                                                         // (dg[j] and dots[j] are not read again)
        dots[p] = oj;
        G[p + (int64_t)p * ldg] = dj;                                       // the trailing update reads the diagonal from memory
      }
    }
    __syncthreads();
    const int done = j - k0;
    if (tid < done) cj[tid] = G[k0 + tid + (int64_t)j * ldg];
    __syncthreads();
    const double ajj = sqrt(bv);
    if (tid == 0) G[j + (int64_t)j * ldg] = ajj;
    for (int i = k0 + tid; i < n; i += T) {
      if (i <= j) continue;
      double* const col = G + k0 + (int64_t)i * ldg;
      double s = col[done];
      for (int l = 0; l < done; ++l) s -= cj[l] * col[l];
      s /= ajj;
      col[done] = s;
      dots[i] += s * s;
    }
    __syncthreads();
  }
}

__global__ void scatter_zero_kernel(int64_t n, int64_t ncols, double* __restrict__ D, int64_t ldd) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int64_t c = blockIdx.y; c < ncols; c += gridDim.y) D[i + c * ldd] = 0.0;
}

// D(piv[i], :) <- S(i, :), i < k; tri: the entries left of S's diagonal count as zero and are not read.  A piv[i] outside 0 .. n - 1 writes nothing
__global__ void row_scatter_kernel(int tri, int64_t k, int64_t ncols, int64_t n, const double* __restrict__ S, int64_t lds_, const int* __restrict__ piv,
                                   double* __restrict__ D, int64_t ldd) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int64_t row = piv[i];
  if (row < 0 || row >= n) return;
  for (int64_t c = blockIdx.y; c < ncols; c += gridDim.y) {
    const bool in = !tri || c >= i;
    const double v = *(in ? S + i + c * lds_ : S);
    D[row + c * ldd] = in ? v : 0.0;
  }
}

}  // namespace

extern "C" {

int capi_dpstrf(capi_handle_t h, int64_t n, double* G, int64_t ldg, double tol, int* piv, int* rank_host) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE(h, n >= 1 && n <= PS_MAX_N, "n: 1 <= n <= 2048");
  CAPI_REQUIRE(h, G && ldg >= n && piv && rank_host, "G / ldg >= n / piv / rank_host");
  CAPI_REQUIRE(h, tol >= 0.0, "tol >= 0");
  void* pv = nullptr;
  int rc = capi_ws4_get(h, sizeof(PsState), &pv);
  if (rc != CAPI_OK) return rc;
  PsState* const st = (PsState*)pv;
  const int ni = (int)n;
  hipLaunchKernelGGL(pstrf_init_kernel, dim3(1), dim3(PS_INIT_THREADS), 0, h->stream, ni, (const double*)G, ldg, tol, piv, st);
  CAPI_HIP_CHECK(h, hipGetLastError());
  for (int64_t k0 = 0; k0 < n; k0 += PS_NB) {
    const int64_t rest = n - k0, k1 = k0 + PS_NB;
    const int threads = (int)(rest >= PS_MAX_THREADS ? PS_MAX_THREADS : cdiv(rest, 64) * 64);
    hipLaunchKernelGGL(pstrf_panel_kernel, dim3(1), dim3(threads), 0, h->stream, ni, (int)k0, G, ldg, piv, st);
    CAPI_HIP_CHECK(h, hipGetLastError());
    if (k1 < n && (rc = capi_dsyrk(h, CAPI_UPPER, CAPI_TRANS, n - k1, PS_NB, -1.0, G + k0 + k1 * ldg, ldg, 1.0, G + k1 + k1 * ldg, ldg)) != CAPI_OK) return rc;
  }
  CAPI_HIP_CHECK(h, hipMemcpyAsync(h->h_info, &st->rank, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  CAPI_HIP_CHECK(h, hipStreamSynchronize(h->stream));
  *rank_host = *h->h_info;
  return CAPI_OK;
}

int capi_drow_scatter(capi_handle_t h, int tri, int64_t k, int64_t ncols, int64_t n, const double* S, int64_t lds, const int* piv, double* D, int64_t ldd) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE(h, (tri == 0 || tri == 1) && n >= 0 && n < (1LL << 31) && k >= 0 && k <= n && ncols >= 0 && ncols < (1LL << 31), "tri / 0 <= k <= n / ncols");
  if (n == 0 || ncols == 0) return CAPI_OK;
  CAPI_REQUIRE(h, D && ldd >= n, "D / ldd >= n");
  CAPI_REQUIRE(h, k == 0 || (S && lds >= k && piv && (const double*)D != S), "S / lds >= k / piv / D must not alias S");
  const unsigned gy = (unsigned)(ncols < 65535 ? ncols : 65535);
  hipLaunchKernelGGL(scatter_zero_kernel, dim3((unsigned)cdiv(n, 256), gy), dim3(256), 0, h->stream, n, ncols, D, ldd);
  if (k > 0) hipLaunchKernelGGL(row_scatter_kernel, dim3((unsigned)cdiv(k, 256), gy), dim3(256), 0, h->stream, tri, k, ncols, n, S, lds, piv, D, ldd);
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

}  // extern "C"
