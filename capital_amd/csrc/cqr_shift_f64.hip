// cqr_shift_f64.hip -- the n x n steps of a SHIFTED CholeskyQR sweep (qr::cacqr, num_shifted > 0): between the Gram matrix's
// all-reduce and capi_dpotrf_trtri, and behind it.  The reference's sweep (src/alg/qr/cacqr/cacqr.hpp:7-29) has no shift: its
// CholeskyQR2 breaks down beyond kappa(A) ~ 1e8.  Shifted CholeskyQR (Fukaya, Kannan, Nakatsukasa, Yamamoto, Yanagisawa, SIAM J. Sci.
// Comput. 42 (2020)) adds s I to the Gram matrix of the leading sweeps; here the shift is taken on the column-equilibrated Gram matrix
// G' = D^-1 G D^-1, D = diag(2^e_j), so that it is relative to every column's own norm.
//
//   capi_dgram_equilibrate_shift   diag/trace in ONE workgroup (fixed summation order: the same bits on every rank), then the scaling
//   capi_dtri_rescale              the 1- and infinity-norms of the unscaled triangles, one workgroup per column and row, then the scaling, whose
//                                  first workgroup closes the record
// Four small launches per shifted sweep on the handle's stream, no host round trip.  Every scaling is a v_ldexp_f64 by an integer
// exponent: exact, and exactly equivariant under power-of-two column scalings of A.
#include <limits.h>
#include <math.h>
#include "capi_internal.h"

namespace {

constexpr int CS_T = 256;

__device__ __forceinline__ double cs_block_sum(double v, double* red) {   // sum over the workgroup, fixed order
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = CS_T / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}
__device__ __forceinline__ int cs_block_min(int v, int* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = CS_T / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = min(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  const int r = red[0];
  __syncthreads();
  return r;
}

// one workgroup: e_j = floor(exponent(g_jj) / 2) (frexp convention: g = f 2^ex, f in [0.5, 1)), dscale[j] = 2^e_j,
// trace(G') = sum_j g_jj 2^(-2 e_j) (every term in [0.5, 2)), rec[0] = s = factor * trace(G'), rec[1] = trace(G')
__global__ __launch_bounds__(CS_T) void cs_diag_kernel(const double* __restrict__ G, int64_t ldg, int n, double factor,
                                                       double* __restrict__ dscale, double* __restrict__ rec, int* info) {
  __shared__ double red[CS_T];
  __shared__ int redi[CS_T];
  double tr = 0.0;
  int bad = INT_MAX;
  for (int j = threadIdx.x; j < n; j += CS_T) {
    const double g = G[j + (int64_t)j * ldg];
    if (!(g > 0.0) || isinf(g)) {                            // zero, negative, NaN, Inf: a failed pivot; the column stays unscaled
      bad = min(bad, j + 1);
      dscale[j] = 1.0;
      continue;
    }
    int ex;
    (void)frexp(g, &ex);
    const int e = (ex - (ex & 1)) / 2;                        // floor(ex / 2), also for negative ex
    dscale[j] = ldexp(1.0, e);                                // |e| <= 537: always a normal number
    tr += ldexp(g, -2 * e);
  }
  tr = cs_block_sum(tr, red);
  bad = cs_block_min(bad, redi);
  if (threadIdx.x == 0) {
    rec[0] = factor * tr;
    rec[1] = tr;
    if (bad != INT_MAX) atomicCAS(info, 0, bad);              // first failure wins, as in potrf
  }
}

// G'_ij = g_ij 2^-(e_i + e_j) on the upper triangle, + s on the diagonal
__global__ __launch_bounds__(CS_T) void cs_scale_kernel(double* __restrict__ G, int64_t ldg, int n, const double* __restrict__ dscale,
                                                        const double* __restrict__ rec) {
  const int i = blockIdx.x * CS_T + threadIdx.x;
  for (int j = blockIdx.y; j < n; j += gridDim.y) {
    if (i > j) continue;
    const int e = ilogb(dscale[i]) + ilogb(dscale[j]);
    double v = ldexp(G[i + (int64_t)j * ldg], -e);
    if (i == j) v += rec[0];
    G[i + (int64_t)j * ldg] = v;
  }
}

__device__ __forceinline__ double cs_block_max(double v, double* red) {   // a NaN wins: a failed factorisation must not report a finite bound
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = CS_T / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { const double a = red[threadIdx.x], c = red[threadIdx.x + o]; red[threadIdx.x] = (a > c || a != a) ? a : c; }
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// workgroup b, on the UNSCALED triangles (read only): part[5 b ..] = sum_i |R'_ib|, sum_j |R'_bj|, sum_i |X'_ib|, sum_j |X'_bj| (column and row b,
// fixed order), and whether r_bb 2^e_b or x_bb 2^-e_b would leave the normal range of fp64
__global__ __launch_bounds__(CS_T) void cs_norms_kernel(const double* __restrict__ R, int64_t ldr, const double* __restrict__ X, int64_t ldx, int n,
                                                        const double* __restrict__ dscale, double* __restrict__ part) {
  __shared__ double red[CS_T];
  for (int b = blockIdx.x; b < n; b += gridDim.x) {
    double cr = 0.0, cx = 0.0, rr = 0.0, rx = 0.0;
    for (int i = threadIdx.x; i <= b; i += CS_T) { cr += fabs(R[i + (int64_t)b * ldr]); cx += fabs(X[i + (int64_t)b * ldx]); }
    for (int j = b + threadIdx.x; j < n; j += CS_T) { rr += fabs(R[b + (int64_t)j * ldr]); rx += fabs(X[b + (int64_t)j * ldx]); }
    cr = cs_block_sum(cr, red);
    rr = cs_block_sum(rr, red);
    cx = cs_block_sum(cx, red);
    rx = cs_block_sum(rx, red);
    if (threadIdx.x == 0) {
      double* p = part + 5 * (int64_t)b;
      p[0] = cr; p[1] = rr; p[2] = cx; p[3] = rx;
      p[4] = 0.0;
      if (dscale) {
        const int e = ilogb(dscale[b]);
        if (!isnormal(ldexp(R[b + (int64_t)b * ldr], e)) || !isnormal(ldexp(X[b + (int64_t)b * ldx], -e))) p[4] = 1.0;
      }
    }
  }
}

// column j: R_ij = R'_ij 2^e_j, X_ij = X'_ij 2^-e_i (i <= j; dscale == nullptr: nothing is scaled, one workgroup).  Workgroup 0 also closes the
// record: rec[2] = ||R'||_1 ||R'||_inf, rec[3] = ||X'||_1 ||X'||_inf from the shares of cs_norms_kernel
__global__ __launch_bounds__(CS_T) void cs_rescale_kernel(double* __restrict__ R, int64_t ldr, double* __restrict__ X, int64_t ldx, int n,
                                                          const double* __restrict__ dscale, const double* __restrict__ part, double* __restrict__ rec,
                                                          int* info) {
  __shared__ double red[CS_T];
  __shared__ int redi[CS_T];
  if (blockIdx.x == 0) {
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
    int bad = INT_MAX;
    for (int b = threadIdx.x; b < n; b += CS_T) {
      const double* p = part + 5 * (int64_t)b;
      m0 = (p[0] > m0 || p[0] != p[0]) ? p[0] : m0;
      m1 = (p[1] > m1 || p[1] != p[1]) ? p[1] : m1;
      m2 = (p[2] > m2 || p[2] != p[2]) ? p[2] : m2;
      m3 = (p[3] > m3 || p[3] != p[3]) ? p[3] : m3;
      if (p[4] != 0.0) bad = min(bad, b + 1);
    }
    m0 = cs_block_max(m0, red);
    m1 = cs_block_max(m1, red);
    m2 = cs_block_max(m2, red);
    m3 = cs_block_max(m3, red);
    bad = cs_block_min(bad, redi);
    if (threadIdx.x == 0) {
      rec[2] = m0 * m1;
      rec[3] = m2 * m3;
      if (bad != INT_MAX) atomicCAS(info, 0, bad);
    }
  }
  if (!dscale) return;
  for (int j = blockIdx.x; j < n; j += gridDim.x) {
    const int ej = ilogb(dscale[j]);
    for (int i = threadIdx.x; i <= j; i += CS_T) {
      R[i + (int64_t)j * ldr] = ldexp(R[i + (int64_t)j * ldr], ej);
      X[i + (int64_t)j * ldx] = ldexp(X[i + (int64_t)j * ldx], -ilogb(dscale[i]));
    }
  }
}

}  // namespace

extern "C" {

int capi_dgram_equilibrate_shift(capi_handle_t h, int64_t n, double* G, int64_t ldg, int64_t m_global, double shift_scale, double* dscale,
                                 double* rec) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE(h, n >= 0 && n < (1LL << 30) && m_global >= 0 && shift_scale >= 0.0 && shift_scale <= 1.79e308, "n / m_global / shift_scale");
  if (n == 0) return CAPI_OK;
  CAPI_REQUIRE(h, G && dscale && rec && ldg >= n, "G/ldg/dscale/rec");
  // s = factor * trace(G'), factor = shift_scale * 11 (m n + n (n + 1)) u, u = 2^-53
  const double factor = shift_scale * (11.0 * ((double)m_global * (double)n + (double)n * (double)(n + 1)) * 0x1p-53);
  hipLaunchKernelGGL(cs_diag_kernel, dim3(1), dim3(CS_T), 0, h->stream, G, ldg, (int)n, factor, dscale, rec, h->d_info);
  hipLaunchKernelGGL(cs_scale_kernel, dim3((unsigned)cdiv(n, CS_T), (unsigned)(n < 65535 ? n : 65535)), dim3(CS_T), 0, h->stream, G, ldg, (int)n,
                     dscale, rec);
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

int capi_dtri_rescale(capi_handle_t h, int64_t n, double* R, int64_t ldr, double* Rinv, int64_t ldi, const double* dscale, double* rec) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE(h, n >= 0 && n < (1LL << 30), "n");
  if (n == 0) return CAPI_OK;
  CAPI_REQUIRE(h, R && Rinv && rec && ldr >= n && ldi >= n, "R/ldr/Rinv/ldi/rec");   // dscale == NULL: D = I, the norms alone
  void* pv = nullptr;
  int rc = capi_ws_get(h, sizeof(double) * 5 * (size_t)n, &pv);
  if (rc != CAPI_OK) return rc;
  double* part = (double*)pv;
  const unsigned grid = (unsigned)(n < 65535 ? n : 65535);
  hipLaunchKernelGGL(cs_norms_kernel, dim3(grid), dim3(CS_T), 0, h->stream, R, ldr, Rinv, ldi, (int)n, dscale, part);
  hipLaunchKernelGGL(cs_rescale_kernel, dim3(dscale ? grid : 1u), dim3(CS_T), 0, h->stream, R, ldr, Rinv, ldi, (int)n, dscale, part, rec, h->d_info);
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

}  // extern "C"
