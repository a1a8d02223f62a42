// svd_f64.hip -- the singular value decomposition of an upper triangular R of order n <= 2048 on the device, R = U diag(sigma) V^T: the last step of
// a tall-skinny SVD on the CholeskyQR factors (qr::cacqr::svd: A = Q R = (Q U) Sigma V^T).  Not in the reference: cacqr.hpp stops at Q and R.
//
//   capi_dgesvj   LAPACK's dgesvj for a triangle: one-sided (Hestenes) Jacobi, cyclic sweeps in round-robin order
//
// The columns of M = R^T are rotated until they are orthogonal, M J = V Sigma: the normalised columns are V, their norms sigma, and the accumulated
// rotations J are U (R = J Sigma V^T).  On R^T the sweeps converge in 8 to 14 sweeps up to kappa 1e12; on the columns of R itself they do not within
// 30.  A sweep is the N - 1 steps of jacobi_plan.h, ONE LAUNCH PER STEP and ONE WORKGROUP PER PAIR: the workgroup holds its two columns in
// registers (8 elements a thread at n = 2048), forms a = ||x||^2, b = ||y||^2, c = x^T y -- a thread's elements in order, a butterfly inside the wave,
// the four waves in order -- and rotates when |c| > sqrt(n) 2^-53 sqrt(a) sqrt(b) (dgesvj's criterion), the same rotation on the two columns of J when
// U is wanted.  A pair with a == 0 or b == 0 is skipped; a NaN compares false and rotates nothing.  The rotations of a sweep are counted by an
// integer atomic (order-independent) in a word of the sweep's own, and those 4 bytes are read once per sweep: the first sweep that rotates nothing
// ends the loop, the 30th at the latest, whatever the input holds.  Steps are ordered by kernel boundaries on the handle's stream alone: no
// cooperative launch, no grid barrier, no flag is waited on, no floating-point atomics -- the same bits on every run and on every rank that holds
// the same R.
// Afterwards: column norms, a stable descending sort (NaN first, ties by index: a total order, so the permutation is one whatever the norms hold),
// V's columns divided by their norms, and J polished by one Newton-Schulz step J (1.5 I - 0.5 J^T J) on the tile kernel (capi_dgemm): a column of J
// goes through ~13 n rotations, which leaves ||J^T J - I||_F near 60 u per entry at n = 256; the step brings it to LAPACK's level.
#include "capi_internal.h"
#include "jacobi_plan.h"
#include "thin_tile.h"

namespace {

namespace jp = jacobi_plan;
namespace tt = thin_tile;

constexpr int SV_THREADS = 256;
constexpr int SV_EPT = jp::MAX_N / SV_THREADS;   // elements of a column per thread, at most
static_assert(SV_EPT * SV_THREADS == jp::MAX_N, "a column of the largest order fills the workgroup's registers exactly");

// the four waves' partial sums in order; every thread receives the result.  red: 4 doubles of LDS per call site
__device__ __forceinline__ double ordered_sum(double v, double* red) {
  v = tt::butterfly_sum<64>(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// W <- R^T from R's upper triangle (nothing below R's diagonal is read), J <- I.  One workgroup per column of W
__global__ __launch_bounds__(SV_THREADS) void svd_init_kernel(int n, const double* __restrict__ R, int64_t ldr, double* __restrict__ W, double* __restrict__ J) {
  const int j = blockIdx.x;
  for (int i = threadIdx.x; i < n; i += SV_THREADS) {
    const bool in = i >= j;
    const double v = *(in ? R + j + (int64_t)i * ldr : R);      // R(j, i), an element of the upper triangle
    W[(int64_t)j * n + i] = in ? v : 0.0;
    if (J) J[(int64_t)j * n + i] = i == j ? 1.0 : 0.0;
  }
}

struct StepArgs {
  double* W; double* J;
  int* count;
  int n, step;
  double tol;
};

template <bool ACC>
__global__ __launch_bounds__(SV_THREADS) void jacobi_step_kernel(const StepArgs s) {
  __shared__ double red[3][4];
  int p, q;
  if (!jp::pair_of(s.n, s.step, blockIdx.x, &p, &q)) return;    // (the whole workgroup: an odd n's resting slot)
  const int n = s.n, tid = threadIdx.x;
  double* const xp = s.W + (int64_t)p * n;
  double* const yq = s.W + (int64_t)q * n;
  double x[SV_EPT], y[SV_EPT];
  double a = 0.0, b = 0.0, c = 0.0;
#pragma unroll
  for (int t = 0; t < SV_EPT; ++t) {
    const int i = tid + SV_THREADS * t;
    const bool in = i < n;
    const double xv = *(in ? xp + i : xp), yv = *(in ? yq + i : yq);
    x[t] = in ? xv : 0.0;
    y[t] = in ? yv : 0.0;
    a += x[t] * x[t];
    b += y[t] * y[t];
    c += x[t] * y[t];
  }
  a = ordered_sum(a, red[0]);
  b = ordered_sum(b, red[1]);
  c = ordered_sum(c, red[2]);
  // every thread holds the same a, b, c: the decision is the workgroup's
  if (!(a != 0.0 && b != 0.0 && fabs(c) > s.tol * sqrt(a) * sqrt(b))) return;
  const double zeta = (b - a) / (2.0 * c);
  const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
  for (int u = 0; u < SV_EPT; ++u) {
    const int i = tid + SV_THREADS * u;
    if (i < n) {
      xp[i] = cs * x[u] - sn * y[u];
      yq[i] = sn * x[u] + cs * y[u];
    }
  }
  if (ACC) {
    double* const up = s.J + (int64_t)p * n;
    double* const uq = s.J + (int64_t)q * n;
#pragma unroll
    for (int u = 0; u < SV_EPT; ++u) {
      const int i = tid + SV_THREADS * u;
      if (i < n) {
        const double xv = up[i], yv = uq[i];
        up[i] = cs * xv - sn * yv;
        uq[i] = sn * xv + cs * yv;
      }
    }
  }
  if (tid == 0) atomicAdd(s.count, 1);
}

// norms[j] <- ||W(:, j)||_2.  One workgroup per column
__global__ __launch_bounds__(SV_THREADS) void svd_norms_kernel(int n, const double* __restrict__ W, double* __restrict__ norms) {
  __shared__ double red[4];
  const double* w = W + (int64_t)blockIdx.x * n;
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += SV_THREADS) a += w[i] * w[i];
  a = ordered_sum(a, red);
  if (threadIdx.x == 0) norms[blockIdx.x] = sqrt(a);
}

// (v_j, j) before (v_i, i) in the output: NaN first, then descending, ties by index -- a strict total order for any values
__device__ __forceinline__ bool sorts_before(double vj, int j, double vi, int i) {
  const bool nj = vj != vj, ni = vi != vi;
  if (nj || ni) return nj && (!ni || j < i);
  return vj > vi || (vj == vi && j < i);
}

// perm[k] <- the column that takes place k, sigma[k] <- its norm: a rank sort by one workgroup (n <= 2048: 2^22 comparisons)
__global__ __launch_bounds__(SV_THREADS) void svd_sort_kernel(int n, const double* __restrict__ norms, int* __restrict__ perm, double* __restrict__ sigma) {
  __shared__ double v[jp::MAX_N];
  for (int i = threadIdx.x; i < n; i += SV_THREADS) v[i] = norms[i];
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += SV_THREADS) {
    const double vi = v[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += sorts_before(v[j], j, vi, i) ? 1 : 0;
    perm[rank] = i;                                             // rank < n: the order is total, so the ranks are 0 .. n - 1, each once
    sigma[rank] = vi;
  }
}

// Dst(:, k) <- Src(:, perm[k]) / norms[perm[k]] (norms == NULL: the column as it is; a norm of exactly zero: the column stays zero)
__global__ __launch_bounds__(SV_THREADS) void svd_gather_kernel(int n, const double* __restrict__ Src, const int* __restrict__ perm,
                                                                const double* __restrict__ norms, double* __restrict__ Dst, int64_t ldd) {
  int c = perm[blockIdx.x];
  c = c < 0 ? 0 : (c >= n ? n - 1 : c);
  const double nrm = norms ? norms[c] : 1.0, den = nrm == 0.0 ? 1.0 : nrm;
  const double* src = Src + (int64_t)c * n;
  double* dst = Dst + (int64_t)blockIdx.x * ldd;
  for (int i = threadIdx.x; i < n; i += SV_THREADS) dst[i] = src[i] / den;
}

// T <- 1.5 I - 0.5 T, one workgroup per column
__global__ __launch_bounds__(SV_THREADS) void svd_polish_kernel(int n, double* __restrict__ T) {
  const int j = blockIdx.x;
  for (int i = threadIdx.x; i < n; i += SV_THREADS) T[(int64_t)j * n + i] = (i == j ? 1.5 : 0.0) - 0.5 * T[(int64_t)j * n + i];
}

}  // namespace

extern "C" {

int capi_dgesvj(capi_handle_t h, int64_t n, const double* R, int64_t ldr, double* U, int64_t ldu, double* sigma, double* V, int64_t ldv, int* sweeps_host) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE(h, n >= 1 && n <= jp::MAX_N, "n: 1 <= n <= 2048");
  CAPI_REQUIRE(h, R && ldr >= n && sigma && sweeps_host, "R / ldr >= n / sigma / sweeps_host");
  CAPI_REQUIRE(h, (!U || ldu >= n) && (!V || ldv >= n) && (!U || U != V), "ldu >= n / ldv >= n / U must not alias V");
  const int ni = (int)n;
  const size_t nn = (size_t)n * (size_t)n;
  // W, J (with U), the norms, then the permutation and one counter per sweep
  const size_t doubles = nn * (U ? 2 : 1) + (size_t)n;
  void* pv = nullptr;
  int rc = capi_ws4_get(h, sizeof(double) * doubles + sizeof(int) * ((size_t)n + jp::MAX_SWEEPS), &pv);
  if (rc != CAPI_OK) return rc;
  double* const W = (double*)pv;
  double* const J = U ? W + nn : nullptr;
  double* const norms = W + nn * (U ? 2 : 1);
  int* const perm = (int*)(norms + n);
  int* const count = perm + n;
  CAPI_HIP_CHECK(h, hipMemsetAsync(count, 0, sizeof(int) * jp::MAX_SWEEPS, h->stream));
  hipLaunchKernelGGL(svd_init_kernel, dim3((unsigned)n), dim3(SV_THREADS), 0, h->stream, ni, R, ldr, W, J);
  StepArgs s;
  s.W = W; s.J = J; s.n = ni;
  s.tol = sqrt((double)n) * 0x1p-53;
  const int steps = jp::steps(ni), slots = jp::slots(ni);
  int sweeps = 0;
  bool converged = false;
  while (!converged && sweeps < jp::MAX_SWEEPS) {
    s.count = count + sweeps;
    for (s.step = 0; s.step < steps; ++s.step) {
      if (U) hipLaunchKernelGGL(jacobi_step_kernel<true>, dim3((unsigned)slots), dim3(SV_THREADS), 0, h->stream, s);
      else hipLaunchKernelGGL(jacobi_step_kernel<false>, dim3((unsigned)slots), dim3(SV_THREADS), 0, h->stream, s);
    }
    CAPI_HIP_CHECK(h, hipGetLastError());
    CAPI_HIP_CHECK(h, hipMemcpyAsync(h->h_info, s.count, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    CAPI_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    ++sweeps;
    converged = *h->h_info == 0;
  }
  hipLaunchKernelGGL(svd_norms_kernel, dim3((unsigned)n), dim3(SV_THREADS), 0, h->stream, ni, (const double*)W, norms);
  hipLaunchKernelGGL(svd_sort_kernel, dim3(1), dim3(SV_THREADS), 0, h->stream, ni, (const double*)norms, perm, sigma);
  if (V) hipLaunchKernelGGL(svd_gather_kernel, dim3((unsigned)n), dim3(SV_THREADS), 0, h->stream, ni, (const double*)W, (const int*)perm, (const double*)norms, V, ldv);
  CAPI_HIP_CHECK(h, hipGetLastError());
  if (U) {
    // W is free: it receives J's columns in their final order, J's block the polishing factor
    hipLaunchKernelGGL(svd_gather_kernel, dim3((unsigned)n), dim3(SV_THREADS), 0, h->stream, ni, (const double*)J, (const int*)perm, (const double*)nullptr, W, n);
    CAPI_HIP_CHECK(h, hipGetLastError());
    if ((rc = capi_dgemm(h, CAPI_TRANS, CAPI_NOTRANS, n, n, n, 1.0, W, n, W, n, 0.0, J, n)) != CAPI_OK) return rc;
    hipLaunchKernelGGL(svd_polish_kernel, dim3((unsigned)n), dim3(SV_THREADS), 0, h->stream, ni, J);
    CAPI_HIP_CHECK(h, hipGetLastError());
    if ((rc = capi_dgemm(h, CAPI_NOTRANS, CAPI_NOTRANS, n, n, n, 1.0, W, n, J, n, 0.0, U, ldu)) != CAPI_OK) return rc;
  }
  *sweeps_host = converged ? sweeps : -jp::MAX_SWEEPS;
  return CAPI_OK;
}

}  // extern "C"
