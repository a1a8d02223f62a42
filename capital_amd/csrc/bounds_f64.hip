// bounds_f64.hip -- the elementwise and vector steps of the error bounds of cholesky::cholinv (condition, error_bounds): LAPACK's dporfs / dpocon
// around products that the caller makes with the resident factors.  Not in the reference: its cholinv stops at R and R^-1.
//
//   capi_dberr        berr[j] <- max_i |rho_ij| / w_ij (dporfs's guarded quotient), W <- |rho| + (n + 1) eps W: the weights of the forward bound
//   capi_dcolamax     colmax[j] <- max_i |X(i, j)|
//   capi_dcolnorm2    out[j] <- sum_i X(i, j)^2 (cholinv::quadratic_forms: b^T A^-1 b from R^-T b)
//   capi_dlacn_block  one transition of the Hager-Higham 1-norm estimator (dlacn2) for r columns in lockstep, by reverse communication
//
// One workgroup of 256 threads per column.  A thread takes the lines tid, tid + 256, ..; its partial results meet in a butterfly inside the wave and
// the four waves in order, so sums have one fixed order (the same bits on every run, no atomics) and an argmax is the FIRST maximum.
#include <float.h>

#include "capi_internal.h"
#include "thin_tile.h"

namespace {

namespace tt = thin_tile;

constexpr int BD_THREADS = 256;
constexpr double BD_EPS = 0x1p-53;               // dlamch('E')

// sum / maximum / first argmax over the workgroup; every thread receives the result.  red: 4 doubles (+ 4 ints) of LDS
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = tt::butterfly_sum<64>(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ double block_max(double v, double* red) {
  v = tt::butterfly_max<64>(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return tt::max_nan(tt::max_nan(tt::max_nan(red[0], red[1]), red[2]), red[3]);
}
// (a, i) against (b, k): the larger value, of equal values the smaller index
__device__ __forceinline__ void first_max(double& a, int64_t& i, double b, int64_t k) {
  if (b > a || (b == a && k < i)) { a = b; i = k; }
}
__device__ __forceinline__ int64_t block_argmax(double v, int64_t i, double* red, int64_t* redi, double* vmax) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double b = __shfl_xor(v, d);
    const int64_t k = __shfl_xor((long long)i, d);
    first_max(v, i, b, k);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = v; redi[threadIdx.x >> 6] = i; }
  __syncthreads();
  v = red[0]; i = redi[0];
  for (int w = 1; w < 4; ++w) first_max(v, i, red[w], redi[w]);
  *vmax = v;
  return i;
}

__global__ __launch_bounds__(BD_THREADS) void berr_kernel(int64_t n, const double* __restrict__ Rho, int64_t ldr, double* __restrict__ W, int64_t ldw,
                                                          double* __restrict__ berr) {
  __shared__ double red[4];
  const double* rho = Rho + (int64_t)blockIdx.x * ldr;
  double* w = W + (int64_t)blockIdx.x * ldw;
  const double nz = (double)(n + 1), safe1 = nz * DBL_MIN, safe2 = safe1 / BD_EPS, nzeps = nz * BD_EPS;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += BD_THREADS) {
    const double a = fabs(rho[i]), wi = w[i];
    const bool big = wi > safe2;
    s = tt::max_nan(s, big ? a / wi : (a + safe1) / (wi + safe1));
    const double t = a + nzeps * wi;
    w[i] = big ? t : t + safe1;
  }
  s = block_max(s, red);
  if (threadIdx.x == 0) berr[blockIdx.x] = s;
}

__global__ __launch_bounds__(BD_THREADS) void colamax_kernel(int64_t n, const double* __restrict__ X, int64_t ldx, double* __restrict__ colmax) {
  __shared__ double red[4];
  const double* x = X + (int64_t)blockIdx.x * ldx;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += BD_THREADS) s = tt::max_nan(s, fabs(x[i]));
  s = block_max(s, red);
  if (threadIdx.x == 0) colmax[blockIdx.x] = s;
}

__global__ __launch_bounds__(BD_THREADS) void colnorm2_kernel(int64_t n, const double* __restrict__ X, int64_t ldx, double* __restrict__ out) {
  __shared__ double red[4];
  const double* x = X + (int64_t)blockIdx.x * ldx;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += BD_THREADS) s += x[i] * x[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// ---- the estimator.  Per column the state is LACN_HEAD doubles and the n signs of dlacn2's ISGN; behind the r columns lie the words of the count ----
constexpr int LACN_HEAD = 8;                     // stage, iter, j, jlast, est, applies, 2 spare
constexpr int LACN_MAX_APPLIES = 11;             // 1 + 1 + 2 * 4 + 1: iter runs from 2 to ITMAX = 5
enum { ST_DONE = 0, ST_FIRST = 1, ST_ARGMAX0 = 2, ST_NORM = 3, ST_ARGMAX = 4, ST_ALT = 5 };
constexpr int LACN_ITMAX = 5;

__host__ __device__ inline int64_t lacn_col_doubles(int64_t n) { return n + LACN_HEAD; }

// X holds, for a call with init == 0, A^-1 times what the call before left there.  The stages name what that product is (dlacn2's JUMP):
//   ST_FIRST    of x = 1/n                      est = ||x||_1, x <- sign(x)
//   ST_ARGMAX0  of the signs                    j = argmax |x|, x <- e_j
//   ST_NORM     of e_j                          est = ||x||_1; signs as before, or est no larger: the last stage; else x <- sign(x)
//   ST_ARGMAX   of the signs                    a new j (at most ITMAX rounds): x <- e_j; else the last stage
//   ST_ALT      of x_i = (-1)^i (1 + i/(n-1))   est = max(est, 2 ||x||_1 / (3 n)): finished
// With weights (dporfs) the operator is diag(w) A^-1: products of ST_FIRST, ST_NORM and ST_ALT (dlacn2's KASE 1) are multiplied by w as they are
// read, the sign vectors (KASE 2, the transposed operator A^-1 diag(w)) as they are written.
__global__ __launch_bounds__(BD_THREADS) void lacn_step_kernel(int init, int64_t n, double* __restrict__ X, int64_t ldx, const double* __restrict__ Wt,
                                                               int64_t ldw, double* __restrict__ state, double* __restrict__ est) {
  __shared__ double red[4];
  __shared__ int64_t redi[4];
  const int tid = threadIdx.x;
  double* x = X + (int64_t)blockIdx.x * ldx;
  const double* w = Wt ? Wt + (int64_t)blockIdx.x * ldw : nullptr;
  double* st = state + (int64_t)blockIdx.x * lacn_col_doubles(n);
  double* isgn = st + LACN_HEAD;
  if (init) {
    for (int64_t i = tid; i < n; i += BD_THREADS) x[i] = 1.0 / (double)n;
    if (tid == 0) { st[0] = ST_FIRST; st[1] = 0.0; st[2] = 0.0; st[3] = 0.0; st[4] = 0.0; st[5] = 0.0; }
    return;
  }
  const int stage = (int)st[0];
  if (stage == ST_DONE) return;                                  // frozen: x is zero and stays zero under the caller's product
  int iter = (int)st[1];
  int64_t j = (int64_t)st[2], jlast = (int64_t)st[3];
  double e = st[4];
  const double applies = st[5] + 1.0;
  __syncthreads();                                               // every thread has read the head before thread 0 rewrites it
  auto kase1 = [&](int64_t i) { return w ? x[i] * w[i] : x[i]; };
  auto sgn = [](double v) { return v >= 0.0 ? 1.0 : -1.0; };     // sign(0) = +1
  int next = ST_DONE;
  bool to_alt = false;
  if (!(applies <= (double)LACN_MAX_APPLIES) || stage < ST_FIRST || stage > ST_ALT || j < 0 || j >= n) {
    next = -1;                                                   // no state of this estimator (iter <= ITMAX allows 11 products): the host reports it
    j = 0;
  } else if (stage == ST_FIRST) {
    double s = 0.0;
    for (int64_t i = tid; i < n; i += BD_THREADS) s += fabs(kase1(i));
    e = block_sum(s, red);
    if (n > 1) {
      for (int64_t i = tid; i < n; i += BD_THREADS) {
        const double sg = sgn(kase1(i));
        isgn[i] = sg;
        x[i] = w ? sg * w[i] : sg;
      }
      next = ST_ARGMAX0;
    }
  } else if (stage == ST_ARGMAX0 || stage == ST_ARGMAX) {
    double v = -1.0, vmax;
    int64_t k = n;
    for (int64_t i = tid; i < n; i += BD_THREADS) first_max(v, k, fabs(x[i]), i);
    const int64_t jn = block_argmax(v, k, red, redi, &vmax);
    const int64_t jc = jn < n ? jn : 0;                          // (all NaN: no maximum)
    bool again = true;
    if (stage == ST_ARGMAX) {
      again = fabs(x[j]) != fabs(x[jc]) && iter < LACN_ITMAX;
      jlast = j;
      if (again) ++iter;
    } else {
      iter = 2;
    }
    j = jc;
    __syncthreads();                                             // x[jlast], x[j] are read by all before anyone overwrites x
    if (again) {
      for (int64_t i = tid; i < n; i += BD_THREADS) x[i] = i == j ? 1.0 : 0.0;
      next = ST_NORM;
    } else {
      to_alt = true;
    }
  } else if (stage == ST_NORM) {
    double s = 0.0, differ = 0.0;
    for (int64_t i = tid; i < n; i += BD_THREADS) {
      const double v = kase1(i);
      s += fabs(v);
      differ += sgn(v) != isgn[i] ? 1.0 : 0.0;
    }
    const double eold = e;
    e = block_sum(s, red);
    differ = block_sum(differ, red);
    if (differ == 0.0 || e <= eold) {
      to_alt = true;
    } else {
      for (int64_t i = tid; i < n; i += BD_THREADS) {
        const double sg = sgn(kase1(i));
        isgn[i] = sg;
        x[i] = w ? sg * w[i] : sg;
      }
      next = ST_ARGMAX;
    }
  } else {                                                       // ST_ALT
    double s = 0.0;
    for (int64_t i = tid; i < n; i += BD_THREADS) s += fabs(kase1(i));
    const double t = 2.0 * (block_sum(s, red) / (double)(3 * n));
    if (t > e) e = t;
  }
  if (to_alt) {
    for (int64_t i = tid; i < n; i += BD_THREADS) x[i] = ((i & 1) ? -1.0 : 1.0) * (1.0 + (double)i / (double)(n - 1));
    next = ST_ALT;
  }
  if (next == ST_DONE)
    for (int64_t i = tid; i < n; i += BD_THREADS) x[i] = 0.0;
  if (tid == 0) {
    st[0] = next; st[1] = iter; st[2] = (double)j; st[3] = (double)jlast; st[4] = e; st[5] = applies;
    if (next == ST_DONE) est[blockIdx.x] = e;
  }
}

// *count = the columns that are not finished, or -1 when a column's state is out of the protocol
__global__ __launch_bounds__(64) void lacn_count_kernel(int64_t n, int r, const double* __restrict__ state, int* __restrict__ count) {
  if (threadIdx.x != 0) return;
  int c = 0;
  bool bad = false;
  for (int k = 0; k < r; ++k) {
    const double s = state[(int64_t)k * lacn_col_doubles(n)];
    bad = bad || !(s >= 0.0 && s <= (double)ST_ALT);
    c += s != (double)ST_DONE;
  }
  *count = bad ? -1 : c;
}

}  // namespace

extern "C" {

int capi_dberr(capi_handle_t h, int64_t n, int64_t r, const double* Rho, int64_t ldr, double* W, int64_t ldw, double* berr) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE_THIN_R(h, r);
  CAPI_REQUIRE(h, n >= 0 && berr && (n == 0 || (Rho && W && ldr >= n && ldw >= n)), "n/Rho/ldr/W/ldw/berr");
  CAPI_REQUIRE(h, n == 0 || Rho != W, "W must not alias Rho");
  hipLaunchKernelGGL(berr_kernel, dim3((unsigned)r), dim3(BD_THREADS), 0, h->stream, n, Rho, ldr, W, ldw, berr);
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

int capi_dcolamax(capi_handle_t h, int64_t n, int64_t r, const double* X, int64_t ldx, double* colmax) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE_THIN_R(h, r);
  CAPI_REQUIRE(h, n >= 0 && colmax && (n == 0 || (X && ldx >= n)), "n/X/ldx/colmax");
  hipLaunchKernelGGL(colamax_kernel, dim3((unsigned)r), dim3(BD_THREADS), 0, h->stream, n, X, ldx, colmax);
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

int capi_dcolnorm2(capi_handle_t h, int64_t n, int64_t r, const double* X, int64_t ldx, double* out) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE_THIN_R(h, r);
  CAPI_REQUIRE(h, n >= 0 && out && (n == 0 || (X && ldx >= n)), "n/X/ldx/out");
  hipLaunchKernelGGL(colnorm2_kernel, dim3((unsigned)r), dim3(BD_THREADS), 0, h->stream, n, X, ldx, out);
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

size_t capi_dlacn_state_bytes(int64_t n, int64_t r) {
  if (n < 1 || r < 1 || r > CAPI_TS_MAX_RHS) return 0;
  return sizeof(double) * (size_t)(r * lacn_col_doubles(n) + 1);
}

int capi_dlacn_block(capi_handle_t h, int init, int64_t n, int64_t r, double* X, int64_t ldx, const double* Wt, int64_t ldw, double* state, double* est,
                     int* active_host) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE_THIN_R(h, r);
  CAPI_REQUIRE(h, n >= 1 && X && ldx >= n && (!Wt || ldw >= n) && state && est && active_host, "n >= 1/X/ldx/Wt/ldw/state/est/active_host");
  int* count = (int*)(state + r * lacn_col_doubles(n));
  hipLaunchKernelGGL(lacn_step_kernel, dim3((unsigned)r), dim3(BD_THREADS), 0, h->stream, init, n, X, ldx, Wt, ldw, state, est);
  hipLaunchKernelGGL(lacn_count_kernel, dim3(1), dim3(64), 0, h->stream, n, (int)r, (const double*)state, count);
  CAPI_HIP_CHECK(h, hipGetLastError());
  CAPI_HIP_CHECK(h, hipMemcpyAsync(h->h_info, count, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  CAPI_HIP_CHECK(h, hipStreamSynchronize(h->stream));
  *active_host = *h->h_info;
  CAPI_REQUIRE(h, *active_host >= 0, "state: a column is outside the protocol (more than 11 products, or not a state of this estimator)");
  return CAPI_OK;
}

}  // extern "C"
