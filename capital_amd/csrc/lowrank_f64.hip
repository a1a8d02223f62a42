// lowrank_f64.hip -- the diagonal pieces of the low-rank-plus-diagonal operator M = L L^T + D on the pivoted partial Cholesky factor
// (cholesky::cholinv::lowrank_prepare / lowrank_solve / lowrank_quadratic_forms): Woodbury's identity with the k x k capacitance matrix
// C = I + L^T D^-1 L.  Not in the reference: cholinv.hpp stops at R and R^-1.
//
//   capi_dlr_diag   d_i <- (shift + diag_i) + schur_i; rec <- sum log d_i, min d, max d, first entry that is not a finite number > 0
//   capi_drow_pow   Y <- alpha diag(d)^power X + beta Y, power +1, -1 or -1/2, on an m x r block of any width; the squared column norms where asked for
//   capi_ddiag_add  C_ii += alpha
//
// Everything else of the operator runs on entry points that exist: capi_dsyrk (the Gram matrix), capi_dpotrf, capi_dgemtn_ts, capi_dtrsm_thin,
// capi_dresid_ts, capi_dtri_logdiag, capi_dsym_abs.
//
// capi_drow_pow is a pure stream.  A workgroup owns 512 rows x cb columns (cb = 32, or 8 where 32 would leave the CUs without a workgroup each) and
// walks them in passes of 8 columns: a thread owns one 16-byte row pair (or, where an address or a leading dimension is odd, the rows tid and tid + 256 as
// 8-byte accesses, capi_dsym_scale2's choice), computes its rows' factors ONCE -- a division and a square root per row, not per element -- and has the
// pass's eight loads in flight before the first store.  An element is read and written by the same thread, all loads of a pass before its stores: Y may be X.
//
// Rounding.  The file is compiled with floating-point contraction OFF: every product and every sum below is rounded on its own, so that
//   power +1:    Y = fl(fl(alpha fl(x d)) + fl(beta y))
//   power -1:    Y = fl(fl(alpha fl(x / d)) + fl(beta y))            (a division per element, as a restatement divides)
//   power -1/2:  Y = fl(fl(alpha fl(x w)) + fl(beta y)), w = fl(1 / fl(sqrt d))
// are what numpy gives for alpha * (x * d) + beta * y and its siblings, bit for bit; beta == 0 stores fl(alpha t) and does not read Y.
#include <float.h>
#include <limits.h>

#include "capi_internal.h"
#include "thin_tile.h"

#pragma clang fp contract(off)

namespace {

namespace tt = thin_tile;
using tt::d2_t;

// ---- capi_dlr_diag ----
constexpr int LD_THREADS = 1024;

// One workgroup: a thread takes the entries tid, tid + 1024, ..; its logarithms are added in that order, the 64 sums of a wave meet in a butterfly and
// the 16 waves in order.  Minimum, maximum and the first bad index do not depend on the order they are taken in
__global__ __launch_bounds__(LD_THREADS) void lr_diag_kernel(int64_t n, double shift, const double* __restrict__ diag, const double* __restrict__ schur,
                                                             double* __restrict__ d, double* __restrict__ rec) {
  __shared__ double s_sum[16], s_min[16], s_max[16];
  __shared__ long long s_bad[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double sum = 0.0, dmin = DBL_MAX, dmax = 0.0;
  long long bad = LLONG_MAX;
  for (int64_t j = tid; j < n; j += LD_THREADS) {
    double v = shift;
    if (diag) v = v + diag[j];
    if (schur) v = v + schur[j];
    d[j] = v;
    if (!(v > 0.0) || !(v <= DBL_MAX)) { bad = bad < j ? bad : (long long)j; continue; }       // zero, negative, NaN, Inf
    sum += log(v);
    dmin = v < dmin ? v : dmin; dmax = v > dmax ? v : dmax;
  }
  sum = tt::butterfly_sum<64>(sum);
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const double a0 = __shfl_xor(dmin, s), a1 = __shfl_xor(dmax, s);
    const long long b = __shfl_xor(bad, s);
    dmin = a0 < dmin ? a0 : dmin; dmax = a1 > dmax ? a1 : dmax;
    bad = b < bad ? b : bad;
  }
  if (lane == 0) { s_sum[w] = sum; s_min[w] = dmin; s_max[w] = dmax; s_bad[w] = bad; }
  __syncthreads();
  if (tid != 0) return;
  sum = s_sum[0];
  for (int k = 1; k < 16; ++k) {
    sum += s_sum[k];
    dmin = s_min[k] < dmin ? s_min[k] : dmin; dmax = s_max[k] > dmax ? s_max[k] : dmax;
    bad = s_bad[k] < bad ? s_bad[k] : bad;
  }
  const bool ok = bad == LLONG_MAX;
  rec[0] = ok ? sum : 0.0;
  rec[1] = ok ? dmin : 0.0;
  rec[2] = ok ? dmax : 0.0;
  rec[3] = ok ? 0.0 : (double)(bad + 1);
}

// ---- capi_drow_pow ----
constexpr int RP_THREADS = 256;
constexpr int RP_ROWS = 512, RP_PASS = 8;                      // the rows of a workgroup; the columns of one pass
enum { POW_MUL = 0, POW_DIV = 1, POW_RSQRT = 2 };

// what a row keeps of d_i, and what it does to an element
template <int POW>
__device__ __forceinline__ double row_factor(double di) { return POW == POW_RSQRT ? 1.0 / sqrt(di) : di; }
template <int POW>
__device__ __forceinline__ double row_apply(double x, double f) { return POW == POW_DIV ? x / f : x * f; }
__device__ __forceinline__ double axpby(double alpha, double t, bool read_y, double beta, double y) {
  const double a = alpha * t;
  return read_y ? a + beta * y : a;
}

// One pass: the columns c .. c + np - 1 (np == RP_PASS where FULL) of the thread's two rows ra and rb (adjacent where PAIR: one 16-byte access)
template <int POW, bool PAIR, bool FULL>
__device__ __forceinline__ void row_pow_pass(int64_t c, int np, int64_t ra, int64_t rb, bool vb, double fa, double fb, double alpha, const double* X, int64_t ldx,
                                             bool read_y, double beta, double* Y, int64_t ldy) {
  if (PAIR) {
    d2_t x[RP_PASS], y[RP_PASS];
#pragma unroll
    for (int p = 0; p < RP_PASS; ++p)
      if (FULL || p < np) {
        x[p] = *(const d2_t*)(X + ra + (c + p) * ldx);
        y[p] = read_y ? *(const d2_t*)(Y + ra + (c + p) * ldy) : d2_t{0.0, 0.0};
      }
#pragma unroll
    for (int p = 0; p < RP_PASS; ++p)
      if (FULL || p < np) {
        d2_t o;
        o.x = axpby(alpha, row_apply<POW>(x[p].x, fa), read_y, beta, y[p].x);
        o.y = axpby(alpha, row_apply<POW>(x[p].y, fb), read_y, beta, y[p].y);
        *(d2_t*)(Y + ra + (c + p) * ldy) = o;
      }
  } else {
    double xa[RP_PASS], xb[RP_PASS], ya[RP_PASS], yb[RP_PASS];
#pragma unroll
    for (int p = 0; p < RP_PASS; ++p)
      if (FULL || p < np) {
        xa[p] = X[ra + (c + p) * ldx];
        xb[p] = vb ? X[rb + (c + p) * ldx] : 0.0;
        ya[p] = read_y ? Y[ra + (c + p) * ldy] : 0.0;
        yb[p] = read_y && vb ? Y[rb + (c + p) * ldy] : 0.0;
      }
#pragma unroll
    for (int p = 0; p < RP_PASS; ++p)
      if (FULL || p < np) {
        Y[ra + (c + p) * ldy] = axpby(alpha, row_apply<POW>(xa[p], fa), read_y, beta, ya[p]);
        if (vb) Y[rb + (c + p) * ldy] = axpby(alpha, row_apply<POW>(xb[p], fb), read_y, beta, yb[p]);
      }
  }
}

// VEC: X, Y 16-byte aligned and ldx, ldy even: a thread owns the row pair (i0 + 2 tid, + 1) -- the last pair of an odd m is a single row, taken as one
// 8-byte access; otherwise the rows i0 + tid and i0 + tid + 256.  No row >= m is read or written
template <int POW, bool VEC>
__global__ __launch_bounds__(RP_THREADS) void row_pow_kernel(int64_t m, int64_t r, int cb, const double* __restrict__ d, double alpha, const double* X, int64_t ldx,
                                                             double beta, double* Y, int64_t ldy) {
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * RP_ROWS;
  const int64_t c0 = (int64_t)blockIdx.y * cb, c1 = c0 + cb < r ? c0 + cb : r;
  const int64_t ra = VEC ? i0 + 2 * tid : i0 + tid, rb = VEC ? ra + 1 : ra + RP_THREADS;
  if (ra >= m) return;
  const bool vb = rb < m;
  const double fa = row_factor<POW>(d[ra]), fb = vb ? row_factor<POW>(d[rb]) : 1.0;
  const bool read_y = beta != 0.0;
  int64_t c = c0;
  if (VEC && vb) {
    for (; c + RP_PASS <= c1; c += RP_PASS) row_pow_pass<POW, true, true>(c, RP_PASS, ra, rb, true, fa, fb, alpha, X, ldx, read_y, beta, Y, ldy);
    if (c < c1) row_pow_pass<POW, true, false>(c, (int)(c1 - c), ra, rb, true, fa, fb, alpha, X, ldx, read_y, beta, Y, ldy);
  } else {
    for (; c + RP_PASS <= c1; c += RP_PASS) row_pow_pass<POW, false, true>(c, RP_PASS, ra, rb, vb, fa, fb, alpha, X, ldx, read_y, beta, Y, ldy);
    if (c < c1) row_pow_pass<POW, false, false>(c, (int)(c1 - c), ra, rb, vb, fa, fb, alpha, X, ldx, read_y, beta, Y, ldy);
  }
}

// capi_dcolnorm2's kernel on the result: one workgroup per column, a thread adds the squares of the lines tid, tid + 256, .., a butterfly inside the wave,
// then the four waves in order.  (Contraction is on in here, as it is there: the same sum, bit for bit.)
__global__ __launch_bounds__(RP_THREADS) void row_pow_norm2_kernel(int64_t m, const double* __restrict__ Y, int64_t ldy, double* __restrict__ norm2) {
#pragma clang fp contract(fast)
  __shared__ double red[4];
  const double* y = Y + (int64_t)blockIdx.x * ldy;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < m; i += RP_THREADS) s += y[i] * y[i];
  s = tt::butterfly_sum<64>(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) norm2[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

template <int POW>
void launch_row_pow(capi_handle_t h, bool vec, dim3 grid, int64_t m, int64_t r, int cb, const double* d, double alpha, const double* X, int64_t ldx, double beta,
                    double* Y, int64_t ldy) {
  if (vec) hipLaunchKernelGGL((row_pow_kernel<POW, true>), grid, dim3(RP_THREADS), 0, h->stream, m, r, cb, d, alpha, X, ldx, beta, Y, ldy);
  else hipLaunchKernelGGL((row_pow_kernel<POW, false>), grid, dim3(RP_THREADS), 0, h->stream, m, r, cb, d, alpha, X, ldx, beta, Y, ldy);
}

// ---- capi_ddiag_add ----
__global__ void diag_add_kernel(int64_t n, double alpha, double* __restrict__ C, int64_t ldc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) C[i + i * ldc] += alpha;
}

}  // namespace

extern "C" {

int capi_dlr_diag(capi_handle_t h, int64_t n, double shift, const double* diag, const double* schur, double* d, double* rec) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE(h, n >= 0 && n < (1LL << 31), "n");
  if (n == 0) return CAPI_OK;
  CAPI_REQUIRE(h, d && rec, "d / rec");
  hipLaunchKernelGGL(lr_diag_kernel, dim3(1), dim3(LD_THREADS), 0, h->stream, n, shift, diag, schur, d, rec);
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

int capi_drow_pow(capi_handle_t h, int64_t m, int64_t r, double power, const double* d, double alpha, const double* X, int64_t ldx, double beta, double* Y,
                  int64_t ldy, double* norm2) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE(h, m >= 0 && r >= 0 && r < (1LL << 31), "m / r");
  CAPI_REQUIRE(h, power == 1.0 || power == -1.0 || power == -0.5, "power: +1 multiplies by d, -1 divides by it, -0.5 divides by its square root");
  if (r == 0 || m == 0) return CAPI_OK;
  CAPI_REQUIRE(h, d && X && Y && ldx >= m && ldy >= m, "d / X / Y / ldx >= m / ldy >= m");
  CAPI_REQUIRE(h, X != Y || ldx == ldy, "Y == X needs ldy == ldx");
  const int64_t row_tiles = cdiv(m, RP_ROWS);
  CAPI_REQUIRE(h, row_tiles < (1LL << 31), "m too large");
  // 32 columns a workgroup where that still gives every CU four workgroups, 8 otherwise; more where the grid's second dimension would not hold them
  int64_t cb = row_tiles * cdiv(r, 32) >= 4 * (int64_t)h->num_cu ? 32 : 8;
  while (cdiv(r, cb) > 65535) cb *= 2;
  const dim3 grid((unsigned)row_tiles, (unsigned)cdiv(r, cb));
  const bool vec = (((uintptr_t)X | (uintptr_t)Y) & 15) == 0 && ((ldx | ldy) & 1) == 0;     // workgroups start at even rows: every row pair is 16-byte aligned
  if (power == 1.0) launch_row_pow<POW_MUL>(h, vec, grid, m, r, (int)cb, d, alpha, X, ldx, beta, Y, ldy);
  else if (power == -1.0) launch_row_pow<POW_DIV>(h, vec, grid, m, r, (int)cb, d, alpha, X, ldx, beta, Y, ldy);
  else launch_row_pow<POW_RSQRT>(h, vec, grid, m, r, (int)cb, d, alpha, X, ldx, beta, Y, ldy);
  if (norm2) hipLaunchKernelGGL(row_pow_norm2_kernel, dim3((unsigned)r), dim3(RP_THREADS), 0, h->stream, m, (const double*)Y, ldy, norm2);
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

int capi_ddiag_add(capi_handle_t h, int64_t n, double alpha, double* C, int64_t ldc) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE(h, n >= 0 && n < (1LL << 31), "n");
  if (n == 0) return CAPI_OK;
  CAPI_REQUIRE(h, C && ldc >= n, "C / ldc >= n");
  hipLaunchKernelGGL(diag_add_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream, n, alpha, C, ldc);
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

}  // extern "C"
