// equil_f64.hip -- power-of-two equilibration of a symmetric positive definite A (cholesky::cholinv::equilibrate): LAPACK's dpoequb + dlaqsy, with the
// exponent rule of capi_dgram_equilibrate_shift / capi_dtri_rescale at any order.  Not in the reference: its cholinv stops at R and R^-1.
//
//   capi_dpoequ2      dscale[j] <- 2^e_j, e_j = floor(ex_j / 2) for a_jj = f 2^ex_j, f in [0.5, 1); rec <- scond, amax, amin, first bad entry
//   capi_dsym_scale2  a_ij <- ldexp(a_ij, -sign (e_i + e_j)) on the upper triangle, in place: A_s = D^-1 A D^-1 (sign = +1) and back (sign = -1)
//   capi_drow_scale2  Y(i, j) <- ldexp(X(i, j), sign e_i) on a thin block, with the squared column norms of Y where asked for
//
// Every scale factor is a power of two, so every operation here is exact (where nothing over- or underflows) and the way back restores every bit.  An
// element takes ONE exponent addition (v_ldexp_f64: zero, Inf and NaN pass through, a result below the normal range is rounded once), never two
// multiplications whose intermediate could leave the range.  e_i is read from the exponent field of dscale[i], which is always a normal number.
//
// capi_dsym_scale2 is bound by the stream over the triangle.  A tile is 512 rows x 64 columns, walked in eight passes of 8 columns: a thread owns one
// 16-byte row pair (or, where an address or a leading dimension is odd, the rows tid and tid + 256 as 8-byte accesses, copy2d_kernel<VEC>'s choice) and
// has the pass's eight loads in flight before the first store.  Only the tiles that touch the triangle are launched: the workgroup index is turned into
// (row tile, column tile) by inverting the count of the tiles before a column tile.  The tiles that the diagonal or the matrix's edge crosses load
// every element from a clamped address and select afterwards, as the thin kernels do: nothing below the diagonal or beyond row n - 1 is read into a
// result or stored to, whatever it holds.
#include <float.h>
#include <limits.h>

#include "capi_internal.h"
#include "thin_tile.h"

namespace {

namespace tt = thin_tile;
using tt::d2_t;

// the unbiased exponent of a normal power of two (dscale[i])
__device__ __forceinline__ int scale_exponent(double s) { return (int)((__double_as_longlong(s) >> 52) & 0x7ff) - 1023; }

// ---- capi_dpoequ2 ----
constexpr int PQ_THREADS = 1024;

// ex with a = f 2^ex, f in [0.5, 1) (frexp's convention), from the bits; a > 0 and finite, subnormals included
__device__ __forceinline__ int frexp_exponent(double a) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(a);
  const int E = (int)((b >> 52) & 0x7ff);
  if (E != 0) return E - 1022;
  return (63 - __clzll((long long)(b & 0xfffffffffffffULL))) - 1073;           // the top set bit p of the fraction: a in [2^(p - 1074), 2^(p - 1073))
}

// One workgroup: a thread takes the entries tid, tid + 1024, ..  Minima, maxima and the first bad index do not depend on the order they are taken in
__global__ __launch_bounds__(PQ_THREADS) void poequ2_kernel(int64_t n, const double* __restrict__ A, int64_t lda, double* __restrict__ dscale,
                                                            double* __restrict__ rec) {
  __shared__ int s_emin[16], s_emax[16];
  __shared__ double s_amin[16], s_amax[16];
  __shared__ long long s_bad[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int emin = INT_MAX, emax = INT_MIN;
  double amin = DBL_MAX, amax = 0.0;
  long long bad = LLONG_MAX;
  for (int64_t j = tid; j < n; j += PQ_THREADS) {
    const double a = A[j + j * lda];
    if (!(a > 0.0) || !(a <= DBL_MAX)) { bad = bad < j ? bad : (long long)j; continue; }       // zero, negative, NaN, Inf
    const int e = frexp_exponent(a) >> 1;                                                     // floor: the shift is arithmetic
    emin = e < emin ? e : emin; emax = e > emax ? e : emax;
    amin = a < amin ? a : amin; amax = a > amax ? a : amax;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int e0 = __shfl_xor(emin, d), e1 = __shfl_xor(emax, d);
    const double a0 = __shfl_xor(amin, d), a1 = __shfl_xor(amax, d);
    const long long b = __shfl_xor(bad, d);
    emin = e0 < emin ? e0 : emin; emax = e1 > emax ? e1 : emax;
    amin = a0 < amin ? a0 : amin; amax = a1 > amax ? a1 : amax;
    bad = b < bad ? b : bad;
  }
  if (lane == 0) { s_emin[w] = emin; s_emax[w] = emax; s_amin[w] = amin; s_amax[w] = amax; s_bad[w] = bad; }
  __syncthreads();
  for (int k = 0; k < 16; ++k) {
    emin = s_emin[k] < emin ? s_emin[k] : emin; emax = s_emax[k] > emax ? s_emax[k] : emax;
    amin = s_amin[k] < amin ? s_amin[k] : amin; amax = s_amax[k] > amax ? s_amax[k] : amax;
    bad = s_bad[k] < bad ? s_bad[k] : bad;
  }
  const bool ok = bad == LLONG_MAX;
  for (int64_t j = tid; j < n; j += PQ_THREADS) {
    double s = 1.0;
    if (ok) s = __longlong_as_double((long long)((frexp_exponent(A[j + j * lda]) >> 1) + 1023) << 52);
    dscale[j] = s;
  }
  if (tid == 0) {
    rec[0] = ok ? ldexp(1.0, emin - emax) : 1.0;
    rec[1] = ok ? amax : 0.0;
    rec[2] = ok ? amin : 0.0;
    rec[3] = ok ? 0.0 : (double)(bad + 1);
  }
}

// ---- capi_dsym_scale2 ----
constexpr int SC_THREADS = 256;
constexpr int SC_ROWS = 512, SC_COLS = 64, SC_PASS = 8;       // a tile; the columns of one pass
constexpr int SC_K = SC_ROWS / SC_COLS;                       // column tiles per row tile

// The tiles that touch the upper triangle: column tile J has the row tiles 0 .. J / SC_K, and before it lie tiles_before(J) tiles
__host__ __device__ inline int64_t tiles_before(int64_t J) {
  const int64_t q = J / SC_K, s = J % SC_K;
  return SC_K * q * (q + 1) / 2 + s * (q + 1);
}

template <bool VEC>
__global__ __launch_bounds__(SC_THREADS) void sym_scale2_kernel(int64_t n, double* __restrict__ A, int64_t lda, const double* __restrict__ dscale, int sign) {
  const int tid = threadIdx.x;
  // (I, J) from the workgroup's index t: q = J / SC_K is the largest q with SC_K q (q + 1) / 2 <= t
  const int64_t t = blockIdx.x;
  int64_t q = (int64_t)((sqrt(1.0 + 8.0 * (double)t / SC_K) - 1.0) * 0.5);
  while (q > 0 && SC_K * q * (q + 1) / 2 > t) --q;
  while (SC_K * (q + 1) * (q + 2) / 2 <= t) ++q;
  const int64_t rem = t - SC_K * q * (q + 1) / 2;
  const int64_t J = SC_K * q + rem / (q + 1), I = rem % (q + 1);
  const int64_t i0 = I * SC_ROWS, j0 = J * SC_COLS;
  const bool whole = i0 + SC_ROWS <= j0 + 1 && j0 + SC_COLS <= n;     // every row of the tile is above every column's diagonal entry, no ragged column
  if (whole) {                                                        // (then i0 + SC_ROWS <= n as well)
    if (VEC) {
      const int64_t i = i0 + 2 * tid;
      const int ei0 = scale_exponent(dscale[i]), ei1 = scale_exponent(dscale[i + 1]);
      for (int64_t c = j0; c < j0 + SC_COLS; c += SC_PASS) {
        d2_t v[SC_PASS];
#pragma unroll
        for (int p = 0; p < SC_PASS; ++p) v[p] = *(const d2_t*)(A + i + (c + p) * lda);
#pragma unroll
        for (int p = 0; p < SC_PASS; ++p) {
          const int ej = scale_exponent(dscale[c + p]);
          v[p].x = ldexp(v[p].x, -sign * (ei0 + ej));
          v[p].y = ldexp(v[p].y, -sign * (ei1 + ej));
        }
#pragma unroll
        for (int p = 0; p < SC_PASS; ++p) *(d2_t*)(A + i + (c + p) * lda) = v[p];
      }
    } else {
      const int64_t i = i0 + tid;
      const int ei0 = scale_exponent(dscale[i]), ei1 = scale_exponent(dscale[i + SC_THREADS]);
      for (int64_t c = j0; c < j0 + SC_COLS; c += SC_PASS) {
        double x[SC_PASS], y[SC_PASS];
#pragma unroll
        for (int p = 0; p < SC_PASS; ++p) { x[p] = A[i + (c + p) * lda]; y[p] = A[i + SC_THREADS + (c + p) * lda]; }
#pragma unroll
        for (int p = 0; p < SC_PASS; ++p) {
          const int ej = scale_exponent(dscale[c + p]);
          x[p] = ldexp(x[p], -sign * (ei0 + ej));
          y[p] = ldexp(y[p], -sign * (ei1 + ej));
        }
#pragma unroll
        for (int p = 0; p < SC_PASS; ++p) { A[i + (c + p) * lda] = x[p]; A[i + SC_THREADS + (c + p) * lda] = y[p]; }
      }
    }
    return;
  }
  // An edge tile: the rows tid and tid + 256, every element from a clamped address (A: the first element, always inside), selected afterwards
  const int64_t ra = i0 + tid, rb = ra + SC_THREADS;
  const int ea = scale_exponent(dscale[ra < n ? ra : 0]), eb = scale_exponent(dscale[rb < n ? rb : 0]);
  for (int64_t c = j0; c < j0 + SC_COLS && c < n; c += SC_PASS) {
    if (i0 + (tid & ~63) > c + SC_PASS - 1) continue;               // wave-uniform: the wave's first row lies below the pass's last diagonal entry
    double x[SC_PASS], y[SC_PASS];
    bool va[SC_PASS], vb[SC_PASS];
#pragma unroll
    for (int p = 0; p < SC_PASS; ++p) {
      const int64_t col = c + p;
      va[p] = col < n && ra <= col;                                 // (ra <= col < n: the row is inside too)
      vb[p] = col < n && rb <= col;
      x[p] = *(va[p] ? A + ra + col * lda : A);
      y[p] = *(vb[p] ? A + rb + col * lda : A);
    }
#pragma unroll
    for (int p = 0; p < SC_PASS; ++p) {
      const int ej = scale_exponent(dscale[c + p < n ? c + p : 0]);
      x[p] = ldexp(x[p], -sign * (ea + ej));
      y[p] = ldexp(y[p], -sign * (eb + ej));
    }
#pragma unroll
    for (int p = 0; p < SC_PASS; ++p) {
      if (va[p]) A[ra + (c + p) * lda] = x[p];
      if (vb[p]) A[rb + (c + p) * lda] = y[p];
    }
  }
}

// ---- capi_drow_scale2 ----
constexpr int RS_THREADS = 256;

// One workgroup per column.  A thread takes the lines tid, tid + 256, ..; the squares meet in a butterfly inside the wave and the four waves in order
__global__ __launch_bounds__(RS_THREADS) void row_scale2_kernel(int64_t m, const double* __restrict__ dscale, int sign, const double* X, int64_t ldx, double* Y,
                                                                int64_t ldy, double* __restrict__ norm2) {
  __shared__ double red[4];
  const double* x = X + (int64_t)blockIdx.x * ldx;
  double* y = Y + (int64_t)blockIdx.x * ldy;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < m; i += RS_THREADS) {
    const double v = ldexp(x[i], sign * scale_exponent(dscale[i]));
    y[i] = v;
    s += v * v;
  }
  if (!norm2) return;
  s = tt::butterfly_sum<64>(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) norm2[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

}  // namespace

extern "C" {

int capi_dpoequ2(capi_handle_t h, int64_t n, const double* A, int64_t lda, double* dscale, double* rec) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE(h, n >= 0 && n < (1LL << 31), "n");
  if (n == 0) return CAPI_OK;
  CAPI_REQUIRE(h, A && lda >= n && dscale && rec, "A / lda >= n / dscale / rec");
  hipLaunchKernelGGL(poequ2_kernel, dim3(1), dim3(PQ_THREADS), 0, h->stream, n, A, lda, dscale, rec);
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

int capi_dsym_scale2(capi_handle_t h, int64_t n, double* A, int64_t lda, const double* dscale, int sign) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE(h, n >= 0 && n < (1LL << 31), "n");
  CAPI_REQUIRE(h, sign == 1 || sign == -1, "sign: +1 scales, -1 undoes");
  if (n == 0) return CAPI_OK;
  CAPI_REQUIRE(h, A && lda >= n && dscale, "A / lda >= n / dscale");
  const int64_t tiles = tiles_before(cdiv(n, SC_COLS));
  CAPI_REQUIRE(h, tiles < (1LL << 31), "n too large");
  const bool vec = ((uintptr_t)A & 15) == 0 && (lda & 1) == 0;       // whole tiles start at even rows: every row pair is then 16-byte aligned
  if (vec) hipLaunchKernelGGL(sym_scale2_kernel<true>, dim3((unsigned)tiles), dim3(SC_THREADS), 0, h->stream, n, A, lda, dscale, sign);
  else hipLaunchKernelGGL(sym_scale2_kernel<false>, dim3((unsigned)tiles), dim3(SC_THREADS), 0, h->stream, n, A, lda, dscale, sign);
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

int capi_drow_scale2(capi_handle_t h, int64_t m, int64_t r, const double* dscale, int sign, const double* X, int64_t ldx, double* Y, int64_t ldy, double* norm2) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE(h, m >= 0 && r >= 0 && r < (1LL << 31), "m / r");
  CAPI_REQUIRE(h, sign == 1 || sign == -1, "sign: +1 multiplies by dscale, -1 divides");
  if (r == 0 || m == 0) return CAPI_OK;
  CAPI_REQUIRE(h, dscale && X && Y && ldx >= m && ldy >= m, "dscale / X / Y / ldx >= m / ldy >= m");
  hipLaunchKernelGGL(row_scale2_kernel, dim3((unsigned)r), dim3(RS_THREADS), 0, h->stream, m, dscale, sign, X, ldx, Y, ldy, norm2);
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

}  // extern "C"
