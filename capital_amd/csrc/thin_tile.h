// thin_tile.h -- device code shared by the thin kernels (ts_apply_f64.hip, tri_apply_f64.hip, sym_apply_f64.hip): a large operand streamed from HBM
// once, times a block of r <= 32 columns that sits in LDS, on v_mfma_f64_16x16x4_f64 with the r columns padded to 16-column planes.
//
// The instruction computes D (16 x 16) += A (16 x 4) B (4 x 16).  Lane (l16 = lane & 15, g4 = lane >> 4) supplies A(l16, g4) and B(g4, l16) and holds
// D(g4 + 4 reg, l16) in reg = 0..3.  A wave's 32 x 32 tile of the streamed operand takes part in one of two forms, 8 row pairs (16 bytes) per lane:
//   ROW DOTS (tile times block): piece q is rows 2 l16, + 1 of column 4 q + g4 -- 16 lanes fetch 256 bytes of a column.  The thin block is the A operand:
//     acc[h][rb][reg] = (tile X)(2 l16 + h, 16 rb + g4 + 4 reg), the two rows of a pair in two accumulator sets.
//   COLUMN DOTS (tile^T times block): piece q is rows 8 (q & 3) + 2 g4, + 1 of the lane's OWN column 16 (q >> 2) + l16 -- the four lane groups share a
//     64-byte piece.  The order of k in a dot product is free, so the MFMA's k index is dealt to suit the loads; no transpose through LDS:
//     acc[t][rb][reg] = (tile^T X)(16 t + g4 + 4 reg, 16 rb + l16).
// In LDS the thin block is [plane rb][contraction index k][16 columns], `plane` doubles from one plane to the next.
#pragma once
#include <stdint.h>

namespace thin_tile {

typedef double d4_t __attribute__((ext_vector_type(4)));
typedef double d2_t __attribute__((ext_vector_type(2)));
// A row pair of a column that is 8-byte aligned only (every other column of a packed triangle, any column behind an odd leading dimension).  Global
// loads of gfx950 need dword alignment only, so the steady loops load 16 bytes all the same (an odd column costs one more 128-byte line per
// 256-byte run); the type is declared 8-byte aligned so that the compiler may not assume more.
typedef d2_t d2u_t __attribute__((aligned(8)));

// lx: the lane's first element of the thin block, L + (k0 + g4) * 16 + l16 for tile contraction index k0
template <int RB>
__device__ __forceinline__ void mfma_row_dots(d4_t (&acc)[2][RB], const double* lx, int plane, const d2_t (&cur)[8]) {
#pragma unroll
  for (int q = 0; q < 8; ++q)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const double xv = lx[rb * plane + 64 * q];
      acc[0][rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(xv, cur[q].x, acc[0][rb], 0, 0, 0);
      acc[1][rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(xv, cur[q].y, acc[1][rb], 0, 0, 0);
    }
}
// lx: L + (k0 + 2 g4) * 16 + l16
template <int RB>
__device__ __forceinline__ void mfma_col_dots(d4_t (&acc)[2][RB], const double* lx, int plane, const d2_t (&cur)[8]) {
#pragma unroll
  for (int q = 0; q < 8; ++q)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const double b0 = lx[rb * plane + 8 * (q & 3) * 16], b1 = lx[rb * plane + (8 * (q & 3) + 1) * 16];
      acc[q >> 2][rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[q].x, b0, acc[q >> 2][rb], 0, 0, 0);
      acc[q >> 2][rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[q].y, b1, acc[q >> 2][rb], 0, 0, 0);
    }
}

// the sum over LANES consecutive lanes by a fixed butterfly: the same bits on every run
template <int LANES>
__device__ __forceinline__ double butterfly_sum(double v) {
#pragma unroll
  for (int d = 1; d < LANES; d <<= 1) v += __shfl_xor(v, d);
  return v;
}
// the squared column norms of the lines of a workgroup of THREADS = 256 (four waves: the caller's launch bound): value(j) is the thread's element of
// column j (0 beyond the last line).  Square (rounded on its own, never fused into the butterfly's first sum), butterfly inside the wave, then the
// four waves in order: part[group blockIdx.x][j], groups of `stride` doubles (part may be null).  Holds MAXR x 4 doubles of static LDS
template <int MAXR, int THREADS, class VALUE>
__device__ __forceinline__ void group_colnorms(int r, double* part, int stride, VALUE&& value) {
  static_assert(THREADS == 256, "red[][4] and the ordered sum below are for four waves");
  __shared__ double red[MAXR][4];
  const int tid = threadIdx.x;
  for (int j = 0; j < r; ++j) {
    // contraction is off for v * v and the sums of this block only: value() is the caller's lambda, compiled under the caller's setting, as before
#pragma clang fp contract(off)
    const double v = value(j), sq = butterfly_sum<64>(v * v);
    if ((tid & 63) == 0) red[j][tid >> 6] = sq;
  }
  __syncthreads();
  if (part && tid < r) part[(int64_t)blockIdx.x * stride + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}
// the larger of the two, a NaN winning over any number: a maximum that must not hide one
__device__ __forceinline__ double max_nan(double m, double v) { return (v > m || v != v) ? v : m; }
template <int LANES>
__device__ __forceinline__ double butterfly_max(double v) {
#pragma unroll
  for (int d = 1; d < LANES; d <<= 1) v = max_nan(v, __shfl_xor(v, d));
  return v;
}
// the column maxima in group_colnorms's arrangement: part[group blockIdx.x][j] = the largest value(j) of the workgroup's 256 lines (part may be null)
template <int MAXR, int THREADS, class VALUE>
__device__ __forceinline__ void group_colmax(int r, double* part, int stride, VALUE&& value) {
  static_assert(THREADS == 256, "red[][4] is for four waves");
  __shared__ double red[MAXR][4];
  const int tid = threadIdx.x;
  for (int j = 0; j < r; ++j) {
    const double m = butterfly_max<64>(value(j));
    if ((tid & 63) == 0) red[j][tid >> 6] = m;
  }
  __syncthreads();
  if (part && tid < r) part[(int64_t)blockIdx.x * stride + tid] = max_nan(max_nan(max_nan(red[tid][0], red[tid][1]), red[tid][2]), red[tid][3]);
}
// colnorm2[j] = part[group 0][j] + part[group 1][j] + ..  (groups of `stride` doubles); groups == 0 gives zeros.  Local to the including file (the
// anonymous namespace), and a template so that only the files that launch it hold a copy
namespace {
template <class = void>
__global__ __launch_bounds__(64) void colnorms_kernel(const double* __restrict__ part, int64_t groups, int stride, int r, double* __restrict__ colnorm2) {
  const int j = threadIdx.x;
  if (j >= r) return;
  double sum = 0.0;
  for (int64_t g = 0; g < groups; ++g) sum += part[g * stride + j];
  colnorm2[j] = sum;
}
// colmax[j] = the largest of part[group][j] (values >= 0, or NaN); groups == 0 gives zeros
template <class = void>
__global__ __launch_bounds__(64) void colmax_kernel(const double* __restrict__ part, int64_t groups, int stride, int r, double* __restrict__ colmax) {
  const int j = threadIdx.x;
  if (j >= r) return;
  double m = 0.0;
  for (int64_t g = 0; g < groups; ++g) m = max_nan(m, part[g * stride + j]);
  colmax[j] = m;
}
}  // namespace

}  // namespace thin_tile
