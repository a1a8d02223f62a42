// qrcp_f64.hip -- capi_dgeqp3 for gfx950: Householder QR with column pivoting (LAPACK's dgeqp3 in dlaqp2's unblocked form) of a block of order up to
// CAPI_GEQP3_MAX, the rank-revealing step of capi_dgelsy: A = Q1 R1 by capi_dgeqrf, then R1 P = Q2 R here.  Not in the reference: lapack/interface.h
// declares _geqrf and _orgqr only.
//
// Swap-free: a column stays where it is in W, a chosen column is marked (sel[c] = its step) and never moved; the output image is assembled column by
// column in a second mr x n block W2 and copied back at the end.  ONE LAUNCH PER STEP j, 256-thread workgroups; a WAVE owns QP_CPW = 2 columns and a
// workgroup QP_COLS = 8 for the whole call, so a column's running norms (vn1, vn2), its mark and its part of the candidate have one writer:
//   - every workgroup reduces the per-workgroup candidates (value, index) the launch before left, under the total order of pivots_before (the larger
//     running norm, ties to the smaller index; a NaN was entered as -inf): the first index p of the largest vn1 among the columns not yet chosen;
//   - every workgroup forms the reflector from the read-only pivot column W(j:mr, p): alpha = W(j, p), s2 = the sum of squares below alpha (a thread adds
//     rows j + 1 + tid, + 256, .. ascending, a butterfly inside the wave, the four waves in order), nu = sqrt(alpha^2 + s2); every workgroup holds the
//     same bits and takes the same decision;
//   - stops unless nu > rtol nu_0 && nu > 0 (a NaN compares false and stops): workgroup 0 writes the rank and a flag, every later launch reads the flag
//     at entry and returns;
//   - dlarfg without its rescaling: beta = -sign(alpha) nu, tau = (beta - alpha) / beta, v = x / (alpha - beta) (a division per element), v_0 = 1; when
//     s2 == 0 (nothing below alpha) tau = 0, beta = alpha.  v is staged in LDS (mr - j <= 2048 doubles, 16 KiB);
//   - a wave applies a_c -= tau (v^T a_c) v to its columns that are not chosen (two passes over the column: the dot product -- lanes take rows j + lane,
//     + 64, .., a butterfly -- then the update, which also sums the squares of the new rows below j) and downdates the running norm by dlaqp2's
//     two-vector rule: temp = max(0, 1 - (|a_jc| / vn1)^2), temp2 = temp (vn1 / vn2)^2; temp2 <= tol3z = sqrt(2^-53): vn1 = vn2 = the norm just summed
//     from the column; else vn1 *= sqrt(temp);
//   - the pivot's owner writes column j of the image to W2 (rows < j of the pivot column, beta, v below), tau[j] and the mark;
//   - a workgroup ends by writing its candidate for step j + 1 to the OTHER of two candidate arrays (workgroups of this launch still read this step's).
// The host enqueues the steps in rounds of 64 and reads the flag once per round.  Steps are ordered by kernel boundaries on the handle's stream alone:
// no cooperative launch, no device-side waiting, no atomics.  All sums have a fixed order: two calls on the same bits give identical bytes.  Every loop
// has a trip count fixed by mr and n: non-finite input ends the call like any other, with 0 <= rank <= min(mr, n) and jpvt a permutation.
#include <math.h>

#include "capi_internal.h"
#include "thin_tile.h"

namespace {

namespace tt = thin_tile;

constexpr int QP_T = 256;                    // threads of a workgroup
constexpr int QP_W = QP_T / 64;
constexpr int QP_CPW = 2;                    // columns a wave owns
constexpr int QP_COLS = QP_W * QP_CPW;       // columns a workgroup owns
constexpr int QP_ROUND = 64;                 // steps enqueued between two reads of the stop flag
constexpr int QP_NONE = 0x7fffffff;          // the index of "no candidate": after every column index
constexpr double QP_TOL3Z = 1.0536712127723509e-08;   // sqrt(2^-53)
static_assert(CAPI_GEQP3_MAX / QP_COLS <= QP_T, "a thread reads one candidate");

struct QpState {
  double nu0;          // the pivot norm of step 0
  int stopped;         // a step met a pivot norm <= rtol nu0
  int rank;
};
struct QpCand { double v; int i; int pad; };

// (av, ai) before (bv, bi): the larger value, ties to the smaller index -- a strict total order (no NaN reaches it)
__device__ __forceinline__ bool pivots_before(double av, int ai, double bv, int bi) { return av > bv || (av == bv && ai < bi); }

// the sum of the workgroup's values in every thread: a butterfly inside the wave, the four waves in order
__device__ __forceinline__ double wg_sum(double s, double* reds) {
  s = tt::butterfly_sum<64>(s);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) reds[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((reds[0] + reds[1]) + reds[2]) + reds[3];
}

// the first of the waves' candidates (wave-uniform bv, bi) goes to out[workgroup]
__device__ __forceinline__ void wg_candidate_out(double bv, int bi, double* redv, int* redi, QpCand* out) {
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { redv[threadIdx.x >> 6] = bv; redi[threadIdx.x >> 6] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < QP_W; ++w)
      if (pivots_before(redv[w], redi[w], bv, bi)) { bv = redv[w]; bi = redi[w]; }
    out[blockIdx.x] = QpCand{bv, bi, 0};
  }
}

// vn1 = vn2 = the column norms, sel <- -1, tau <- 0, the state, the candidates of step 0
__global__ __launch_bounds__(QP_T) void qrcp_init_kernel(int mr, int n, int kmin, const double* __restrict__ W, int64_t ldw, double* __restrict__ tau,
                                                         double* __restrict__ vn1, double* __restrict__ vn2, int* __restrict__ sel,
                                                         QpCand* __restrict__ cand, QpState* __restrict__ st) {
  __shared__ double redv[QP_W];
  __shared__ int redi[QP_W];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.x * QP_T + tid;
  if (t < kmin) tau[t] = 0.0;
  if (t == 0) { st->nu0 = 0.0; st->stopped = 0; st->rank = kmin; }
  double bv = -INFINITY;
  int bi = QP_NONE;
  for (int cc = 0; cc < QP_CPW; ++cc) {
    const int c = blockIdx.x * QP_COLS + wave * QP_CPW + cc;
    if (c >= n) break;
    const double* col = W + (int64_t)c * ldw;
    double s = 0.0;
    for (int i = lane; i < mr; i += 64) s += col[i] * col[i];
    const double nrm = sqrt(tt::butterfly_sum<64>(s));
    if (lane == 0) { vn1[c] = nrm; vn2[c] = nrm; sel[c] = -1; }
    const double w = nrm == nrm ? nrm : -INFINITY;
    if (pivots_before(w, c, bv, bi)) { bv = w; bi = c; }
  }
  wg_candidate_out(bv, bi, redv, redi, cand);
}

// step j: see the file comment.  cin: the candidates for this step, cout: for the next
__global__ __launch_bounds__(QP_T) void qrcp_step_kernel(int mr, int n, int j, int nwg, double rtol, double* __restrict__ W, int64_t ldw, double* __restrict__ W2,
                                                         double* __restrict__ tau, double* __restrict__ vn1, double* __restrict__ vn2, int* __restrict__ sel,
                                                         const QpCand* __restrict__ cin, QpCand* __restrict__ cout, QpState* st) {
  __shared__ double v[CAPI_GEQP3_MAX];
  __shared__ double redv[QP_W], reds[QP_W];
  __shared__ int redi[QP_W];
  __shared__ int stopped;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) stopped = st->stopped;
  __syncthreads();
  if (stopped) return;                                                      // (the whole workgroup, and every workgroup)
  // the pivot: the first of the candidates, in every thread of every workgroup
  double bv = -INFINITY;
  int bi = QP_NONE;
  if (tid < nwg) { const QpCand c = cin[tid]; bv = c.v; bi = c.i; }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const double ov = __shfl_xor(bv, s);
    const int oi = __shfl_xor(bi, s);
    if (pivots_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if (lane == 0) { redv[wave] = bv; redi[wave] = bi; }
  __syncthreads();
  bv = redv[0];
  bi = redi[0];
#pragma unroll
  for (int w = 1; w < QP_W; ++w)
    if (pivots_before(redv[w], redi[w], bv, bi)) { bv = redv[w]; bi = redi[w]; }
  const bool none = bi >= n;                                                // cannot happen while j < n; a guard for the address below
  const int p = none ? 0 : bi;
  // the pivot column's norm from the column itself, and its rows below j into LDS
  const double* pc = W + (int64_t)p * ldw;
  const double alpha = pc[j];
  double s = 0.0;
  for (int i = j + 1 + tid; i < mr; i += QP_T) {
    const double x = pc[i];
    v[i - j] = x;
    s += x * x;
  }
  const double s2 = wg_sum(s, reds);
  const double nu = sqrt(alpha * alpha + s2);
  const double nu0 = j == 0 ? nu : st->nu0;
  if (none || !(nu > rtol * nu0 && nu > 0.0)) {                             // a NaN compares false and stops
    if (blockIdx.x == 0 && tid == 0) { st->rank = j; st->stopped = 1; }
    return;
  }
  if (j == 0 && blockIdx.x == 0 && tid == 0) st->nu0 = nu;
  double beta = alpha, tj = 0.0;
  if (s2 != 0.0) {                                                          // else: nothing below alpha, the identity reflector in dlarfg's form
    beta = -copysign(nu, alpha);
    tj = (beta - alpha) / beta;
    const double den = alpha - beta;
    for (int i = j + 1 + tid; i < mr; i += QP_T) v[i - j] /= den;           // the thread's own entries
  }
  if (tid == 0) v[0] = 1.0;
  __syncthreads();
  // the wave's columns
  double* col[QP_CPW];
  bool act[QP_CPW];
  int cidx[QP_CPW];
  for (int cc = 0; cc < QP_CPW; ++cc) {
    const int c = blockIdx.x * QP_COLS + wave * QP_CPW + cc;
    cidx[cc] = c;
    col[cc] = W + (int64_t)(c < n ? c : 0) * ldw;
    act[cc] = c < n && c != p && sel[c] < 0;
    if (c == p) {                                                           // the owner: column j of the image
      double* out = W2 + (int64_t)j * mr;
      for (int i = lane; i < j; i += 64) out[i] = pc[i];
      for (int i = j + lane; i < mr; i += 64) out[i] = i == j ? beta : v[i - j];
      if (lane == 0) { sel[c] = j; tau[j] = tj; }
    }
  }
  double dot[QP_CPW] = {0.0, 0.0};
  for (int i = j + lane; i < mr; i += 64) {
    const double vv = v[i - j];
#pragma unroll
    for (int cc = 0; cc < QP_CPW; ++cc)
      if (act[cc]) dot[cc] += vv * col[cc][i];
  }
  double ss[QP_CPW] = {0.0, 0.0}, ajj[QP_CPW] = {0.0, 0.0}, t[QP_CPW];
#pragma unroll
  for (int cc = 0; cc < QP_CPW; ++cc) t[cc] = tj * tt::butterfly_sum<64>(dot[cc]);
  for (int i = j + lane; i < mr; i += 64) {
    const double vv = v[i - j];
#pragma unroll
    for (int cc = 0; cc < QP_CPW; ++cc)
      if (act[cc]) {
        const double x = col[cc][i] - t[cc] * vv;
        col[cc][i] = x;
        if (i > j) ss[cc] += x * x; else ajj[cc] = x;
      }
  }
  bv = -INFINITY;
  bi = QP_NONE;
#pragma unroll
  for (int cc = 0; cc < QP_CPW; ++cc) {
    if (!act[cc]) continue;                                                 // (wave-uniform)
    const int c = cidx[cc];
    const double below = sqrt(tt::butterfly_sum<64>(ss[cc])), a = fabs(__shfl(ajj[cc], 0));
    double n1 = vn1[c], n2 = vn2[c];
    if (n1 != 0.0) {
      const double q = a / n1;
      double temp = 1.0 - q * q;
      temp = temp > 0.0 ? temp : 0.0;                                       // (a NaN becomes 0: recomputed below)
      const double rr = n1 / n2, temp2 = temp * (rr * rr);
      if (!(temp2 > QP_TOL3Z)) { n1 = below; n2 = below; }
      else n1 *= sqrt(temp);
      if (lane == 0) { vn1[c] = n1; vn2[c] = n2; }
    }
    const double w = n1 == n1 ? n1 : -INFINITY;
    if (pivots_before(w, c, bv, bi)) { bv = w; bi = c; }
  }
  wg_candidate_out(bv, bi, redv, redi, cout);
}

// one workgroup per column c.  A chosen column: jpvt[its step] = c (its image is in W2 already).  Any other: it goes behind the chosen ones, ascending,
// whole (its rows < rank hold R12's column, the rows below the remainder)
__global__ __launch_bounds__(QP_T) void qrcp_tail_kernel(int mr, int n, const double* __restrict__ W, int64_t ldw, double* __restrict__ W2,
                                                         const int* __restrict__ sel, int* __restrict__ jpvt, const QpState* __restrict__ st) {
  __shared__ int redc[QP_W];
  const int tid = threadIdx.x, c = blockIdx.x;
  const int s = sel[c];
  if (s >= 0) {
    if (tid == 0) jpvt[s] = c;
    return;
  }
  int before = 0;                                                           // columns not chosen in front of c
  for (int i = tid; i < c; i += QP_T) before += sel[i] < 0;
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) before += __shfl_xor(before, k);
  if ((tid & 63) == 0) redc[tid >> 6] = before;
  __syncthreads();
  const int pos = st->rank + (((redc[0] + redc[1]) + redc[2]) + redc[3]);
  if (pos >= n) return;                                                     // (cannot happen: rank + the columns not chosen = n)
  if (tid == 0) jpvt[pos] = c;
  const double* src = W + (int64_t)c * ldw;
  double* dst = W2 + (int64_t)pos * mr;
  for (int i = tid; i < mr; i += QP_T) dst[i] = src[i];
}

static size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

int capi_dgeqp3(capi_handle_t h, int64_t mr, int64_t n, double* W, int64_t ldw, int* jpvt, double* tau, double rtol, int* rank_host) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE(h, mr >= 0 && n >= 0 && mr <= CAPI_GEQP3_MAX && n <= CAPI_GEQP3_MAX, "mr, n: 0 .. CAPI_GEQP3_MAX (2048)");
  CAPI_REQUIRE(h, rank_host, "rank_host");
  CAPI_REQUIRE(h, rtol == rtol, "rtol is not a number");
  CAPI_REQUIRE(h, ldw >= mr, "ldw >= mr");
  if (mr == 0 || n == 0) { *rank_host = 0; return CAPI_OK; }
  CAPI_REQUIRE(h, W && jpvt && tau, "W / jpvt / tau");
  CAPI_REQUIRE(h, ((uintptr_t)W & 7) == 0 && ((uintptr_t)tau & 7) == 0 && ((uintptr_t)jpvt & 3) == 0, "pointers aligned to 8 bytes (jpvt to 4)");
  const int mi = (int)mr, ni = (int)n, kmin = mi < ni ? mi : ni, nwg = (int)cdiv(n, QP_COLS);
  if (rtol < 0.0) rtol = (double)(mr > n ? mr : n) * 0x1p-52;
  // the call's scratch: the image block, the state, two candidate arrays, the running norms, the marks
  const size_t o_st = sizeof(double) * (size_t)mr * (size_t)n, o_cand = o_st + up16(sizeof(QpState)), o_vn = o_cand + 2 * sizeof(QpCand) * (size_t)nwg,
               o_sel = o_vn + 2 * sizeof(double) * (size_t)n, total = o_sel + sizeof(int) * (size_t)n;
  void* pv = nullptr;
  int rc = capi_ws_get(h, total, &pv);
  if (rc != CAPI_OK) return rc;
  char* const b = (char*)pv;
  double* const W2 = (double*)b;
  QpState* const st = (QpState*)(b + o_st);
  QpCand* const cand[2] = {(QpCand*)(b + o_cand), (QpCand*)(b + o_cand) + nwg};
  double* const vn1 = (double*)(b + o_vn);
  double* const vn2 = vn1 + n;
  int* const sel = (int*)(b + o_sel);
  const dim3 grid((unsigned)nwg), block(QP_T);
  hipLaunchKernelGGL(qrcp_init_kernel, grid, block, 0, h->stream, mi, ni, kmin, (const double*)W, ldw, tau, vn1, vn2, sel, cand[0], st);
  CAPI_HIP_CHECK(h, hipGetLastError());
  for (int j0 = 0; j0 < kmin; j0 += QP_ROUND) {
    const int j1 = j0 + QP_ROUND < kmin ? j0 + QP_ROUND : kmin;
    for (int j = j0; j < j1; ++j)
      hipLaunchKernelGGL(qrcp_step_kernel, grid, block, 0, h->stream, mi, ni, j, nwg, rtol, W, ldw, W2, tau, vn1, vn2, sel, (const QpCand*)cand[j & 1],
                         cand[(j + 1) & 1], st);
    CAPI_HIP_CHECK(h, hipGetLastError());
    if (j1 == kmin) break;
    // the one read of the state word per round: a stop ends the enqueueing
    int stopped = 0;
    CAPI_HIP_CHECK(h, hipMemcpyAsync(&stopped, &st->stopped, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    CAPI_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    if (stopped) break;
  }
  hipLaunchKernelGGL(qrcp_tail_kernel, dim3((unsigned)n), block, 0, h->stream, mi, ni, (const double*)W, ldw, W2, (const int*)sel, jpvt, (const QpState*)st);
  CAPI_HIP_CHECK(h, hipGetLastError());
  rc = capi_dlacpy(h, 0, mr, n, W2, mr, W, ldw);
  if (rc != CAPI_OK) return rc;
  QpState out;
  CAPI_HIP_CHECK(h, hipMemcpyAsync(&out, st, sizeof(QpState), hipMemcpyDeviceToHost, h->stream));
  CAPI_HIP_CHECK(h, hipStreamSynchronize(h->stream));
  *rank_host = out.rank;
  return CAPI_OK;
}

}  // extern "C"
