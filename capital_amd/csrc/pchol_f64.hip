// pchol_f64.hip -- diagonally pivoted, PARTIAL Cholesky of a symmetric positive semidefinite (or numerically low-rank) matrix of any order,
// A ~= L L^T with L n x k, k <= max_rank: what cholesky::cholinv::factor_pivoted calls where factor() refuses.  Not in the reference: cholinv.hpp stops
// at R and R^-1.
//
//   capi_dpchol          the factorization: L, piv, the remaining Schur diagonal d, the rank and trace of what was left out
//   capi_dpchol_thresh   the threshold a capi_dpchol call with the same (n, A, tol) stops at, bit for bit
//
// Swap-free: A is only read (its upper triangle), L lies in A's own row ordering, a chosen row is marked and never moved.  ONE LAUNCH PER STEP j,
// 256-thread workgroups, a thread owns row i through the whole call:
//   - every workgroup reduces the small array of per-workgroup candidates (value, index) that the launch before left, under the total order of
//     pivots_before (the larger value, ties to the smaller index; a NaN was entered as -inf): the first index p of the largest remaining d_i.  No
//     workgroup reads the whole of d;
//   - stops unless d_p > thresh (a NaN compares false and stops): workgroup 0 writes the rank and a flag to a device word, every later launch reads the
//     flag at entry and returns;
//   - stages the pivot row L(p, 0 .. j) in LDS (j <= 4096 doubles, 32 KiB), once per workgroup;
//   - L(i, j) = (A(i, p) - sum_{l < j} L(i, l) L(p, l)) / sqrt(d_p), l ascending: the reads of L's earlier columns are coalesced over i; chosen rows
//     take an exact zero, row p takes sqrt(d_p); d_i <- fl(d_i - fl(L(i, j)^2)), two roundings, never fused, so that the running diagonal can be
//     recomputed from L bit for bit;
//   - ends by writing its own candidate for step j + 1 to the OTHER of two candidate arrays (workgroups of the same launch still read this step's).
// The host enqueues the steps in rounds of 64 and reads the flag once per round, so a stop at rank 50 of max_rank 4096 costs 64 launches, not 4096.
// Steps are ordered by kernel boundaries on the handle's stream alone: no cooperative launch, no device-side waiting, no flag that anyone spins on, no
// atomics.  All sums have a fixed order: two calls on the same bits give identical bytes.  Every loop has a trip count fixed by n and max_rank:
// non-finite input ends the call like any other, with 0 <= rank <= max_rank and piv a permutation (an index enters piv once, when its row is marked).
#include <math.h>

#include "capi_internal.h"
#include "thin_tile.h"

namespace {

namespace tt = thin_tile;

constexpr int PC_T = 256;            // threads of a workgroup = rows of a workgroup
constexpr int PC_W = PC_T / 64;
constexpr int PC_ROUND = 64;         // steps enqueued between two reads of the stop flag
constexpr int PC_NONE = 0x7fffffff;  // the index of "no candidate": after every row index

struct PcState {
  double thresh;       // tol * trace(A), or n u max_i a_ii
  double resid;        // sum of d over the rows that were not chosen
  int stopped;         // a step met a pivot <= thresh
  int rank;
};
struct PcCand { double v; int i; int pad; };
struct PcPart { double sum, max; };

// (av, ai) before (bv, bi): the larger value, ties to the smaller index -- a strict total order (no NaN reaches it)
__device__ __forceinline__ bool pivots_before(double av, int ai, double bv, int bi) { return av > bv || (av == bv && ai < bi); }

// fl(d - fl(s s)): the product and the difference rounded one after the other.  (__dmul_rn is a plain product to the compiler, which contracts it into
// the subtraction; the pragma is what keeps the two roundings apart)
__device__ __forceinline__ double minus_square(double d, double s) {
#pragma clang fp contract(off)
  const double q = s * s;
  return d - q;
}

// the first of the workgroup's candidates under pivots_before, in every thread: a butterfly inside the wave, the waves in order.  The leading barrier
// lets the arrays be used again by a second call
__device__ __forceinline__ void wg_first(double& bv, int& bi, double* redv, int* redi) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const double ov = __shfl_xor(bv, s);
    const int oi = __shfl_xor(bi, s);
    if (pivots_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { redv[threadIdx.x >> 6] = bv; redi[threadIdx.x >> 6] = bi; }
  __syncthreads();
  bv = redv[0];
  bi = redi[0];
#pragma unroll
  for (int w = 1; w < PC_W; ++w)
    if (pivots_before(redv[w], redi[w], bv, bi)) { bv = redv[w]; bi = redi[w]; }
}

// d <- diag(A), sel <- -1 (both may be null: the threshold alone), and per workgroup the sum and the maximum of its diagonal entries and its candidate
// for step 0.  A NaN counts as -inf for the maximum and stays a NaN in the sum
__global__ __launch_bounds__(PC_T) void pchol_init_kernel(int n, const double* __restrict__ A, int64_t lda, double* __restrict__ d, int* __restrict__ sel,
                                                          PcCand* __restrict__ cand, PcPart* __restrict__ part) {
  __shared__ double reds[PC_W], redv[PC_W];
  __shared__ int redi[PC_W];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * PC_T + tid;
  double a = 0.0, w = -INFINITY;
  int wi = PC_NONE;
  if (i < n) {
    a = A[i + i * lda];
    if (d) { d[i] = a; sel[i] = -1; }
    w = a == a ? a : -INFINITY;
    wi = (int)i;
  }
  const double s = tt::butterfly_sum<64>(a);
  if ((tid & 63) == 0) reds[tid >> 6] = s;
  wg_first(w, wi, redv, redi);
  if (tid == 0) {
    part[blockIdx.x] = PcPart{((reds[0] + reds[1]) + reds[2]) + reds[3], w};
    cand[blockIdx.x] = PcCand{w, wi, 0};
  }
}

// state <- (thresh, 0, not stopped, rank max_rank).  One workgroup: a thread's workgroups in order, a butterfly inside the wave, the four waves in order
__global__ __launch_bounds__(PC_T) void pchol_state_kernel(int n, int nwg, double tol, int max_rank, const PcPart* __restrict__ part, PcState* __restrict__ st) {
  __shared__ double reds[PC_W], redm[PC_W];
  const int tid = threadIdx.x;
  double s = 0.0, m = -INFINITY;
  for (int b = tid; b < nwg; b += PC_T) {
    const PcPart q = part[b];
    s += q.sum;
    m = q.max > m ? q.max : m;
  }
  s = tt::butterfly_sum<64>(s);
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    const double o = __shfl_xor(m, k);
    m = o > m ? o : m;
  }
  if ((tid & 63) == 0) { reds[tid >> 6] = s; redm[tid >> 6] = m; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < PC_W; ++w) m = redm[w] > m ? redm[w] : m;
    const double trace = ((reds[0] + reds[1]) + reds[2]) + reds[3];
    st->thresh = tol < 0.0 ? (double)n * 0x1p-53 * m : tol * trace;          // tol < 0: LAPACK dpstrf's default
    st->resid = 0.0;
    st->stopped = 0;
    st->rank = max_rank;
  }
}

// step j: see the file comment.  cin: the candidates for this step, cout: for the next
__global__ __launch_bounds__(PC_T) void pchol_step_kernel(int n, int j, int nwg, const double* __restrict__ A, int64_t lda, double* __restrict__ L, int64_t ldl,
                                                          int* __restrict__ piv, double* __restrict__ d, int* __restrict__ sel,
                                                          const PcCand* __restrict__ cin, PcCand* __restrict__ cout, PcState* st) {
  __shared__ double prow[CAPI_PCHOL_MAX_RANK];
  __shared__ double redv[PC_W];
  __shared__ int redi[PC_W];
  __shared__ int stopped;
  const int tid = threadIdx.x;
  if (tid == 0) stopped = st->stopped;
  __syncthreads();
  if (stopped) return;                                                      // (the whole workgroup, and every workgroup)
  const double thresh = st->thresh;
  double bv = -INFINITY;
  int bi = PC_NONE;
  for (int b = tid; b < nwg; b += PC_T) {
    const PcCand c = cin[b];
    if (pivots_before(c.v, c.i, bv, bi)) { bv = c.v; bi = c.i; }
  }
  wg_first(bv, bi, redv, redi);
  // every thread of every workgroup holds the same (bv, bi): the decision is the launch's.  A candidate that passes is a row index: "no candidate"
  // and a NaN carry -inf, which is above no threshold
  if (!(bv > thresh) || bi >= n) {
    if (blockIdx.x == 0 && tid == 0) { st->rank = j; st->stopped = 1; }
    return;
  }
  const int p = bi;
  for (int l = tid; l < j; l += PC_T) prow[l] = L[p + (int64_t)l * ldl];
  __syncthreads();
  const double ajj = sqrt(bv);
  const int64_t i = (int64_t)blockIdx.x * PC_T + tid;
  double w = -INFINITY;
  int wi = PC_NONE;
  if (i < n) {
    double* const Lij = L + i + (int64_t)j * ldl;
    if (i == p) {
      *Lij = ajj;
      sel[i] = j;
      d[i] = 0.0;
      piv[j] = p;
    } else if (sel[i] >= 0) {
      *Lij = 0.0;
    } else {
      double s = i < p ? A[i + (int64_t)p * lda] : A[p + i * lda];
      const double* const Li = L + i;
#pragma unroll 8
      for (int l = 0; l < j; ++l) s -= Li[(int64_t)l * ldl] * prow[l];
      s /= ajj;
      *Lij = s;
      const double dn = minus_square(d[i], s);
      d[i] = dn;
      w = dn == dn ? dn : -INFINITY;
      wi = (int)i;
    }
  }
  wg_first(w, wi, redv, redi);
  if (tid == 0) cout[blockIdx.x] = PcCand{w, wi, 0};
}

// per workgroup: how many of its rows were not chosen, and the sum of their d (a butterfly inside the wave, the four waves in order)
__global__ __launch_bounds__(PC_T) void pchol_tail_count_kernel(int n, const int* __restrict__ sel, const double* __restrict__ d, int* __restrict__ cnt,
                                                                double* __restrict__ psum) {
  __shared__ double reds[PC_W];
  __shared__ int redc[PC_W];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * PC_T + tid;
  const bool rest = i < n && sel[i] < 0;
  const double s = tt::butterfly_sum<64>(rest ? d[i] : 0.0);
  const int c = __popcll(__ballot(rest));
  if ((tid & 63) == 0) { reds[tid >> 6] = s; redc[tid >> 6] = c; }
  __syncthreads();
  if (tid == 0) {
    psum[blockIdx.x] = ((reds[0] + reds[1]) + reds[2]) + reds[3];
    cnt[blockIdx.x] = ((redc[0] + redc[1]) + redc[2]) + redc[3];
  }
}

// piv[rank ..] <- the rows that were not chosen, ascending; workgroup 0: state.resid <- the sum of psum, a thread's workgroups in order, a butterfly, the
// four waves in order
__global__ __launch_bounds__(PC_T) void pchol_tail_kernel(int n, int nwg, const int* __restrict__ sel, const int* __restrict__ cnt, const double* __restrict__ psum,
                                                          int* __restrict__ piv, PcState* st) {
  __shared__ double reds[PC_W];
  __shared__ int redc[PC_W], redo[PC_W];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t i = (int64_t)blockIdx.x * PC_T + tid;
  int before = 0;                                                           // rows not chosen in the workgroups before this one
  for (int b = tid; b < (int)blockIdx.x; b += PC_T) before += cnt[b];
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) before += __shfl_xor(before, k);
  const bool rest = i < n && sel[i] < 0;
  const unsigned long long mask = __ballot(rest);
  if (lane == 0) { redo[wave] = before; redc[wave] = __popcll(mask); }
  double s = 0.0;
  if (blockIdx.x == 0) {
    for (int b = tid; b < nwg; b += PC_T) s += psum[b];
    s = tt::butterfly_sum<64>(s);
    if (lane == 0) reds[wave] = s;
  }
  __syncthreads();
  int64_t pos = (int64_t)st->rank + (((redo[0] + redo[1]) + redo[2]) + redo[3]);
  for (int w = 0; w < wave; ++w) pos += redc[w];
  pos += __popcll(mask & ((1ull << lane) - 1ull));
  if (rest && pos < n) piv[pos] = (int)i;
  if (blockIdx.x == 0 && tid == 0) st->resid = ((reds[0] + reds[1]) + reds[2]) + reds[3];
}

struct PcScratch {
  PcState* st;
  PcCand* cand[2];
  PcPart* part;
  double* psum;
  int* cnt;
  int* sel;
};

static size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// the call's scratch, of the handle's workspace: the state, two candidate arrays, the partial sums and counts per workgroup, the marks per row
static int pchol_scratch(capi_handle_t h, int64_t n, int64_t nwg, PcScratch* s) {
  const size_t o_cand = up16(sizeof(PcState)), o_part = o_cand + 2 * sizeof(PcCand) * (size_t)nwg, o_psum = o_part + sizeof(PcPart) * (size_t)nwg,
               o_cnt = o_psum + up16(sizeof(double) * (size_t)nwg), o_sel = o_cnt + up16(sizeof(int) * (size_t)nwg), total = o_sel + sizeof(int) * (size_t)n;
  void* pv = nullptr;
  const int rc = capi_ws4_get(h, total, &pv);
  if (rc != CAPI_OK) return rc;
  char* const b = (char*)pv;
  s->st = (PcState*)b;
  s->cand[0] = (PcCand*)(b + o_cand);
  s->cand[1] = s->cand[0] + nwg;
  s->part = (PcPart*)(b + o_part);
  s->psum = (double*)(b + o_psum);
  s->cnt = (int*)(b + o_cnt);
  s->sel = (int*)(b + o_sel);
  return CAPI_OK;
}

}  // namespace

extern "C" {

int capi_dpchol_thresh(capi_handle_t h, int64_t n, const double* A, int64_t lda, double tol, double* thresh_host) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE(h, n >= 1 && n < (1LL << 31), "n: 1 <= n < 2^31");
  CAPI_REQUIRE(h, A && lda >= n && thresh_host, "A / lda >= n / thresh_host");
  CAPI_REQUIRE(h, tol == tol, "tol is not a number");
  const int64_t nwg = cdiv(n, PC_T);
  PcScratch s;
  int rc = pchol_scratch(h, n, nwg, &s);
  if (rc != CAPI_OK) return rc;
  hipLaunchKernelGGL(pchol_init_kernel, dim3((unsigned)nwg), dim3(PC_T), 0, h->stream, (int)n, A, lda, (double*)nullptr, (int*)nullptr, s.cand[0], s.part);
  hipLaunchKernelGGL(pchol_state_kernel, dim3(1), dim3(PC_T), 0, h->stream, (int)n, (int)nwg, tol, 0, (const PcPart*)s.part, s.st);
  CAPI_HIP_CHECK(h, hipGetLastError());
  double t = 0.0;
  CAPI_HIP_CHECK(h, hipMemcpyAsync(&t, &s.st->thresh, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  CAPI_HIP_CHECK(h, hipStreamSynchronize(h->stream));
  *thresh_host = t;
  return CAPI_OK;
}

int capi_dpchol(capi_handle_t h, int64_t n, const double* A, int64_t lda, double tol, int64_t max_rank, double* L, int64_t ldl, int* piv, double* d,
                int* rank_host, double* resid_trace_host) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE(h, n >= 1 && n < (1LL << 31), "n: 1 <= n < 2^31");
  CAPI_REQUIRE(h, max_rank >= 1 && max_rank <= n && max_rank <= CAPI_PCHOL_MAX_RANK, "max_rank: 1 <= max_rank <= min(n, CAPI_PCHOL_MAX_RANK)");
  CAPI_REQUIRE(h, A && lda >= n && L && ldl >= n, "A / lda >= n / L / ldl >= n");
  CAPI_REQUIRE(h, piv && d && rank_host && resid_trace_host, "piv / d / rank_host / resid_trace_host");
  CAPI_REQUIRE(h, tol == tol, "tol is not a number");
  const int64_t nwg = cdiv(n, PC_T);
  PcScratch s;
  int rc = pchol_scratch(h, n, nwg, &s);
  if (rc != CAPI_OK) return rc;
  const int ni = (int)n, wi = (int)nwg, kmax = (int)max_rank;
  const dim3 grid((unsigned)nwg), block(PC_T);
  hipLaunchKernelGGL(pchol_init_kernel, grid, block, 0, h->stream, ni, A, lda, d, s.sel, s.cand[0], s.part);
  hipLaunchKernelGGL(pchol_state_kernel, dim3(1), block, 0, h->stream, ni, wi, tol, kmax, (const PcPart*)s.part, s.st);
  CAPI_HIP_CHECK(h, hipGetLastError());
  for (int j0 = 0; j0 < kmax; j0 += PC_ROUND) {
    const int j1 = j0 + PC_ROUND < kmax ? j0 + PC_ROUND : kmax;
    for (int j = j0; j < j1; ++j)
      hipLaunchKernelGGL(pchol_step_kernel, grid, block, 0, h->stream, ni, j, wi, A, lda, L, ldl, piv, d, s.sel, (const PcCand*)s.cand[j & 1], s.cand[(j + 1) & 1], s.st);
    CAPI_HIP_CHECK(h, hipGetLastError());
    if (j1 == kmax) break;
    // the one read of the state word per round: a stop ends the enqueueing
    CAPI_HIP_CHECK(h, hipMemcpyAsync(h->h_info, &s.st->stopped, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    CAPI_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    if (*h->h_info) break;
  }
  hipLaunchKernelGGL(pchol_tail_count_kernel, grid, block, 0, h->stream, ni, (const int*)s.sel, (const double*)d, s.cnt, s.psum);
  hipLaunchKernelGGL(pchol_tail_kernel, grid, block, 0, h->stream, ni, wi, (const int*)s.sel, (const int*)s.cnt, (const double*)s.psum, piv, s.st);
  CAPI_HIP_CHECK(h, hipGetLastError());
  PcState out;
  CAPI_HIP_CHECK(h, hipMemcpyAsync(&out, s.st, sizeof(PcState), hipMemcpyDeviceToHost, h->stream));
  CAPI_HIP_CHECK(h, hipStreamSynchronize(h->stream));
  *rank_host = out.rank;
  *resid_trace_host = out.resid;
  return CAPI_OK;
}

}  // extern "C"
