// chud_f64.hip -- the rank-r update (sign = +1) or downdate (sign = -1) of an upper triangular factor T of order n (column-major, or a view into a packed
// triangle) and of its inverse: T'^T T' = T^T T + sign V V^T for a THIN V (r <= 32 columns), in O(n^2 r) instead of a new factorisation
// (cholesky::cholinv::update).  LINPACK's dchud / dchdd in one formula.  Not in the reference: its cholinv stops at R and R^-1.
//
//   capi_dchud       T <- T', V is destroyed, the n steps are recorded in a log
//   capi_dchud_inv   Tinv <- T'^-1 from the log, for the diagonal sub-triangle [k0, k1)
//
// STEP k has alpha = T_kk and x = the current row k of V (an r-vector), sg = sign:
//   beta = sqrt(alpha^2 + sg ||x||^2), not positive definite unless alpha^2 + sg ||x||^2 > 0 (a NaN compares false);
//   for every column j >= k:  t = (alpha T_kj + sg x^T v_j) / beta,  v_j <- v_j - x (T_kj + t) / (alpha + beta),  T_kj <- t
// which leaves T_kk = beta and v_k = 0.  The step is a linear map of the pair (T_kj, v_j) that preserves tau^2 + sg ||v||^2.  M = [T; V^T] and
// N = [T^-T; 0] satisfy M^T J N = I with J = diag(I, sg I), and the steps preserve J: the same step applied to the pairs (Tinv_ck, e_c), c <= k, with
// e_c an r-vector that starts at zero and is dropped at the end, turns T^-1 into T'^-1.  The two divisions are taken once per step, as reciprocals.
//
// The schedule is chud_plan.h's: panels of B rows; per panel the DIAGONAL kernel (one wave: a lane owns a column of the B x B diagonal block and its
// v_j in registers, x_k goes through LDS, the B steps follow each other) and the APPLY kernel (a thread owns a trailing column j: v_j in registers,
// the column's B entries of T through an LDS tile so that HBM sees whole column pieces, the panel's log in LDS).  The inverse is the transposed
// picture: a thread owns a row c of Tinv -- consecutive threads read consecutive addresses of a column, packed or not -- and walks k upward with e_c
// in registers, the next chunk of the row on its way while the current one is computed.  Ordering is by kernel boundaries on the handle's stream
// alone: no cooperative launch, no device-side waiting, no atomics, and every sum has a fixed order -- the same bits on every run.
// A failed step sets a device flag: every later kernel of the call reads it at entry and returns.
#include <math.h>

#include "capi_internal.h"
#include "chud_plan.h"
#include "tri_thin_plan.h"

namespace {

namespace cp = chud_plan;
namespace tp = tri_thin_plan;

constexpr int CH_B = cp::B, CH_TP = cp::B + 1;     // rows of a panel; pitch of a column of the apply kernel's tile

struct ChudState { int stopped, info; };

struct ChudArgs {
  double *T, *V, *log;
  ChudState* st;
  int64_t ldt, col0, ldv;
  int n, r;
  double sg;
};

// the fields stay where they lie in ChudArgs / ChudInvArgs: a tri_view_rw in their place cost capi_dchud up to 1.6 % (profiles/tri_view_refactor.txt)
__device__ __forceinline__ double* chud_col(double* T, int64_t ldt, int64_t col0, int64_t j) { return tp::tri_view_rw{T, ldt, col0}.col(j); }

// one step on the pair (tau, v); x[RP] (zero beyond r), ib = 1 / beta, ig = 1 / (alpha + beta)
template <int RP>
__device__ __forceinline__ void chud_step(double& tau, double (&v)[RP], const double* __restrict__ x, double alpha, double ib, double ig, double sg) {
  double dot = 0.0;
#pragma unroll
  for (int c = 0; c < RP; ++c) dot += x[c] * v[c];
  const double t = (alpha * tau + sg * dot) * ib;
  const double w = (tau + t) * ig;
#pragma unroll
  for (int c = 0; c < RP; ++c) v[c] -= x[c] * w;
  tau = t;
}
// .. with the record that chud_stage_log left in LDS
template <int RP>
__device__ __forceinline__ void chud_step_rec(double& tau, double (&v)[RP], const double* __restrict__ rec, double sg) {
  chud_step<RP>(tau, v, rec, rec[RP], rec[RP + 1], rec[RP + 2], sg);
}

// the record of step k from the log, into LDS: called by every thread of the workgroup, nt threads, for the steps [ks, ks + kc)
template <int RP>
__device__ __forceinline__ void chud_stage_log(double* __restrict__ lg, const double* __restrict__ log, int r, int ks, int kc, int tid, int nt) {
  const int64_t LS = r + 2;
  for (int e = tid; e < kc * RP; e += nt) {
    const int k = e / RP, c = e % RP;
    const bool in = c < r;
    const double x = *(in ? log + (ks + k) * LS + c : log);
    lg[k * (RP + 3) + c] = in ? x : 0.0;
  }
  for (int k = tid; k < kc; k += nt) {
    const double alpha = log[(ks + k) * LS + r], beta = log[(ks + k) * LS + r + 1];
    lg[k * (RP + 3) + RP] = alpha;
    lg[k * (RP + 3) + RP + 1] = 1.0 / beta;
    lg[k * (RP + 3) + RP + 2] = 1.0 / (alpha + beta);
  }
}

// the steps [k0, min(k0 + B, n)) on the diagonal block and the panel's rows of V.  One wave; lane l owns column k0 + l
template <int RP>
__global__ __launch_bounds__(64) void chud_diag_kernel(const ChudArgs p, int k0) {
  // the panel's records, x_k (zero beyond r), alpha_k, beta_k: a step publishes its own and reads no other, so one barrier per step is enough; they
  // go to the log in one piece behind the last step (a store to global memory inside the loop would be waited for at every barrier)
  __shared__ double plog[CH_B * (RP + 2)];
  if (p.st->stopped) return;                                                 // (the whole workgroup)
  const int lane = threadIdx.x, n = p.n, r = p.r;
  const int bp = min(CH_B, n - k0);
  const bool own = lane < bp;
  double* const col = chud_col(p.T, p.ldt, p.col0, k0 + (own ? lane : 0)) + k0;
  double tc[CH_B], v[RP];
#pragma unroll
  for (int i = 0; i < CH_B; ++i) {
    const bool in = own && i <= lane;
    const double x = *(in ? col + i : p.T);
    tc[i] = in ? x : 0.0;
  }
#pragma unroll
  for (int c = 0; c < RP; ++c) {
    const bool in = own && c < r;
    const double x = *(in ? p.V + k0 + lane + (int64_t)c * p.ldv : p.V);
    v[c] = in ? x : 0.0;
  }
  int fail = 0;
#pragma unroll
  for (int k = 0; k < CH_B; ++k) {
    if (k < bp && fail == 0) {                                               // (the whole wave)
      double* const rec = plog + k * (RP + 2);
      if (lane == k) {
#pragma unroll
        for (int c = 0; c < RP; ++c) rec[c] = v[c];
        rec[RP] = tc[k];
      }
      __syncthreads();
      const double alpha = rec[RP];
      double nrm = 0.0;
#pragma unroll
      for (int c = 0; c < RP; ++c) nrm += rec[c] * rec[c];
      const double d = alpha * alpha + p.sg * nrm;
      if (!(d > 0.0)) {
        fail = k + 1;
      } else {
        const double beta = sqrt(d);
        if (own && lane >= k) chud_step<RP>(tc[k], v, rec, alpha, 1.0 / beta, 1.0 / (alpha + beta), p.sg);
        if (lane == k) { tc[k] = beta; rec[RP + 1] = beta; }                 // (what the step gives for j == k, to rounding; v_k, now zero, is not used again)
      }
    }
  }
#pragma unroll
  for (int i = 0; i < CH_B; ++i)
    if (own && i <= lane) col[i] = tc[i];
  __syncthreads();
  const int done = fail != 0 ? fail - 1 : bp, LS = r + 2;                    // the finished steps
  for (int e = lane; e < done * LS; e += 64) {
    const int k = e / LS, c = e % LS;
    p.log[(int64_t)(k0 + k) * LS + c] = plog[k * (RP + 2) + (c < r ? c : RP + (c - r))];
  }
  if (fail != 0 && lane == 0) { p.st->info = k0 + fail; p.st->stopped = 1; }
}

// the panel's steps [k0, k0 + bp) on the trailing columns [j0, j0 + COLS) of this workgroup, j0 = k0 + bp + COLS blockIdx.x
template <int RP>
__global__ __launch_bounds__(cp::COLS) void chud_apply_kernel(const ChudArgs p, int k0) {
  __shared__ double tile[cp::COLS * CH_TP];
  __shared__ double lg[CH_B * (RP + 3)];
  if (p.st->stopped) return;                                                 // (the whole workgroup)
  const int tid = threadIdx.x, n = p.n, r = p.r;
  const int bp = min(CH_B, n - k0);
  const int j0 = k0 + bp + cp::COLS * (int)blockIdx.x;
  chud_stage_log<RP>(lg, p.log, r, k0, bp, tid, cp::COLS);
  // rows k0 .. k0 + bp - 1 of the columns j0 ..: strictly above the diagonal
  // (all CH_B loads of a thread are issued before the first is stored to LDS: one memory latency per panel, not one per load)
  double tv[CH_B];
#pragma unroll
  for (int q = 0; q < CH_B; ++q) {
    const int e = tid + q * cp::COLS, row = e % CH_B, c = e / CH_B;
    const bool in = row < bp && j0 + c < n;
    tv[q] = *(in ? chud_col(p.T, p.ldt, p.col0, j0 + c) + k0 + row : p.T);
  }
#pragma unroll
  for (int q = 0; q < CH_B; ++q) {
    const int e = tid + q * cp::COLS;
    tile[(e / CH_B) * CH_TP + e % CH_B] = tv[q];
  }
  const int j = j0 + tid;
  const bool own = j < n;
  double v[RP];
#pragma unroll
  for (int c = 0; c < RP; ++c) {
    const bool in = own && c < r;
    const double x = *(in ? p.V + j + (int64_t)c * p.ldv : p.V);
    v[c] = in ? x : 0.0;
  }
  __syncthreads();
  if (own) {
    double* const tc = tile + tid * CH_TP;
#pragma unroll 4
    for (int k = 0; k < bp; ++k) {
      double tau = tc[k];
      chud_step_rec<RP>(tau, v, lg + k * (RP + 3), p.sg);
      tc[k] = tau;
    }
  }
  __syncthreads();
  for (int e = tid; e < CH_B * cp::COLS; e += cp::COLS) {
    const int row = e % CH_B, c = e / CH_B;
    if (row < bp && j0 + c < n) chud_col(p.T, p.ldt, p.col0, j0 + c)[k0 + row] = tile[c * CH_TP + row];
  }
  if (own)
#pragma unroll
    for (int c = 0; c < RP; ++c)
      if (c < r) p.V[j + (int64_t)c * p.ldv] = v[c];
}

struct ChudInvArgs {
  double* Tinv;
  const double* log;
  int64_t ldt, col0;
  int r, k0, k1;
  double sg;
};

// the steps [k0, k1) on the rows k0 + ROWS blockIdx.x .. of the inverse's sub-triangle [k0, k1): row c takes the steps k >= c
template <int RP>
__global__ __launch_bounds__(cp::ROWS) void chud_inv_kernel(const ChudInvArgs p) {
  constexpr int KC = cp::KCHUNK;
  __shared__ double lg[KC * (RP + 3)];
  const int tid = threadIdx.x, r = p.r, k1 = p.k1;
  const int c = p.k0 + cp::ROWS * (int)blockIdx.x + tid;
  const bool own = c < k1;
  double e[RP], cur[KC], nxt[KC];
#pragma unroll
  for (int q = 0; q < RP; ++q) e[q] = 0.0;
  // the row's entries of the columns ks .. ks + KC - 1, on and right of the diagonal
  auto load = [&](int ks, double (&tv)[KC]) {
#pragma unroll
    for (int q = 0; q < KC; ++q) {
      const int k = ks + q;
      const bool in = own && k < k1 && k >= c;
      const double x = *(in ? chud_col(p.Tinv, p.ldt, p.col0, k) + c : p.Tinv);
      tv[q] = in ? x : 0.0;
    }
  };
  int ks = (int)cp::inv_first_step(p.k0, blockIdx.x);
  load(ks, cur);
  for (; ks < k1; ks += KC) {
    const int kc = min(KC, k1 - ks);
    __syncthreads();                               // the last chunk's records are used up
    chud_stage_log<RP>(lg, p.log, r, ks, kc, tid, cp::ROWS);
    __syncthreads();
    load(ks + KC, nxt);                            // behind the barrier, which would wait for it (nothing beyond k1 is read)
#pragma unroll
    for (int q = 0; q < KC; ++q) {
      const int k = ks + q;
      if (own && k < k1 && k >= c) {
        chud_step_rec<RP>(cur[q], e, lg + q * (RP + 3), p.sg);
        chud_col(p.Tinv, p.ldt, p.col0, k)[c] = cur[q];
      }
    }
#pragma unroll
    for (int q = 0; q < KC; ++q) cur[q] = nxt[q];
  }
}

inline int chud_rp(int64_t r) { return r <= 1 ? 1 : (r <= 2 ? 2 : (r <= 4 ? 4 : (r <= 8 ? 8 : (r <= 16 ? 16 : 32)))); }
inline bool aligned8(const void* q) { return ((uintptr_t)q & 7) == 0; }

#define CHUD_DISPATCH(rp, LAUNCH) \
  switch (rp) {                   \
    case 1: LAUNCH(1); break;     \
    case 2: LAUNCH(2); break;     \
    case 4: LAUNCH(4); break;     \
    case 8: LAUNCH(8); break;     \
    case 16: LAUNCH(16); break;   \
    default: LAUNCH(32); break;   \
  }

}  // namespace

extern "C" {

size_t capi_dchud_log_bytes(int64_t n, int64_t r) {
  if (n < 0 || n >= (1LL << 31) || r < 1 || r > CAPI_TS_MAX_RHS) return 0;
  return sizeof(double) * (size_t)cp::log_doubles(n, r);
}

int capi_dchud(capi_handle_t h, int sign, int64_t n, int64_t r, double* T, int64_t ldt, int64_t col0, double* V, int64_t ldv, double* log,
               int* info_host) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE_THIN_R(h, r);
  CAPI_REQUIRE(h, sign == 1 || sign == -1, "sign: +1 (update) or -1 (downdate)");
  CAPI_REQUIRE(h, n >= 0 && n < (1LL << 31), "n");
  CAPI_REQUIRE_TRI_VIEW(h, n, n, ldt, col0);
  CAPI_REQUIRE(h, ldv >= (n > 1 ? n : 1), "ldv");
  CAPI_REQUIRE(h, info_host, "info_host");
  CAPI_REQUIRE(h, n == 0 || (T && V && log), "T / V / log");
  CAPI_REQUIRE(h, aligned8(T) && aligned8(V) && aligned8(log), "pointers aligned to 8 bytes");
  if (n == 0) { *info_host = 0; return CAPI_OK; }
  void* pv = nullptr;
  const int rc = capi_ws4_get(h, sizeof(ChudState), &pv);
  if (rc != CAPI_OK) return rc;
  ChudArgs p;
  p.T = T; p.V = V; p.log = log; p.st = (ChudState*)pv;
  p.ldt = ldt; p.col0 = ldt > 0 ? 0 : col0; p.ldv = ldv;
  p.n = (int)n; p.r = (int)r; p.sg = (double)sign;
  CAPI_HIP_CHECK(h, hipMemsetAsync(p.st, 0, sizeof(ChudState), h->stream));
  const int rp = chud_rp(r);
  for (int64_t q = 0; q < cp::num_panels(n); ++q) {
    const cp::Panel P = cp::panel(n, q);
    const int64_t na = cp::num_applies(n, P);
    const int k0 = (int)P.k0;
#define CHUD_LAUNCH(RP)                                                                                   \
    do {                                                                                                  \
      hipLaunchKernelGGL(chud_diag_kernel<RP>, dim3(1), dim3(64), 0, h->stream, p, k0);                   \
      if (na > 0) hipLaunchKernelGGL(chud_apply_kernel<RP>, dim3((unsigned)na), dim3(cp::COLS), 0, h->stream, p, k0); \
    } while (0)
    CHUD_DISPATCH(rp, CHUD_LAUNCH)
#undef CHUD_LAUNCH
  }
  CAPI_HIP_CHECK(h, hipGetLastError());
  CAPI_HIP_CHECK(h, hipMemcpyAsync(h->h_info, &p.st->info, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  CAPI_HIP_CHECK(h, hipStreamSynchronize(h->stream));
  *info_host = *h->h_info;
  return CAPI_OK;
}

int capi_dchud_inv(capi_handle_t h, int sign, int64_t n, int64_t r, double* Tinv, int64_t ldt, int64_t col0, const double* log, int64_t k0, int64_t k1) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE_THIN_R(h, r);
  CAPI_REQUIRE(h, sign == 1 || sign == -1, "sign: +1 (update) or -1 (downdate)");
  CAPI_REQUIRE(h, n >= 0 && n < (1LL << 31), "n");
  CAPI_REQUIRE_TRI_VIEW(h, n, n, ldt, col0);
  CAPI_REQUIRE(h, 0 <= k0 && k0 <= k1 && k1 <= n, "0 <= k0 <= k1 <= n");
  CAPI_REQUIRE(h, k0 == k1 || (Tinv && log), "Tinv / log");
  CAPI_REQUIRE(h, aligned8(Tinv) && aligned8(log), "pointers aligned to 8 bytes");
  if (k0 == k1) return CAPI_OK;
  ChudInvArgs p;
  p.Tinv = Tinv; p.log = log;
  p.ldt = ldt; p.col0 = ldt > 0 ? 0 : col0;
  p.r = (int)r; p.k0 = (int)k0; p.k1 = (int)k1; p.sg = (double)sign;
  const unsigned groups = (unsigned)cp::inv_groups(k0, k1);
#define CHUD_LAUNCH(RP) hipLaunchKernelGGL(chud_inv_kernel<RP>, dim3(groups), dim3(cp::ROWS), 0, h->stream, p)
  CHUD_DISPATCH(chud_rp(r), CHUD_LAUNCH)
#undef CHUD_LAUNCH
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

}  // extern "C"
