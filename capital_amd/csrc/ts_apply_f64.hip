// ts_apply_f64.hip -- streaming tall-skinny products with a NARROW output (r <= 32 columns), for least-squares solves on the
// CholeskyQR factors (qr::cacqr::least_squares).  Not in the reference: its cacqr.hpp stops at Q and R.
//
//   capi_dgemtn_ts   C (n x r) <- alpha A^T B + beta C        A m x n, B m x r, tall
//   capi_dresid_ts   Rout (m x r) <- B - A X, colnorm2[j] <- sum_i Rout(i, j)^2      X n x r
//
// Both read A from HBM exactly once and are bound by that stream (8 m (n + r) bytes; the residual adds 8 m r when it is written);
// the arithmetic goes to v_mfma_f64_16x16x4_f64 with the r columns padded to 16 or 32, which at r = 32 is within a factor of two of
// the memory time and far below it for small r.  Every tall kernel of gemm_f64.hip has an n-wide output instead.
//
// capi_dgemtn_ts: the order of k in a dot product is free, so the MFMA's k index is dealt to suit the loads: lane (c, g) of a wave
// takes 16-byte row pairs of ITS OWN column c of a 16-column strip of A (rows 8 q + 2 g, + 1 of a 32-row chunk: the four lane groups g share
// a 64-byte piece per load), and lane (j, g) the same rows of column j of B -- a k-step multiplies one element of every lane.  No transpose
// through LDS.  A workgroup of 8 waves covers 256 columns (two
// strips per wave) of 32-row chunks; the chunk of B is staged through LDS once per workgroup.  Workgroup z of S takes the chunks
// z, z + S, ..; its partial sums go to slab z, and a second launch adds the slabs in the order z = 0, 1, ..: no floating-point
// atomics, the same bits on every run.
// capi_dresid_ts: X stays in LDS ([k][16] planes, one per 16 right-hand sides); a wave owns 32-row tiles of A and multiplies them in the
// row-dot form of thin_tile.h, so that a lane loads and stores 16 bytes of two consecutive rows.
// n beyond what LDS holds (1024 columns at r <= 16, 512 beyond) goes in column blocks whose X is restaged per round of tiles: A is
// still read once.  The squared norms are summed per lane, per wave (a fixed butterfly) and per worker slot, then in slot order.
#include <type_traits>
#include "capi_internal.h"
#include "thin_tile.h"

namespace {

namespace tt = thin_tile;
using tt::d2_t;
using tt::d4_t;

constexpr int TA_THREADS = 512;          // 8 waves, one workgroup per CU
constexpr int TA_RUN = 8;                // rows of its column a lane takes per chunk of capi_dgemtn_ts (four 16-byte pairs)
constexpr int TA_CHUNK = 4 * TA_RUN;     // rows per chunk there: 4 lane groups x a run
constexpr int TA_GROUP = 256;            // columns of A per workgroup: 8 waves x 2 strips x 16
constexpr int TA_LDB = TA_CHUNK + 2;     // LDS column stride of the staged chunk of B
constexpr int TA_TILE = 32;              // rows per wave tile of capi_dresid_ts
constexpr int TA_KS = 8;                 // k-steps per load batch there
constexpr int TA_BATCH = 4 * TA_KS;      // columns of A per batch
constexpr int TA_XLDS = 16384;           // doubles of LDS for X (128 KiB)

struct GemtnArgs {
  const double* A; const double* B; double* slab;
  int64_t m, lda, ldb;
  int n, r, nchunk, a_vec;
};

// ---- C = A^T B ----------------------------------------------------------------------------------------------------------------
template <int RB>
__global__ __launch_bounds__(TA_THREADS) void gemtn_ts_kernel(const GemtnArgs p) {
  __shared__ __attribute__((aligned(16))) double Lb[2][16 * RB * TA_LDB];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c16 = lane & 15, g = lane >> 4;
  const int z = blockIdx.x, S = gridDim.x, cg = blockIdx.y;
  const int col0 = cg * TA_GROUP + 32 * w;                  // first column of this wave's two strips
  const bool live = col0 < p.n, fullw = col0 + 32 <= p.n;   // wave-uniform
  d4_t acc[2][RB];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) acc[t][rb] = (d4_t){0.0, 0.0, 0.0, 0.0};

  // the chunk of B: thread t stages row t & 31 of columns (t >> 5) + 16 q.  The load is unconditional (from a clamped address); the select
  // waits until the value is stored to LDS, behind the MFMA phase
  const int brow = tid & (TA_CHUNK - 1), bcol = tid / TA_CHUNK;
  double bst[RB];
  auto bload = [&](int chunk) {
    const int64_t row = (int64_t)chunk * TA_CHUNK + brow;
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      const int col = bcol + 16 * q;
      const bool in = row < p.m && col < p.r;
      bst[q] = *(in ? p.B + row + (int64_t)col * p.ldb : p.B);
    }
  };
  auto bstage = [&](double* L, int chunk) {
    const int64_t row = (int64_t)chunk * TA_CHUNK + brow;
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      const int col = bcol + 16 * q;
      L[col * TA_LDB + brow] = (row < p.m && col < p.r) ? bst[q] : 0.0;
    }
  };
  // the lane's rows of A: 32 chunk + 8 q + 2 g, + 1 (q = 0..3) of columns col0 + c16 and col0 + 16 + c16: the four lane groups take one 64-byte piece
  auto aload_steady = [&](int chunk, d2_t (&st)[2][TA_RUN / 2]) {
    const double* src = p.A + (int64_t)chunk * TA_CHUNK + 2 * g + (int64_t)(col0 + c16) * p.lda;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < TA_RUN / 2; ++q) st[t][q] = __builtin_nontemporal_load((const d2_t*)(src + (int64_t)(16 * t) * p.lda + 8 * q));
  };
  auto aload_edge = [&](int chunk, d2_t (&st)[2][TA_RUN / 2]) {        // ragged chunk, ragged strip or unaligned A: guarded scalar reads
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int col = col0 + 16 * t + c16;
      const double* src = p.A + (int64_t)col * p.lda;
#pragma unroll
      for (int q = 0; q < TA_RUN / 2; ++q) {
        const int64_t row = (int64_t)chunk * TA_CHUNK + 8 * q + 2 * g;
        d2_t v = {0.0, 0.0};
        if (col < p.n && row < p.m) v.x = src[row];
        if (col < p.n && row + 1 < p.m) v.y = src[row + 1];
        st[t][q] = v;
      }
    }
  };
  auto steady = [&](int chunk) { return p.a_vec && fullw && (int64_t)(chunk + 1) * TA_CHUNK <= p.m; };
  int par = 0;
  // cur holds this chunk's runs, nxt receives the next chunk's.  STEADY: a next chunk exists and it is whole, aligned and full width:
  // the iteration has no branch around its loads
  auto step = [&](int chunk, d2_t (&cur)[2][TA_RUN / 2], d2_t (&nxt)[2][TA_RUN / 2], auto steady_tag) {
    constexpr bool STEADY = decltype(steady_tag)::value;
    const int next = chunk + S;
    if (STEADY) {
      bload(next);
      aload_steady(next, nxt);
    } else if (next < p.nchunk) {
      bload(next);
      if (live) aload_edge(next, nxt);
    }
    if (live) {
      const double* L = Lb[par];
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const double* lb = L + (16 * rb + c16) * TA_LDB + 2 * g;
#pragma unroll
        for (int q = 0; q < TA_RUN / 2; ++q) {
          const d2_t bv = *(const d2_t*)(lb + 8 * q);
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            acc[t][rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[t][q].x, bv.x, acc[t][rb], 0, 0, 0);
            acc[t][rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[t][q].y, bv.y, acc[t][rb], 0, 0, 0);
          }
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }
    if (STEADY || next < p.nchunk) bstage(Lb[par ^ 1], next);
    par ^= 1;
    __syncthreads();
  };
  d2_t ra[2][TA_RUN / 2], rb_[2][TA_RUN / 2];
  int chunk = z;
  if (chunk < p.nchunk) {
    bload(chunk);
    if (live) { if (steady(chunk)) aload_steady(chunk, ra); else aload_edge(chunk, ra); }
    bstage(Lb[0], chunk);
  }
  __syncthreads();
  while (chunk < p.nchunk) {
    if (chunk + S < p.nchunk && steady(chunk + S)) step(chunk, ra, rb_, std::true_type{}); else step(chunk, ra, rb_, std::false_type{});
    chunk += S;
    if (chunk >= p.nchunk) break;
    if (chunk + S < p.nchunk && steady(chunk + S)) step(chunk, rb_, ra, std::true_type{}); else step(chunk, rb_, ra, std::false_type{});
    chunk += S;
  }
  // lane (j = c16, g) holds C(col0 + 16 t + g + 4 reg, 16 rb + j) of this workgroup's chunks: slab [cg][z][256 columns of A][16 RB]
  double* sl = p.slab + ((int64_t)cg * S + z) * (TA_GROUP * 16 * RB);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) sl[(32 * w + 16 * t + g + 4 * reg) * (16 * RB) + 16 * rb + c16] = acc[t][rb][reg];
}

// C(i, j) = alpha (slab 0 + slab 1 + ..) + beta C(i, j), the slabs in index order; beta == 0 does not read C
__global__ __launch_bounds__(256) void gemtn_ts_combine_kernel(const double* __restrict__ slab, int S, int n, int r, int rpad, double alpha,
                                                               double beta, double* __restrict__ C, int64_t ldc) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n * rpad) return;
  const int i = (int)(e / rpad), j = (int)(e % rpad);
  if (j >= r) return;
  const int64_t zs = (int64_t)TA_GROUP * rpad;
  const double* s = slab + ((int64_t)(i / TA_GROUP) * S * TA_GROUP + i % TA_GROUP) * rpad + j;
  double sum = 0.0;
  for (int z = 0; z < S; ++z) sum += s[z * zs];
  double v = alpha * sum;
  if (beta != 0.0) v += beta * C[i + (int64_t)j * ldc];
  C[i + (int64_t)j * ldc] = v;
}

// ---- Rout = B - A X, column norms ------------------------------------------------------------------------------------------------
struct ResidArgs {
  const double* A; const double* X; const double* B; double* R; double* part;
  int64_t m, lda, ldx, ldb, ldr;
  int n, r, ntile, nblk, kb, a_vec, b_vec;   // kb: columns of A per block of X in LDS, a multiple of TA_BATCH
};

template <int RB>
__global__ __launch_bounds__(TA_THREADS) void resid_ts_kernel(const ResidArgs p) {
  extern __shared__ __attribute__((aligned(16))) double Lx[];     // [RB][kb][16]: X(block column k, 16 rb + jj)
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  const int G = gridDim.x, nbatch = p.kb / TA_BATCH;
  const int nround = (p.ntile + 7) >> 3;                   // a round: one tile per wave
  const int nmine = (int)blockIdx.x < nround ? (nround - (int)blockIdx.x + G - 1) / G : 0;
  const int total = nmine * p.nblk * nbatch;               // (round, block, batch) steps of this workgroup
  auto tile_of = [&](int i) { return ((int)blockIdx.x + i * G) * 8 + w; };

  auto fill = [&](int cb) {                                // X's rows cb kb .. of all right-hand sides; zero beyond n and r
    for (int e = tid; e < RB * p.kb * 16; e += TA_THREADS) {
      const int rb = e / (p.kb * 16), rem = e % (p.kb * 16), k = rem >> 4, jj = rem & 15;
      const int col = cb * p.kb + k, j = 16 * rb + jj;
      Lx[e] = (col < p.n && j < p.r) ? p.X[col + (int64_t)j * p.ldx] : 0.0;
    }
  };
  // the lane's piece of a batch: rows 32 tile + 2 r16, + 1 of columns cbase + 4 s + g, s = 0..7 (16 lanes fetch 256 bytes of one column)
  auto is_steady = [&](int i, int cb, int b) {
    return p.a_vec && (int64_t)(tile_of(i) + 1) * TA_TILE <= p.m && cb * p.kb + (b + 1) * TA_BATCH <= p.n;
  };
  auto aload_steady = [&](int i, int cb, int b, d2_t (&st)[TA_KS]) {
    const double* src = p.A + (int64_t)tile_of(i) * TA_TILE + 2 * r16 + (int64_t)(cb * p.kb + b * TA_BATCH + g) * p.lda;
#pragma unroll
    for (int s = 0; s < TA_KS; ++s) st[s] = __builtin_nontemporal_load((const d2_t*)(src + (int64_t)(4 * s) * p.lda));
  };
  auto aload_edge = [&](int i, int cb, int b, d2_t (&st)[TA_KS]) {
    const int64_t row = (int64_t)tile_of(i) * TA_TILE + 2 * r16;
#pragma unroll
    for (int s = 0; s < TA_KS; ++s) {
      const int col = cb * p.kb + b * TA_BATCH + 4 * s + g;
      d2_t v = {0.0, 0.0};
      if (col < p.n && row < p.m) v.x = p.A[row + (int64_t)col * p.lda];
      if (col < p.n && row + 1 < p.m) v.y = p.A[row + 1 + (int64_t)col * p.lda];
      st[s] = v;
    }
  };
  d4_t acc[2][RB];
  double nrm[RB][4];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) nrm[rb][reg] = 0.0;

  // lane (r16, g) holds (A X)(32 tile + 2 r16 + h, 16 rb + g + 4 reg) in acc[h][rb][reg]
  auto epilogue = [&](int i) {
    const int64_t row = (int64_t)tile_of(i) * TA_TILE + 2 * r16;
    const bool whole = p.b_vec && (int64_t)(tile_of(i) + 1) * TA_TILE <= p.m;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int j = 16 * rb + g + 4 * reg;
        if (j >= p.r) continue;
        if (whole) {
          d2_t v = *(const d2_t*)(p.B + row + (int64_t)j * p.ldb);
          v.x -= acc[0][rb][reg];
          v.y -= acc[1][rb][reg];
          if (p.R) *(d2_t*)(p.R + row + (int64_t)j * p.ldr) = v;
          nrm[rb][reg] += v.x * v.x;
          nrm[rb][reg] += v.y * v.y;
        } else {
          if (row < p.m) {
            const double v = p.B[row + (int64_t)j * p.ldb] - acc[0][rb][reg];
            if (p.R) p.R[row + (int64_t)j * p.ldr] = v;
            nrm[rb][reg] += v * v;
          }
          if (row + 1 < p.m) {
            const double v = p.B[row + 1 + (int64_t)j * p.ldb] - acc[1][rb][reg];
            if (p.R) p.R[row + 1 + (int64_t)j * p.ldr] = v;
            nrm[rb][reg] += v * v;
          }
        }
      }
  };
  // one (round i, block cb, batch b) step: prefetch the following step's piece into nxt, multiply cur.  STEADY: a following step exists and
  // its piece is whole and aligned
  auto step = [&](int i, int cb, int b, d2_t (&cur)[TA_KS], d2_t (&nxt)[TA_KS], int ni, int ncb, int nb, bool has_next, auto steady_tag) {
    constexpr bool STEADY = decltype(steady_tag)::value;
    if (b == 0) {
      if (cb == 0) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int rb = 0; rb < RB; ++rb) acc[h][rb] = (d4_t){0.0, 0.0, 0.0, 0.0};
      }
      if (p.nblk > 1) {                                    // restage X: workgroup-uniform (i, cb, b are)
        __syncthreads();
        fill(cb);
        __syncthreads();
      }
    }
    if (STEADY) aload_steady(ni, ncb, nb, nxt);
    else if (has_next) aload_edge(ni, ncb, nb, nxt);
    const double* lx = Lx + (b * TA_BATCH + g) * 16 + r16;
    __builtin_amdgcn_s_setprio(1);
    tt::mfma_row_dots<RB>(acc, lx, p.kb * 16, cur);
    __builtin_amdgcn_s_setprio(0);
    if (b == nbatch - 1 && cb == p.nblk - 1) epilogue(i);
  };
  if (p.nblk == 1) fill(0);
  __syncthreads();
  d2_t pa[TA_KS], pb[TA_KS];
  int i = 0, cb = 0, b = 0;
  if (total > 0) { if (is_steady(0, 0, 0)) aload_steady(0, 0, 0, pa); else aload_edge(0, 0, 0, pa); }
  for (int q = 0; q < total; ++q) {
    int ni = i, ncb = cb, nb = b + 1;
    if (nb == nbatch) { nb = 0; if (++ncb == p.nblk) { ncb = 0; ++ni; } }
    const bool has_next = q + 1 < total, st = has_next && is_steady(ni, ncb, nb);
    if (q & 1) {
      if (st) step(i, cb, b, pb, pa, ni, ncb, nb, has_next, std::true_type{}); else step(i, cb, b, pb, pa, ni, ncb, nb, has_next, std::false_type{});
    } else {
      if (st) step(i, cb, b, pa, pb, ni, ncb, nb, has_next, std::true_type{}); else step(i, cb, b, pa, pb, ni, ncb, nb, has_next, std::false_type{});
    }
    i = ni; cb = ncb; b = nb;
  }
  // squared norms: the 16 lanes that share g hold the rows of the same columns; a fixed butterfly, then one slot per wave
  if (p.part) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const double v = tt::butterfly_sum<16>(nrm[rb][reg]);
        if (r16 == 0) p.part[((int64_t)blockIdx.x * 8 + w) * 32 + 16 * rb + g + 4 * reg] = v;
      }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int capi_dgemtn_ts(capi_handle_t h, int64_t m, int64_t n, int64_t r, double alpha, const double* A, int64_t lda, const double* B, int64_t ldb,
                   double beta, double* C, int64_t ldc) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE_THIN_R(h, r);
  CAPI_REQUIRE(h, m >= 0 && m < (1LL << 35) && n >= 1 && n <= 65535LL * TA_GROUP, "m / n (m < 2^35 rows, n <= 65535 * 256 columns: the grid's limits)");
  CAPI_REQUIRE(h, C && ldc >= n, "C/ldc");
  CAPI_REQUIRE(h, m == 0 || (A && B && lda >= m && ldb >= m), "A/lda/B/ldb");
  const int rb = capi_thin_rb(r), rpad = 16 * rb;
  const int64_t nchunk = cdiv(m, TA_CHUNK), ncg = cdiv(n, TA_GROUP);
  int64_t S = h->num_cu / ncg;
  if (S < 1) S = 1;
  if (S > nchunk) S = nchunk;
  double* slab = nullptr;
  if (S > 0) {
    void* pv = nullptr;
    int rc = capi_ws_get(h, sizeof(double) * (size_t)(ncg * S * TA_GROUP * rpad), &pv);
    if (rc != CAPI_OK) return rc;
    slab = (double*)pv;
    GemtnArgs p;
    p.A = A; p.B = B; p.slab = slab;
    p.m = m; p.lda = lda; p.ldb = ldb;
    p.n = (int)n; p.r = (int)r; p.nchunk = (int)nchunk;
    p.a_vec = aligned16(A) && (lda & 1) == 0;
    const dim3 grid((unsigned)S, (unsigned)ncg);
    if (rb == 1) hipLaunchKernelGGL(gemtn_ts_kernel<1>, grid, dim3(TA_THREADS), 0, h->stream, p);
    else hipLaunchKernelGGL(gemtn_ts_kernel<2>, grid, dim3(TA_THREADS), 0, h->stream, p);
  }
  hipLaunchKernelGGL(gemtn_ts_combine_kernel, dim3((unsigned)cdiv(n * rpad, 256)), dim3(256), 0, h->stream, slab, (int)S, (int)n, (int)r, rpad, alpha, beta,
                     C, ldc);
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

int capi_dresid_ts(capi_handle_t h, int64_t m, int64_t n, int64_t r, const double* A, int64_t lda, const double* X, int64_t ldx, const double* B,
                   int64_t ldb, double* Rout, int64_t ldr, double* colnorm2) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE_THIN_R(h, r);
  CAPI_REQUIRE(h, m >= 0 && m < (1LL << 35) && n >= 1 && n <= 65535LL * TA_GROUP, "m / n (m < 2^35 rows, n <= 65535 * 256 columns: the grid's limits)");
  CAPI_REQUIRE(h, X && ldx >= n, "X/ldx");
  CAPI_REQUIRE(h, m == 0 || (A && B && lda >= m && ldb >= m && (!Rout || ldr >= m)), "A/lda/B/ldb/Rout/ldr");
  const int rb = capi_thin_rb(r);
  const int64_t ntile = cdiv(m, TA_TILE), nround = cdiv(ntile, 8);
  int64_t G = nround < h->num_cu ? nround : h->num_cu;
  double* part = nullptr;
  if (G > 0) {
    if (colnorm2) {
      void* pv = nullptr;
      int rc = capi_ws_get(h, sizeof(double) * (size_t)(G * 8 * 32), &pv);
      if (rc != CAPI_OK) return rc;
      part = (double*)pv;
    }
    const int kbmax = TA_XLDS / (16 * rb);                  // columns of A whose X fits in LDS
    ResidArgs p;
    p.A = A; p.X = X; p.B = B; p.R = Rout; p.part = part;
    p.m = m; p.lda = lda; p.ldx = ldx; p.ldb = ldb; p.ldr = ldr;
    p.n = (int)n; p.r = (int)r; p.ntile = (int)ntile;
    p.nblk = (int)cdiv(n, kbmax);
    p.kb = (int)(cdiv(cdiv(n, p.nblk), TA_BATCH) * TA_BATCH);
    p.a_vec = aligned16(A) && (lda & 1) == 0;
    p.b_vec = aligned16(B) && (ldb & 1) == 0 && (!Rout || (aligned16(Rout) && (ldr & 1) == 0));
    const size_t lds = sizeof(double) * (size_t)rb * p.kb * 16;
    if (rb == 1) {
      CAPI_RAISE_LDS_LIMIT(h, CAPI_ATTR_RESID_TS0, resid_ts_kernel<1>, sizeof(double) * TA_XLDS);
      hipLaunchKernelGGL(resid_ts_kernel<1>, dim3((unsigned)G), dim3(TA_THREADS), lds, h->stream, p);
    } else {
      CAPI_RAISE_LDS_LIMIT(h, CAPI_ATTR_RESID_TS0 + 1, resid_ts_kernel<2>, sizeof(double) * TA_XLDS);
      hipLaunchKernelGGL(resid_ts_kernel<2>, dim3((unsigned)G), dim3(TA_THREADS), lds, h->stream, p);
    }
  }
  // slots of 32 doubles, of which the first rpad were written
  if (colnorm2) hipLaunchKernelGGL(tt::colnorms_kernel<>, dim3(1), dim3(64), 0, h->stream, (const double*)part, G * 8, 32, (int)r, colnorm2);
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

}  // extern "C"
