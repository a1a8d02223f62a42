// sym_apply_f64.hip -- a SYMMETRIC matrix, given by its upper triangle, times a thin block (r <= 32 columns): the residual of the solves on the
// cholinv factors (cholesky::cholinv::solve) and the weights of their error bounds.  Not in the reference: its cholinv stops at R and R^-1.
//
//   capi_dresid_sym   Rout (n x r) <- B - S X, colnorm2[j] <- sum_i Rout(i, j)^2      S = triu(A) + triu(A, 1)^T, column-major A
//   capi_dsym_abs     W (n x r) <- |S| |X| + |B|, colmax[j] <- max_i W(i, j)          the same kernel on absolute values, at every r (16 columns a pass)
//
// The upper triangle is read from HBM once; nothing below A's diagonal is read into a result.  The triangle is cut into a p x p block triangle,
// one workgroup per block (sym_thin_plan.h).  A 32 x 32 tile U of block (I, J) feeds two products: U X_J goes to the lines of I and U^T X_I to
// the lines of J, both on v_mfma_f64_16x16x4_f64 with the r columns padded to 16.  This kernel serves r < 8 (SY_TWO_PASS_FROM below): from there on
// two capi_dtrmm_thin passes over the same triangle and a correction of the diagonal measured faster, and the call runs those.
// The two products want the tile in the two operand forms of thin_tile.h (row dots for U X, column dots for U^T X).  The tile is LOADED TWICE, once
// in each form, one behind the other: the second load finds the lines of the first in flight or in L2, not in HBM.  An LDS transpose and lane
// permutes are not built.
// A workgroup of 8 waves walks its block in super-tiles of 256 x 256, column of super-tiles by column.  Inside one, wave w owns the row strip
// 32 w.. and takes the column strips (w + t) mod 8, t = 0..7:
//   U X_J    accumulates in registers over the 8 steps, then into the block's row slot (read-modify-write by the one wave that owns the strip)
//   U^T X_I  goes to an LDS image of the 256 columns after every step: the 8 waves are on 8 different strips, a barrier separates the steps, so
//            a strip receives its terms in a fixed order; the image goes to the block's column slot when the column of super-tiles is done
// X_J (256 x 16) stays in LDS for a column of super-tiles, X_I is double-buffered per super-tile; A's pieces are double-buffered in registers, one
// step ahead (one loop body: the prefetched set is moved, not a second copy of the body with the sets swapped -- that copy spilt 300 VGPRs).
// A second launch (sym_combine_kernel) adds the p + 1 slots of every line block in a fixed order, subtracts from B (adds |B|) and forms the squared
// norms (the maxima) per 256 lines, a third adds those in order: no floating-point atomics, the same bits on every run.  sym_fused is the host's
// side of both calls.
// Edges (ragged blocks, the tiles the diagonal crosses): every element from a clamped address, selected afterwards (never multiplied by zero):
// the diagonal tile gives row <= col to U X and row < col to U^T X.  Columns are loaded 16 bytes at a time from 8-byte-aligned addresses (d2u_t).
#include "capi_internal.h"
#include "sym_thin_plan.h"
#include "thin_tile.h"

namespace {

namespace sp = sym_thin_plan;
namespace tt = thin_tile;
using tt::d2_t;
using tt::d2u_t;
using tt::d4_t;

constexpr int SY_THREADS = 512;                 // 8 waves, one workgroup per CU
constexpr int SY_NP = 8;                        // 16-byte pieces of a tile per lane and operand form
constexpr int SY_IMG = sp::SUPER * sp::RPAD;    // doubles of one LDS image: 256 lines x 16 columns
constexpr size_t SY_LDS = sizeof(double) * 4 * SY_IMG;   // X_J, X_I twice, the column sums: 128 KiB

struct SymArgs {
  const double* A; const double* X; double* slab;
  int64_t lda, ldx;
  int r;
  sp::Plan P;
};

// ABS: |U| |X| instead of U X (capi_dsym_abs): the thin operand loses its signs on the way into LDS, a tile's pieces just before they are multiplied.
// The ABS == false instantiation is the kernel as it was, instruction for instruction
template <bool ABS>
__global__ __launch_bounds__(SY_THREADS) void resid_sym_kernel(const SymArgs p) {
  extern __shared__ __attribute__((aligned(16))) double Ls[];   // [4][256][16]: X_J(k, j), X_I(k, j) twice, (U^T X_I)(col, j)
  double* const XJ = Ls;
  double* const XI = Ls + SY_IMG;
  double* const P2 = Ls + 3 * SY_IMG;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15, g4 = lane >> 4;
  int I, J;
  sp::block_of((int)blockIdx.x, &I, &J);
  const bool diag = I == J;
  const int64_t n = p.P.n, bs = p.P.bs;
  const int64_t r0 = sp::line0(p.P, I), r1 = sp::line1(p.P, I), c0 = sp::line0(p.P, J), c1 = sp::line1(p.P, J);
  const int nsr = (int)sp::cdiv64(r1 - r0, sp::SUPER), nsc = (int)sp::cdiv64(c1 - c0, sp::SUPER);
  const int total = 8 * (diag ? nsc * (nsc + 1) / 2 : nsr * nsc);            // steps: 8 per super-tile
  double* const slab1 = p.slab + (int64_t)sp::slot_of(I, J, 0) * sp::slot_doubles(p.P);
  double* const slab2 = p.slab + (int64_t)sp::slot_of(I, J, 1) * sp::slot_doubles(p.P);
  auto last_row = [&](int C) { return diag ? C : nsr - 1; };                 // the last super-tile of column C

  // ---- the thin operand: thread t fetches line t & 255 of columns (t >> 8) + 2 q ----
  const int fk = tid & (sp::SUPER - 1), fj = tid >> 8;
  double xst[8];
  auto xload = [&](int64_t k0) {
    const int64_t k = k0 + fk;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int j = fj + 2 * q;
      const bool in = k < n && j < p.r;
      xst[q] = *(in ? p.X + k + (int64_t)j * p.ldx : p.X);
    }
  };
  auto xstore = [&](double* L, int64_t k0) {
    const int64_t k = k0 + fk;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int j = fj + 2 * q;
      L[fk * 16 + j] = (k < n && j < p.r) ? (ABS ? fabs(xst[q]) : xst[q]) : 0.0;
    }
  };

  // ---- the tile of wave w at step t of super-tile (R, C): rows row0.., columns col0.. ----
  auto origin = [&](int C, int R, int t, int64_t* row0, int64_t* col0) {
    *row0 = r0 + (int64_t)R * sp::SUPER + 32 * w;
    *col0 = c0 + (int64_t)C * sp::SUPER + 32 * ((w + t) & 7);
  };
  // wave-uniform: the tile holds something / is whole and strictly above the diagonal
  auto live = [&](int C, int R, int t) {
    int64_t row0, col0;
    origin(C, R, t, &row0, &col0);
    return row0 < r1 && col0 < c1 && (!diag || row0 <= col0);
  };
  auto steady = [&](int C, int R, int t) {
    int64_t row0, col0;
    origin(C, R, t, &row0, &col0);
    return row0 + 32 <= r1 && col0 + 32 <= c1 && (!diag || row0 < col0);
  };
  // form N (na): the row-dot pieces; form T (ta): the column-dot pieces.  A lane's place inside the tile is a 32-bit offset from the tile's first
  // element, which is wave-uniform: one address register per lane
  const uint32_t ld32 = (uint32_t)p.lda;
  const uint32_t offn = (uint32_t)g4 * ld32 + 2 * (uint32_t)l16, offt = (uint32_t)l16 * ld32 + 2 * (uint32_t)g4;
  auto load_steady = [&](int C, int R, int t, d2_t (&na)[SY_NP], d2_t (&ta)[SY_NP]) {
    int64_t row0, col0;
    origin(C, R, t, &row0, &col0);
    const double* tb = p.A + col0 * p.lda + row0;
#pragma unroll
    for (int q = 0; q < SY_NP; ++q) na[q] = *(const d2u_t*)(tb + (int64_t)(4 * q) * p.lda + offn);
#pragma unroll
    for (int q = 0; q < SY_NP; ++q) ta[q] = __builtin_nontemporal_load((const d2u_t*)(tb + (int64_t)(16 * (q >> 2)) * p.lda + 8 * (q & 3) + offt));
  };
  auto load_edge = [&](int C, int R, int t, d2_t (&na)[SY_NP], d2_t (&ta)[SY_NP]) {
    int64_t row0, col0;
    origin(C, R, t, &row0, &col0);
    const double* tb = p.A + col0 * p.lda + row0;                        // the tile's first element: inside the block, on or above the diagonal
    const int rows = (int)sp::min64(32, r1 - row0), cols = (int)sp::min64(32, c1 - col0);
    const int dg = diag ? (int)(col0 - row0) : 64;                       // row <= col  <=>  i <= j + dg in the tile's own indices
#pragma unroll
    for (int q = 0; q < SY_NP; ++q) {
      const int i = 2 * l16, j = 4 * q + g4;
      const bool v0 = i < rows && j < cols && i <= j + dg, v1 = i + 1 < rows && j < cols && i + 1 <= j + dg;       // U X: the diagonal takes part
      const uint32_t o = (uint32_t)j * ld32 + (uint32_t)i;
      const double x = tb[v0 ? o : 0u], y = tb[v1 ? o + 1u : 0u];
      na[q] = (d2_t){v0 ? x : 0.0, v1 ? y : 0.0};
    }
#pragma unroll
    for (int q = 0; q < SY_NP; ++q) {
      const int i = 8 * (q & 3) + 2 * g4, j = 16 * (q >> 2) + l16;
      const bool v0 = i < rows && j < cols && i < j + dg, v1 = i + 1 < rows && j < cols && i + 1 < j + dg;         // U^T X: it does not
      const uint32_t o = (uint32_t)j * ld32 + (uint32_t)i;
      const double x = tb[v0 ? o : 0u], y = tb[v1 ? o + 1u : 0u];
      ta[q] = (d2_t){v0 ? x : 0.0, v1 ? y : 0.0};
    }
  };

  d4_t acc1[2][1];                       // (U X_J)(row0 + 2 l16 + h, g4 + 4 reg)
  int par = 0;
  // one step: prefetch the following step's pieces (a whole tile's), multiply this one's
  auto step = [&](int C, int R, int t, d2_t (&na)[SY_NP], d2_t (&ta)[SY_NP], d2_t (&nna)[SY_NP], d2_t (&nta)[SY_NP], int nC, int nR, int nt,
                  bool has_next) {
    // an edge tile is fetched where it is used, not a step ahead: its selects beside a second set of pieces cost spills, and the blocks
    // that hold edge tiles (the diagonal's, the ragged last ones) are the short ones
    if (live(C, R, t) && !steady(C, R, t)) load_edge(C, R, t, na, ta);
    if (has_next && live(nC, nR, nt) && steady(nC, nR, nt)) load_steady(nC, nR, nt, nna, nta);
    const bool tile_end = t == 7, col_end = tile_end && R == last_row(C);     // workgroup-uniform
    if (t == 0) { acc1[0][0] = (d4_t){0.0, 0.0, 0.0, 0.0}; acc1[1][0] = (d4_t){0.0, 0.0, 0.0, 0.0}; }
    if (tile_end && !col_end) xload(r0 + (int64_t)(R + 1) * sp::SUPER);
    const int c = (w + t) & 7;
    if (live(C, R, t)) {
      d4_t acc2[2][1] = {{(d4_t){0.0, 0.0, 0.0, 0.0}}, {(d4_t){0.0, 0.0, 0.0, 0.0}}};   // (U^T X_I)(col0 + 16 s + g4 + 4 reg, l16)
      if constexpr (ABS) {
        // here, not where the pieces are loaded: the prefetched set must stay in flight over the step before
#pragma unroll
        for (int q = 0; q < SY_NP; ++q) { na[q] = __builtin_elementwise_abs(na[q]); ta[q] = __builtin_elementwise_abs(ta[q]); }
      }
      __builtin_amdgcn_s_setprio(1);
      tt::mfma_row_dots<1>(acc1, XJ + (32 * c + g4) * 16 + l16, 0, na);
      tt::mfma_col_dots<1>(acc2, XI + par * SY_IMG + (32 * w + 2 * g4) * 16 + l16, 0, ta);
      __builtin_amdgcn_s_setprio(0);
      double* pc = P2 + (32 * c + g4) * 16 + l16;
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) pc[(16 * s + 4 * reg) * 16] += acc2[s][0][reg];
    }
    if (tile_end && r0 + (int64_t)R * sp::SUPER + 32 * w < r1) {
      // the strip's sums over this super-tile join those of the columns before it: only this wave touches these lines of the row slot
      const bool first = C == (diag ? R : 0);
      double* sl = slab1 + (int64_t)R * sp::SUPER + 32 * w + 2 * l16;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        d2_t v = {acc1[0][0][reg], acc1[1][0][reg]};
        d2_t* dst = (d2_t*)(sl + (int64_t)(g4 + 4 * reg) * bs);
        if (!first) v += *dst;
        *dst = v;
      }
    }
    if (tile_end && !col_end) xstore(XI + (par ^ 1) * SY_IMG, r0 + (int64_t)(R + 1) * sp::SUPER);
    __syncthreads();
    if (tile_end && !col_end) par ^= 1;
    if (col_end) {
      // the column sums of this column of super-tiles: to the column slot, and zero again
      for (int e = tid; e < SY_IMG; e += SY_THREADS) {
        const int i = e & (sp::SUPER - 1), j = e >> 8;
        const int64_t x = (int64_t)C * sp::SUPER + i;
        if (x < bs) slab2[(int64_t)j * bs + x] = P2[i * 16 + j];
        P2[i * 16 + j] = 0.0;
      }
      if (has_next) {
        xload(c0 + (int64_t)(C + 1) * sp::SUPER);
        xstore(XJ, c0 + (int64_t)(C + 1) * sp::SUPER);
        xload(r0);
        xstore(XI + par * SY_IMG, r0);
      }
      __syncthreads();
    }
  };

  for (int e = tid; e < SY_IMG; e += SY_THREADS) P2[e] = 0.0;
  xload(c0);
  xstore(XJ, c0);
  xload(r0);
  xstore(XI, r0);
  d2_t na[SY_NP], ta[SY_NP], nna[SY_NP], nta[SY_NP];
  if (live(0, 0, 0) && steady(0, 0, 0)) load_steady(0, 0, 0, na, ta);
  __syncthreads();
  int C = 0, R = 0, t = 0;
  for (int q = 0; q < total; ++q) {
    int nC = C, nR = R, nt = t + 1;
    if (nt == 8) { nt = 0; if (++nR > last_row(C)) { nR = 0; ++nC; } }
    step(C, R, t, na, ta, nna, nta, nC, nR, nt, q + 1 < total);
#pragma unroll
    for (int i = 0; i < SY_NP; ++i) { na[i] = nna[i]; ta[i] = nta[i]; }
    C = nC; R = nR; t = nt;
  }
}

struct SymCombineArgs {
  const double* slab; const double* B; double* out; double* part;
  int64_t ldb, ldo;
  int r;
  sp::Plan P;
};

// sum(l, j): the p + 1 slots of l's line block, in the plan's order.  With the group's 256 lines:
//   ABS == false (capi_dresid_sym)   out(l, j) = B(l, j) - sum,    part[group][j] = the squared norms, sp::RPAD columns per group
//   ABS == true  (capi_dsym_abs)     out(l, j) = sum + |B(l, j)|,  part[group][j] = the largest, CAPI_TS_MAX_RHS columns per group; B may be null
template <bool ABS> constexpr int SY_PART_STRIDE = ABS ? (int)CAPI_TS_MAX_RHS : sp::RPAD;
template <bool ABS>
__global__ __launch_bounds__(sp::SUPER) void sym_combine_kernel(const SymCombineArgs p) {
  const int64_t l = (int64_t)blockIdx.x * sp::SUPER + threadIdx.x;
  const bool in = l < p.P.n;
  const int L = in ? (int)(l / p.P.bs) : 0;
  const int64_t x = in ? l - (int64_t)L * p.P.bs : 0, sd = sp::slot_doubles(p.P);
  auto value = [&](int j) {
    if (!in) return 0.0;
    double sum = 0.0;
    for (int k = 0; k <= p.P.p; ++k) sum += p.slab[(int64_t)sp::contribution(p.P, L, k) * sd + (int64_t)j * p.P.bs + x];
    double v;
    if constexpr (ABS) v = p.B ? sum + fabs(p.B[l + (int64_t)j * p.ldb]) : sum;
    else v = p.B[l + (int64_t)j * p.ldb] - sum;
    if (p.out) p.out[l + (int64_t)j * p.ldo] = v;
    return v;
  };
  if constexpr (ABS) tt::group_colmax<sp::RPAD, sp::SUPER>(p.r, p.part, SY_PART_STRIDE<ABS>, value);
  else tt::group_colnorms<sp::RPAD, sp::SUPER>(p.r, p.part, SY_PART_STRIDE<ABS>, value);
}

// the two-pass route's last step: W = U X + U^T X counted the diagonal twice.  Rout(l, j) = B(l, j) - (W(l, j) - A(l, l) X(l, j)); part as above,
// CAPI_TS_MAX_RHS columns per group
__global__ __launch_bounds__(sp::SUPER) void resid_sym_finish_kernel(const double* __restrict__ W, const double* __restrict__ A, int64_t lda,
                                                                     const double* __restrict__ X, int64_t ldx, const double* B, int64_t ldb, double* R,
                                                                     int64_t ldr, double* __restrict__ part, int64_t n, int r) {
  const int64_t l = (int64_t)blockIdx.x * sp::SUPER + threadIdx.x;
  const bool in = l < n;
  const double d = in ? A[l + l * lda] : 0.0;
  tt::group_colnorms<CAPI_TS_MAX_RHS, sp::SUPER>(r, part, CAPI_TS_MAX_RHS, [&](int j) {
    if (!in) return 0.0;
    const double v = B[l + (int64_t)j * ldb] - (W[l + (int64_t)j * n] - d * X[l + (int64_t)j * ldx]);
    if (R) R[l + (int64_t)j * ldr] = v;
    return v;
  });
}

// From this many columns on the call takes the two-pass route: capi_dtrmm_thin NOTRANS and TRANS over the same triangle (read twice), then the
// diagonal's correction.  Measured (profiles/resid_sym.txt): the fused kernel ties with it at r = 1 and loses at r = 8 (4 % at n = 32768, 8 % at
// 16384) and at r = 32 (1.4 x: it needs two passes of 16 columns itself); between 1 and 8 nothing is measured.
constexpr int SY_TWO_PASS_FROM = 8;

// The fused route of both calls, n > 0: slabs and the groups' parts in the first workspace block, resid_sym_kernel<ABS> and its combine for 16 columns
// (sym_thin_plan::RPAD) a pass (the triangle is read once per pass, the slab reused in stream order), the parts' sum or maximum into col (may be null)
template <bool ABS>
int sym_fused(capi_handle_t h, int64_t n, int64_t r, const double* A, int64_t lda, const double* X, int64_t ldx, const double* B, int64_t ldb, double* out,
              int64_t ldo, double* col) {
  constexpr int STRIDE = SY_PART_STRIDE<ABS>;
  const int64_t groups = cdiv(n, sp::SUPER);
  const sp::Plan P = sp::make_plan(n, capi_stream_cus(h));
  void* pv = nullptr;
  const int rc = capi_ws_get(h, sizeof(double) * (size_t)(sp::slab_doubles(P) + groups * STRIDE), &pv);
  if (rc != CAPI_OK) return rc;
  double* slab = (double*)pv;
  double* part = slab + sp::slab_doubles(P);
  CAPI_RAISE_LDS_LIMIT(h, ABS ? CAPI_ATTR_SYM_ABS : CAPI_ATTR_RESID_SYM, resid_sym_kernel<ABS>, SY_LDS);
  for (int64_t j0 = 0; j0 < r; j0 += sp::RPAD) {
    const int rp = (int)sp::min64(sp::RPAD, r - j0);
    const SymArgs p{A, X + j0 * ldx, slab, lda, ldx, rp, P};
    hipLaunchKernelGGL(resid_sym_kernel<ABS>, dim3((unsigned)sp::num_blocks(P)), dim3(SY_THREADS), SY_LDS, h->stream, p);
    const SymCombineArgs cp{slab, B ? B + j0 * ldb : nullptr, out ? out + j0 * ldo : nullptr, col ? part + j0 : nullptr, ldb, ldo, rp, P};
    hipLaunchKernelGGL(sym_combine_kernel<ABS>, dim3((unsigned)groups), dim3(sp::SUPER), 0, h->stream, cp);
  }
  if (col) {
    if (ABS) hipLaunchKernelGGL(tt::colmax_kernel<>, dim3(1), dim3(64), 0, h->stream, (const double*)part, groups, STRIDE, (int)r, col);
    else hipLaunchKernelGGL(tt::colnorms_kernel<>, dim3(1), dim3(64), 0, h->stream, (const double*)part, groups, STRIDE, (int)r, col);
  }
  CAPI_HIP_CHECK(h, hipGetLastError());
  return CAPI_OK;
}

}  // namespace

extern "C" {

int capi_dresid_sym(capi_handle_t h, int64_t n, int64_t r, const double* A, int64_t lda, const double* X, int64_t ldx, const double* B, int64_t ldb,
                    double* Rout, int64_t ldr, double* colnorm2) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE_THIN_R(h, r);
  CAPI_REQUIRE(h, n >= 0 && n < (1LL << 31) && lda < (1LL << 24), "n / lda (lda < 2^24: 32 columns are addressed by 32-bit byte offsets)");
  CAPI_REQUIRE(h, n == 0 || (A && X && B && lda >= n && ldx >= n && ldb >= n && (!Rout || ldr >= n)), "A/lda/X/ldx/B/ldb/Rout/ldr");
  CAPI_REQUIRE(h, !Rout || Rout != X, "Rout must not alias X");
  if (n == 0) {
    if (colnorm2) hipLaunchKernelGGL(tt::colnorms_kernel<>, dim3(1), dim3(64), 0, h->stream, (const double*)nullptr, (int64_t)0, sp::RPAD, (int)r, colnorm2);
    CAPI_HIP_CHECK(h, hipGetLastError());
    return CAPI_OK;
  }
  const int64_t groups = cdiv(n, sp::SUPER);
  if (r >= SY_TWO_PASS_FROM) {
    // W (n x r) and the norms' partial sums lie in the second workspace block: capi_dtrmm_thin keeps its slabs in the first
    void* pw = nullptr;
    int rc = capi_ws2_get(h, sizeof(double) * (size_t)(n * r + groups * CAPI_TS_MAX_RHS), &pw);
    if (rc != CAPI_OK) return rc;
    double* W = (double*)pw;
    double* part = W + n * r;
    rc = capi_dtrmm_thin(h, CAPI_UPPERTRI, CAPI_NOTRANS, n, n, r, 1.0, A, lda, 0, X, ldx, 0.0, W, n);
    if (rc != CAPI_OK) return rc;
    rc = capi_dtrmm_thin(h, CAPI_UPPERTRI, CAPI_TRANS, n, n, r, 1.0, A, lda, 0, X, ldx, 1.0, W, n);
    if (rc != CAPI_OK) return rc;
    hipLaunchKernelGGL(resid_sym_finish_kernel, dim3((unsigned)groups), dim3(sp::SUPER), 0, h->stream, (const double*)W, A, lda, X, ldx, B, ldb, Rout, ldr,
                       colnorm2 ? part : (double*)nullptr, n, (int)r);
    if (colnorm2) hipLaunchKernelGGL(tt::colnorms_kernel<>, dim3(1), dim3(64), 0, h->stream, (const double*)part, groups, (int)CAPI_TS_MAX_RHS, (int)r, colnorm2);
    CAPI_HIP_CHECK(h, hipGetLastError());
    return CAPI_OK;
  }
  return sym_fused<false>(h, n, r, A, lda, X, ldx, B, ldb, Rout, ldr, colnorm2);
}

int capi_dsym_abs(capi_handle_t h, int64_t n, int64_t r, const double* A, int64_t lda, const double* X, int64_t ldx, const double* B, int64_t ldb,
                  double* W, int64_t ldw, double* colmax) {
  CAPI_REQUIRE(h, h, "null handle");
  CAPI_REQUIRE_THIN_R(h, r);
  CAPI_REQUIRE(h, n >= 0 && n < (1LL << 31) && lda < (1LL << 24), "n / lda (lda < 2^24: 32 columns are addressed by 32-bit byte offsets)");
  CAPI_REQUIRE(h, n == 0 || (A && X && lda >= n && ldx >= n && (!B || ldb >= n) && (!W || ldw >= n)), "A/lda/X/ldx/B/ldb/W/ldw");
  CAPI_REQUIRE(h, !W || W != X, "W must not alias X");
  if (n == 0) {
    if (colmax) hipLaunchKernelGGL(tt::colmax_kernel<>, dim3(1), dim3(64), 0, h->stream, (const double*)nullptr, (int64_t)0, (int)CAPI_TS_MAX_RHS, (int)r, colmax);
    CAPI_HIP_CHECK(h, hipGetLastError());
    return CAPI_OK;
  }
  return sym_fused<true>(h, n, r, A, lda, X, ldx, B, ldb, W, ldw, colmax);
}

}  // extern "C"
