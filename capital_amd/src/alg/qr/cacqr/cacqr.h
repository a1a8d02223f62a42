// alg/qr/cacqr/cacqr.h -- communication-avoiding CholeskyQR / CholeskyQR2 on MI355X
// (reference src/alg/qr/cacqr/cacqr.h:13-78, cacqr.hpp:7-29,174-193,219-270).
//
// Same call surface: cacqr<SerializePolicy,IntermediatesPolicy>::factor(A, args, rectTopo), construct_Q / construct_R,
// info<T,U,CholeskyInversionType>(num_iter, ci_args).  c == 1 is the 1-D variant (BASELINE configs 3 and 5, the hot path);
// c == d is the 3-D variant on a cubic grid (sweep_3d below); 1 < c < d with c | d the tunable grid (d/c cubes, sweep_tune).  1-D, per sweep (cacqr.hpp:7-29):
//     K7  G = Q^T Q            capi_dsyrk, split-K over the tall dimension, upper triangle only
//     C8  G = sum over ranks   capi_allreduce_sum over `world` (packed n(n+1)/2 doubles with Serialize)
//     K8+K9  R = chol(G), R^-1 capi_dpotrf_trtri, replicated on every GPU
//     K5  Q <- Q R^-1          capi_dtrmm_oop (right, upper), out of place into the block's second buffer
// CholeskyQR2 runs the sweep twice and combines R = R2 R1 (cacqr.hpp:181-189, K6).
// Beyond the reference (its sweep has no shift; CholeskyQR2 breaks down at kappa(A) ~ 1e8): info::num_iter is the total number of sweeps,
// 1..4, R = R_k ... R_2 R_1, and the first info::num_shifted of them are SHIFTED sweeps (shifted CholeskyQR, Fukaya et al., SIAM J. Sci.
// Comput. 42, 2020; 1-D variant only).  A shifted sweep differs from a plain one only around K8+K9: the reduced Gram matrix is column-
// equilibrated by powers of two and shifted, G' = D^-1 G D^-1 + s I with s = shift_scale * 11 (m n + n (n + 1)) u trace(D^-1 G D^-1), m the
// global row count (capi_dgram_equilibrate_shift), factored, and R = R' D, R^-1 = D^-1 R'^-1 (capi_dtri_rescale).  Its factorisation cannot
// break down, and the panel it leaves has cond ~ sqrt(s) kappa(A): one shifted sweep serves kappa(A) up to ~1e10, two up to ~1e12.
// The shifted sweeps precondition, the plain ones orthogonalise: num_iter - num_shifted >= 2 is what gives an orthogonal Q (with fewer
// plain sweeps Q R = A still holds, Q^T Q = I does not).  s is computed after the all-reduce from identical bits in a fixed order, so
// R stays bit-identical across the ranks.
// Also beyond the reference (its cacqr.hpp stops at Q and R): least_squares(A, B, args, topo) after factor() solves min ||A X - B||_F for the
// r columns of B as X = R^-1 (Q^T B) on the resident factors (1-D variant only), and returns the residual norms ||b_j - A x_j||_2:
//     C = Q^T B              capi_dgemtn_ts on the local rows, <= CAPI_TS_MAX_RHS columns per call: a streaming kernel with an n x r output
//                            (capi_dgemm(T, N) instead on tall panels of width >= 256: see least_squares)
//     C = sum over ranks     capi_allreduce_sum over `world` (n r doubles), as the Gram matrix
//     X = R^-1 C             capi_dtrsm on a full-storage image of R, replicated: identical bits in, identical bits out on every rank
//     ||b_j - A x_j||^2      capi_dresid_ts on A (not Q), r doubles all-reduced, square roots on the host
// No m x n temporary: the new device memory is B, X and the n x n image of R (the Gram work block, re-registered when the policy released it).
// And svd(args, topo, left) after factor(): the singular values and vectors of A from the resident pair, A = Q R = (Q U_R) Sigma V^T (1-D variant only):
//     R = U_R Sigma V^T      capi_dgesvj on a full-storage image of R: one-sided Jacobi on the device, deterministic, so that every rank computes the
//                            same bits from its replicated R and nothing is communicated
//     U = Q U_R              capi_dgemm on the local rows (left == true only)
// New device memory: Sigma (n), V and U_R (n x n each) and, with left, U: ONE new m_loc x n block.  With left == false no m x n memory is touched.
// And factor_pivoted(A, args, topo) beside factor(): a column-pivoted CholeskyQR for panels whose columns are linearly dependent, A P = Q R with Q
// m x k orthonormal, R k x n upper trapezoidal and k the numerical rank -- dgeqp3 / dgelsy semantics on the CholeskyQR scheme (1-D variant only):
//     G = A^T A, all-reduced     exactly as in a plain sweep
//     P^T G P = R^T R + (0, S)   capi_dpstrf in capi_dpotrf_trtri's place: Cholesky with diagonal pivoting, stopped at rank k where the largest
//                                remaining Schur diagonal is <= tol trace(G), tol = pivot_tol_scale max(pivot_rtol^2, 11 (m n + n (n + 1)) u) -- the
//                                floor is the factor of the shift a shifted sweep would add: a column is dropped when, after projecting out the
//                                accepted ones, its squared norm is at most that shift.  Replicated: every rank computes the same bits
//     M = P(:, 0:k) R11^-1       capi_dtrtri on a copy of the leading block, capi_drow_scatter (n x k)
//     Q1 = A M                   capi_dgemm, m_loc x n x k: dense where a plain sweep's product is triangular
//     Q = Q1 R2^-1               one plain sweep on the m_loc x k panel
//     Rp(0:k, :) = R2 [R11 R12]  capi_dtrmm_oop (left, upper); rows >= k of Rp are zero
// so that A(:, piv[j]) = Q Rp(:, j) up to ||A P - Q R||_F <= sqrt((n - k) tol trace(G)) plus rounding.  The resolution is the Gram matrix's own noise
// level: relative to ||A||_F the rank threshold is sqrt(tol), about 1e-5 at 2048 x 32 and about 1e-3 at 2^22 x 256 -- a singular value below that
// cannot be told from zero here, where dgeqp3 on A itself resolves down to u.  pivot_rtol above the floor gives a truncated pivoted QR, a low-rank
// approximation with that error bound.  least_squares() after it returns the BASIC solution: X = P [R11^-1 (Q^T B); 0], zeros in the dropped
// columns (not the minimum-norm one); svd() after it refuses.
// Underneath, the A -> Q copy of factor() (cacqr.hpp:226) is folded into the first sweep (it reads A, writes Q) and the
// second sweep ping-pongs between Q's data and scratch buffers, so every sweep streams the panel exactly twice
// (read for the Gram, read+write for the solve) with no in-place hazard.
#ifndef CAPITAL_QR_CACQR_H_
#define CAPITAL_QR_CACQR_H_

#include "./../../alg.h"
#include "./../../matmult/summa/summa.h"
#include "./../../cholesky/cholinv/cholinv.h"
#include "./policy.h"

// The two entry points of the shifted sweep are weak references: a stand-in of the C-ABI that does not have them (the CPU rehearsal
// shim of the test suite) still links and loads, every other path runs on it, and invoke_1d refuses num_shifted > 0 there.
#pragma weak capi_dgram_equilibrate_shift
#pragma weak capi_dtri_rescale
// likewise the two streaming kernels of least_squares: without them factor() runs as before and least_squares refuses
#pragma weak capi_dgemtn_ts
#pragma weak capi_dresid_ts
// and the device SVD of R under svd
#pragma weak capi_dgesvj
// and the pivoted Cholesky and the permutation kernel under factor_pivoted
#pragma weak capi_dpstrf
#pragma weak capi_drow_scatter

namespace qr {

template <class SerializePolicy = policy::cacqr::Serialize, class IntermediatesPolicy = policy::cacqr::SaveIntermediates>
class cacqr : public SerializePolicy, public IntermediatesPolicy {
public:
  using SP = SerializePolicy;
  using IP = IntermediatesPolicy;

  template <typename ScalarT, typename DimensionT, typename CholeskyInversionType>
  class info {
  public:
    using ScalarType = ScalarT;
    using DimensionType = DimensionT;
    using alg_type = cacqr<SerializePolicy, IntermediatesPolicy>;
    using cholesky_inverse_type = CholeskyInversionType;
    template <typename CholeskyInversionArgType>
    info(size_t num_iter, CholeskyInversionArgType&& ci_args) : num_iter(num_iter), cholesky_inverse_args(std::forward<CholeskyInversionArgType>(ci_args)) {}
    info(const info& p) : num_iter(p.num_iter), num_shifted(p.num_shifted), shift_scale(p.shift_scale), cholesky_inverse_args(p.cholesky_inverse_args),
                          pivot_rtol(p.pivot_rtol), pivot_tol_scale(p.pivot_tol_scale) {}
    const size_t num_iter;                                                       // 1: CholeskyQR, 2: CholeskyQR2 (bench/qr/cacqr.cpp:14,40); up to 4 sweeps
    size_t num_shifted = 0;                                                      // the first num_shifted sweeps are shifted (1-D variant); see the file comment
    double shift_scale = 1.0;                                                    // multiplies the published shift 11 (m n + n (n + 1)) u ||A D^-1||_F^2
    typename CholeskyInversionType::template info<ScalarType, DimensionType> cholesky_inverse_args;
    matrix<ScalarType, DimensionType, rect> Q;
    matrix<ScalarType, DimensionType, typename SerializePolicy::structure> R;
    // n x n work blocks (Gram/R of the current sweep, its inverse, R1 of the first sweep, packed transfer image)
    matrix<ScalarType, DimensionType, rect> G, Ginv, R1;
    matrix<ScalarType, DimensionType, uppertri> Gpacked;
    // LAPACK info of the Gram matrix's factorisation (1-D variant): 0, or the first non-positive pivot (1-based) -- CholeskyQR's
    // known failure mode is a numerically rank-deficient A^T A (kappa(A) beyond ~1e8).  factor() throws std::domain_error then.
    int potrf_info = 0;
    // per-sweep diagnostics of a run with num_shifted > 0, read back with potrf_info (one synchronisation, behind the launch chain):
    // sweep_shift[k] = s and sweep_trace[k] = trace(D^-1 G D^-1) of a shifted sweep (0 for a plain one);
    // sweep_cond_bound[k] = ||R'||_1 ||R'||_inf ||R'^-1||_1 ||R'^-1||_inf of the sweep's (equilibrated, shifted) Gram matrix G' = R'^T R':
    // cond_2(G') <= sweep_cond_bound[k] <= n^2 cond_2(G'), and 1 for an orthonormal panel.  The Gram matrix of a SHIFTED sweep is capped near
    // trace / s ~ 1 / (11 (m n + n^2) u) whatever kappa(A) is; the figure to watch is that of the first PLAIN sweep, a bound on the squared
    // condition of the panel the shifted sweeps left: below ~1e15 that sweep is safe, above ~1e16 n^2 it cannot succeed and one more shifted
    // sweep is needed; in between the bound does not decide (DESIGN.md section 2a has measured values).
    std::vector<double> sweep_shift, sweep_trace, sweep_cond_bound;
    matrix<ScalarType, DimensionType, rect> Dscale, SweepRec;                    // device: n column scales; 4 doubles per sweep
    // least_squares: the solution X (n x r, replicated on every rank), ||b_j - A x_j||_2 per right-hand side (empty when not asked for);
    // factored: the last factor() came back with valid Q and R
    matrix<ScalarType, DimensionType, rect> X, LsNorm2;
    std::vector<double> ls_residual_norms;
    bool factored = false;
    // svd: A = U diag(singular_values) V^T.  Sigma (n, device) and V (n x n) are replicated on every rank, bit for bit; U (m_loc x n, this rank's
    // rows, with left == true) = Q UR; svd_sweeps = the Jacobi sweeps capi_dgesvj ran; cond2 = sigma_1 / sigma_n
    matrix<ScalarType, DimensionType, rect> U, Sigma, V, UR;
    std::vector<double> singular_values;
    int svd_sweeps = 0;
    double cond2 = 0.0;
    // factor_pivoted: tol = pivot_tol_scale * max(pivot_rtol^2, 11 (m n + n (n + 1)) u) (pivot_rtol: the user's tolerance relative to ||A||_F, 0 = the
    // floor alone).  rank = the numerical rank k; piv (host) / Piv (device: n ints in the first (n + 1) / 2 doubles): column j of A P is column piv[j] of A;
    // Rp (n x n): rows < rank hold R, the rest is zero; Q's first rank columns are the orthonormal factor; pivot_tol: the tol that
    // went into capi_dpstrf (thresh = pivot_tol trace(A^T A)); pivoted: the resident factors are factor_pivoted's (factor() clears it)
    double pivot_rtol = 0.0, pivot_tol_scale = 1.0, pivot_tol = 0.0;
    int64_t rank = 0;
    std::vector<int> piv;
    matrix<ScalarType, DimensionType, rect> Piv, Rp;
    bool pivoted = false;
  };

  template <typename MatrixType, typename ArgType, typename CommType>
  static void factor(const MatrixType& A, ArgType& args, CommType&& CommInfo) {
    static_assert(std::is_same<typename MatrixType::StructureType, rect>::value, "qr::cacqr requires matrices of rect structure");
    const auto gN = A.num_columns_global(), gM = A.num_rows_global();
    args.factored = false;
    args.Q._register_(gN, gM, CommInfo.c, CommInfo.d);
    args.R._register_(gN, gN, CommInfo.c, CommInfo.c);
    if (CommInfo.c == 1) {
      invoke_1d(A, args, CommInfo);
    } else if (args.num_shifted > 0) {
      // the Gram block is element-cyclic on these grids: its diagonal and its trace live on different ranks
      throw std::logic_error("qr::cacqr: shifted sweeps (num_shifted > 0) are built for the 1-D variant (c == 1) only");
    } else if (CommInfo.d % CommInfo.c == 0) {
      // c == d: one cube (sweep_3d); c < d: d/c cubes side by side (sweep_tune, cacqr.hpp:124-170) -- the same sweep per cube
      // plus one all-reduce of the Gram block across the cubes
      invoke_3d(A, args, CommInfo);
    } else {
      throw std::logic_error("qr::cacqr: the c x d x c grid needs c to divide d");
    }
    if (!IP::keep_work) { args.G._destroy_(); args.Ginv._destroy_(); args.R1._destroy_(); args.Gpacked._destroy_(); args.Dscale._destroy_(); args.SweepRec._destroy_(); }
    args.factored = true;
  }

  // Column-pivoted CholeskyQR of a panel that may be rank deficient: args.rank = k, args.piv / args.Piv, the m_loc x k orthonormal factor in the
  // first k columns of args.Q and the k x n trapezoid in args.Rp, A(:, piv[j]) = Q Rp(:, j).  See the file comment.  std::domain_error when the
  // numerical rank is 0 (A is zero or not finite) or the plain sweep on the rank-k panel breaks down.
  template <typename MatrixType, typename ArgType, typename CommType>
  static void factor_pivoted(const MatrixType& A, ArgType& args, CommType&& CommInfo) {
    static_assert(std::is_same<typename MatrixType::StructureType, rect>::value, "qr::cacqr requires matrices of rect structure");
    using Dim = typename MatrixType::DimensionType;
    if (CommInfo.c != 1) throw std::logic_error("qr::cacqr::factor_pivoted is built for the 1-D variant (c == 1) only");
    if (!&capi_dpstrf || !&capi_drow_scatter)
      throw std::logic_error("qr::cacqr: this C-ABI library has no capi_dpstrf / capi_drow_scatter: no pivoted factorization");
    const int64_t n = A.num_columns_global(), m_loc = A.num_rows_local(), m_glob = A.num_rows_global();
    if (n < 1 || n > 2048) throw std::invalid_argument("qr::cacqr::factor_pivoted: 1 <= n <= 2048 columns (capi_dpstrf's range)");
    if (!(args.pivot_rtol >= 0.0) || !(args.pivot_tol_scale >= 0.0) || !(args.pivot_rtol <= 1.0e150) || !(args.pivot_tol_scale <= 1.0e150))
      throw std::invalid_argument("qr::cacqr::factor_pivoted: pivot_rtol and pivot_tol_scale must be finite and >= 0");
    capi_handle_t h = capital::handle();
    args.factored = false;
    args.pivoted = false;
    args.rank = 0;
    args.piv.clear();
    args.Q._register_(n, m_glob, CommInfo.c, CommInfo.d);
    args.G._register_(n, n, 1, 1);
    args.Ginv._register_(n, n, 1, 1);
    args.R1._register_(n, n, 1, 1);
    args.Rp._register_(n, n, 1, 1);
    args.Piv._register_(1, (n + 1) / 2, 1, 1);
    if (SP::packed_gram) args.Gpacked._register_(n, n, 1, 1);
    int* const piv = reinterpret_cast<int*>(args.Piv.data());
    CAPITAL_CHECK(capi_reset_info(h));
    args.potrf_info = 0;
    args.sweep_shift.clear(); args.sweep_trace.clear(); args.sweep_cond_bound.clear();
    gram_1d(A.data(), false, m_loc, n, args.G, args.Gpacked, CommInfo);
    CRITTER_START(CQR::formR);
    // the factor of a shifted sweep's shift, or the user's tolerance squared (G holds squared norms)
    const double floor_tol = 11.0 * ((double)m_glob * (double)n + (double)n * (double)(n + 1)) * 0x1p-53;
    const double tol = args.pivot_tol_scale * std::max(args.pivot_rtol * args.pivot_rtol, floor_tol);
    args.pivot_tol = tol;
    int rank = 0;
    CAPITAL_CHECK(capi_dpstrf(h, n, args.G.data(), n, tol, piv, &rank));                                              // identical bits on every rank
    args.rank = rank;
    args.piv.resize((size_t)n);
    CAPITAL_CHECK(capi_memcpy_d2h(h, args.piv.data(), piv, sizeof(int) * (size_t)n));
    if (rank < 1) {
      CRITTER_STOP(CQR::formR);
      throw std::domain_error("cacqr::factor_pivoted: numerical rank 0: no diagonal entry of the Gram matrix exceeds tol * trace (A is zero or not finite)");
    }
    const int64_t k = rank;
    // M = P(:, 0:k) R11^-1 (n x k) in R1; Q1 = A M
    CAPITAL_CHECK(capi_dlacpy(h, 1, k, k, args.G.data(), n, args.Ginv.data(), n));
    CAPITAL_CHECK(capi_dtrtri(h, CAPI_UPPER, CAPI_NONUNIT, k, args.Ginv.data(), n));
    CAPITAL_CHECK(capi_drow_scatter(h, 1, k, k, n, args.Ginv.data(), n, piv, args.R1.data(), n));
    CAPITAL_CHECK(capi_dgemm(h, CAPI_NOTRANS, CAPI_NOTRANS, m_loc, k, n, 1.0, A.data(), m_loc, args.R1.data(), n, 0.0, args.Q.data(), m_loc));
    CRITTER_STOP(CQR::formR);
    {
      // one plain sweep on the m_loc x k panel, on blocks of the panel's own order; [R11 R12] stays where capi_dpstrf left it
      matrix<double, Dim, rect> Gk(k, k, 1, 1), Gik(k, k, 1, 1);
      matrix<double, Dim, uppertri> Gpk;
      if (SP::packed_gram) Gpk._register_(k, k, 1, 1);
      sweep_1d(args.Q.data(), args.Q.scratch(), m_loc, k, Gk, Gik, Gpk, args, CommInfo);
      args.Q.swap();
      // Rp(0:k, :) = R2 [R11 R12]: the leading block's strictly lower part was never written
      CAPITAL_CHECK(capi_dtrizero(h, CAPI_UPPER, k, args.G.data(), n));
      CAPITAL_CHECK(capi_memset_async(h, args.Rp.data(), 0, sizeof(double) * (size_t)(n * n)));
      CAPITAL_CHECK(capi_dtrmm_oop(h, CAPI_LEFT, CAPI_UPPER, CAPI_NOTRANS, CAPI_NONUNIT, k, n, 1.0, Gk.data(), k, args.G.data(), n, args.Rp.data(), n));
      CAPITAL_CHECK(capi_get_info(h, &args.potrf_info));                                                              // drains the stream: the k x k blocks may go
    }
    if (!IP::keep_work) { args.G._destroy_(); args.Ginv._destroy_(); args.R1._destroy_(); args.Gpacked._destroy_(); }
    if (args.potrf_info != 0)
      throw std::domain_error("cacqr::factor_pivoted: the Gram matrix of the rank-" + std::to_string(k) + " panel is not positive definite (pivot " +
                              std::to_string(args.potrf_info) + "): Q and R are not valid; a larger pivot_tol_scale drops more columns");
    args.factored = true;
    args.pivoted = true;
  }

  // min ||A X - B||_F on the factors factor(A, args, CommInfo) left: args.X (n x r) and, with `residual`, args.ls_residual_norms.
  // B is distributed exactly as A: matrix<double, int64_t, rect>(r, m, c, d), the same row-cyclic owner map.  See the file comment.
  template <typename MatrixType, typename ArgType, typename CommType>
  static void least_squares(const MatrixType& A, const MatrixType& B, ArgType& args, CommType&& CommInfo, bool residual = true) {
    static_assert(std::is_same<typename MatrixType::StructureType, rect>::value, "qr::cacqr requires matrices of rect structure");
    if (CommInfo.c != 1) throw std::logic_error("qr::cacqr::least_squares is built for the 1-D variant (c == 1) only");
    if (!&capi_dgemtn_ts || !&capi_dresid_ts)
      throw std::logic_error("qr::cacqr: this C-ABI library has no capi_dgemtn_ts / capi_dresid_ts: no least-squares solve");
    // On factor_pivoted's factors the basic solution X = P [R11^-1 (Q^T B); 0]: Q has k = rank columns, R11 is Rp's leading block
    const bool piv = args.pivoted;
    if (piv && !&capi_drow_scatter) throw std::logic_error("qr::cacqr: this C-ABI library has no capi_drow_scatter: no solve on pivoted factors");
    if (!args.factored || args.potrf_info != 0 || !args.Q.filled() || (piv ? !args.Rp.filled() || !args.Piv.filled() || args.rank < 1 : !args.R.filled()))
      throw std::logic_error(piv ? "qr::cacqr::least_squares: factor_pivoted() did not succeed: there is no valid Q and R to solve with"
                                 : "qr::cacqr::least_squares: factor() has not run or did not succeed: there is no valid Q and R to solve with");
    capi_handle_t h = capital::handle();
    const int64_t n = A.num_columns_global(), m_loc = A.num_rows_local(), r = B.num_columns_global(), k = piv ? args.rank : n;
    if (r < 1 || B.num_rows_local() != m_loc || B.num_rows_global() != A.num_rows_global() || args.Q.num_rows_local() != m_loc ||
        args.Q.num_columns_global() != n || k > n)
      throw std::invalid_argument("qr::cacqr::least_squares: B must have r >= 1 columns and A's rows, distributed as A, and A must be the factored matrix");
    CRITTER_START(CQR::lstsq);
    util::resize_columns(args.X, r, n);
    const int64_t W = CAPI_TS_MAX_RHS;
    // C = Q^T B (k x r, leading dimension n; the last sweep leaves Q column-major), in X itself or, pivoted, in X's second buffer, whose rows >= k stay
    // zero.  capi_dgemtn_ts as it stands is UNMEASURED.  An earlier form of it lost to capi_dgemm(T, N) on the 128-tile kernel on both shapes that
    // were timed, 2^22 x 256 (3.7-3.9 against 2.5-2.8 ms) and 2^21 x 1024; on that evidence tall panels of width >= 256 take
    // that product.  Narrower or shorter panels take the streaming kernel; no form of it was timed there.
    double* const C = piv ? args.X.scratch() : args.X.data();
    const bool by_gemm = k >= 256 && m_loc >= 64 * k;
    for (int64_t j = 0; j < r; j += W) {
      const int64_t rb = std::min(W, r - j);
      if (by_gemm) CAPITAL_CHECK(capi_dgemm(h, CAPI_TRANS, CAPI_NOTRANS, k, rb, m_loc, 1.0, args.Q.data(), m_loc, B.data() + j * m_loc, m_loc, 0.0, C + j * n, n));
      else CAPITAL_CHECK(capi_dgemtn_ts(h, m_loc, k, rb, 1.0, args.Q.data(), m_loc, B.data() + j * m_loc, m_loc, 0.0, C + j * n, n));
    }
    if (CommInfo.size > 1) CAPITAL_CHECK(capi_allreduce_sum(CommInfo.world, C, n * r));
    if (piv) {
      CAPITAL_CHECK(capi_dtrsm(h, CAPI_LEFT, CAPI_UPPER, CAPI_NOTRANS, CAPI_NONUNIT, k, r, 1.0, args.Rp.data(), n, C, n));          // Y = R11^-1 C
      CAPITAL_CHECK(capi_drow_scatter(h, 0, k, r, n, C, n, reinterpret_cast<const int*>(args.Piv.data()), args.X.data(), n));
    } else {
      CAPITAL_CHECK(capi_dtrsm(h, CAPI_LEFT, CAPI_UPPER, CAPI_NOTRANS, CAPI_NONUNIT, n, r, 1.0, full_storage_R(args, n), n, C, n));  // X = R^-1 C
    }
    args.ls_residual_norms.clear();
    if (residual)
      args.ls_residual_norms = util::residual_norms(args.LsNorm2, r, CommInfo.size > 1 ? CommInfo.world : nullptr, [&](int64_t j, int64_t rb, double* norm2) {
        CAPITAL_CHECK(capi_dresid_ts(h, m_loc, n, rb, A.data(), m_loc, args.X.data() + j * n, n, B.data() + j * m_loc, m_loc, nullptr, 0, norm2));
      });
    if (!piv && !IP::keep_work) { capital::sync(); args.G._destroy_(); }
    CRITTER_STOP(CQR::lstsq);
  }

  // The singular value decomposition of the factored A on the pair factor() left: args.singular_values / args.Sigma, args.V and, with `left`,
  // args.U (m_loc x n).  Nothing of the factorization is overwritten.  See the file comment.
  template <typename ArgType, typename CommType>
  static void svd(ArgType& args, CommType&& CommInfo, bool left = true) {
    if (CommInfo.c != 1) throw std::logic_error("qr::cacqr::svd is built for the 1-D variant (c == 1) only");
    if (!&capi_dgesvj) throw std::logic_error("qr::cacqr: this C-ABI library has no capi_dgesvj: no singular value decomposition");
    if (args.pivoted) throw std::logic_error("qr::cacqr::svd: the resident factors are factor_pivoted's (a trapezoidal R): svd is built for factor()'s pair only");
    if (!args.factored || args.potrf_info != 0 || !args.Q.filled() || !args.R.filled())
      throw std::logic_error("qr::cacqr::svd: factor() has not run or did not succeed: there is no valid Q and R to decompose");
    capi_handle_t h = capital::handle();
    const int64_t n = args.Q.num_columns_global(), m_loc = args.Q.num_rows_local();
    CRITTER_START(CQR::svd);
    double* const Rfull = full_storage_R(args, n);
    args.Sigma._register_(1, n, 1, 1);
    args.V._register_(n, n, 1, 1);
    if (left) args.UR._register_(n, n, 1, 1);
    int sweeps = 0;
    CAPITAL_CHECK(capi_dgesvj(h, n, Rfull, n, left ? args.UR.data() : nullptr, n, args.Sigma.data(), args.V.data(), n, &sweeps));
    args.svd_sweeps = sweeps;
    if (left) {
      args.U._register_(n, args.Q.num_rows_global(), CommInfo.c, CommInfo.d);
      CAPITAL_CHECK(capi_dgemm(h, CAPI_NOTRANS, CAPI_NOTRANS, m_loc, n, n, 1.0, args.Q.data(), m_loc, args.UR.data(), n, 0.0, args.U.data(), m_loc));   // U = Q U_R
    }
    args.singular_values = args.Sigma.to_host();
    args.cond2 = args.singular_values.front() / args.singular_values.back();
    if (!IP::keep_work) { capital::sync(); args.G._destroy_(); args.UR._destroy_(); }
    CRITTER_STOP(CQR::svd);
    if (sweeps < 0)
      throw std::runtime_error("qr::cacqr::svd: the Jacobi sweeps on R did not converge within " + std::to_string(-sweeps) + " sweeps");
  }

  template <typename ArgType, typename CommType>
  static matrix<typename ArgType::ScalarType, typename ArgType::DimensionType, rect> construct_Q(ArgType& args, CommType&& CommInfo) {
    const auto lm = args.Q.num_rows_local(), ln = args.Q.num_columns_local();
    matrix<typename ArgType::ScalarType, typename ArgType::DimensionType, rect> ret(args.Q.num_columns_global(), args.Q.num_rows_global(), CommInfo.c, CommInfo.d);
    serialize<rect, rect>::invoke(args.Q, ret, 0, ln, 0, lm, 0, ln, 0, lm);
    return ret;
  }
  template <typename ArgType, typename CommType>
  static matrix<typename ArgType::ScalarType, typename ArgType::DimensionType, rect> construct_R(ArgType& args, CommType&& CommInfo) {
    const auto ln = args.R.num_columns_local();
    matrix<typename ArgType::ScalarType, typename ArgType::DimensionType, rect> ret(args.R.num_columns_global(), args.R.num_rows_global(), CommInfo.c, CommInfo.c);
    serialize<uppertri, uppertri>::invoke(args.R, ret, 0, ln, 0, ln, 0, ln, 0, ln);
    return ret;
  }

protected:
  // the full-storage image of R that capi_dtrsm and capi_dgesvj take, in the Gram work block (registered anew when the policy released it)
  template <typename ArgType>
  static double* full_storage_R(ArgType& args, int64_t n) {
    args.G._register_(n, n, 1, 1);
    serialize<uppertri, uppertri>::invoke(args.R, args.G, 0, n, 0, n, 0, n, 0, n);
    return args.G.data();
  }

  // K7 + C8: G <- src^T src (n x n, its upper triangle), summed over the ranks -- with Serialize as the n (n + 1) / 2 doubles of Gpacked.
  // src_tiled: the panel is a "panel32" image (include/capital_hip.h) instead of column-major
  template <typename GramType, typename PackedType, typename CommType>
  static void gram_1d(const double* src, bool src_tiled, int64_t m_loc, int64_t n, GramType& G, PackedType& Gpacked, CommType&& CommInfo) {
    capi_handle_t h = capital::handle();
    CRITTER_START(CQR::gram);
    if (src_tiled) CAPITAL_CHECK(capi_dsyrk_panel32(h, n, m_loc, 1.0, src, 0.0, G.data(), n));                       // K7 on the image
    else CAPITAL_CHECK(capi_dsyrk(h, CAPI_UPPER, CAPI_TRANS, n, m_loc, 1.0, src, m_loc, 0.0, G.data(), n));           // K7
    if (CommInfo.size > 1) {                                                                                       // C8
      if (SP::packed_gram) {
        serialize<uppertri, uppertri>::invoke(G, Gpacked, 0, n, 0, n, 0, n, 0, n);
        CAPITAL_CHECK(capi_allreduce_sum(CommInfo.world, Gpacked.data(), Gpacked.num_elems()));
        serialize<uppertri, uppertri>::invoke(Gpacked, G, 0, n, 0, n, 0, n, 0, n);
      } else {
        CAPITAL_CHECK(capi_allreduce_sum(CommInfo.world, G.data(), n * n));
      }
    }
    CRITTER_STOP(CQR::gram);
  }

  // one CholeskyQR sweep: dst <- src * chol(src^T src)^-1 on the blocks it is given, all of order n: leaves R in G and R^-1 in Ginv; Gpacked is the
  // all-reduce's transfer image (Serialize).  src_tiled / dst_tiled: the panel is a "panel32" image instead of column-major -- the intermediate
  // panels Q1, Q2, ..  rec != nullptr (runs with num_shifted > 0): the sweep's 4-double device record; shifted: equilibrate and shift the Gram
  // matrix (m_glob rows)
  template <typename GramType, typename PackedType, typename ArgType, typename CommType>
  static void sweep_1d(const double* src, double* dst, int64_t m_loc, int64_t n, GramType& G, GramType& Ginv, PackedType& Gpacked, ArgType& args,
                       CommType&& CommInfo, bool src_tiled = false, bool dst_tiled = false, bool shifted = false, double* rec = nullptr, int64_t m_glob = 0) {
    capi_handle_t h = capital::handle();
    gram_1d(src, src_tiled, m_loc, n, G, Gpacked, CommInfo);
    CRITTER_START(CQR::formR);
    if (shifted) CAPITAL_CHECK(capi_dgram_equilibrate_shift(h, n, G.data(), n, m_glob, args.shift_scale, args.Dscale.data(), rec));
    CAPITAL_CHECK(capi_dpotrf_trtri(h, n, G.data(), n, Ginv.data(), n));                                              // K8 + K9
    if (rec) CAPITAL_CHECK(capi_dtri_rescale(h, n, G.data(), n, Ginv.data(), n, shifted ? args.Dscale.data() : nullptr, rec));
    if (src_tiled || dst_tiled)
      CAPITAL_CHECK(capi_dtrmm_right_panel32(h, m_loc, n, 1.0, Ginv.data(), n, src, src_tiled ? 0 : m_loc, dst, dst_tiled ? 0 : m_loc));       // K5
    else
      CAPITAL_CHECK(capi_dtrmm_oop(h, CAPI_RIGHT, CAPI_UPPER, CAPI_NOTRANS, CAPI_NONUNIT, m_loc, n, 1.0, Ginv.data(), n, src, m_loc, dst, m_loc));  // K5
    CRITTER_STOP(CQR::formR);
  }

  template <typename MatrixType, typename ArgType, typename CommType>
  static void invoke_1d(const MatrixType& A, ArgType& args, CommType&& CommInfo) {
    capi_handle_t h = capital::handle();
    const int64_t n = A.num_columns_global(), m_loc = A.num_rows_local();
    args.G._register_(n, n, 1, 1);
    args.Ginv._register_(n, n, 1, 1);
    if (SP::packed_gram) args.Gpacked._register_(n, n, 1, 1);
    CAPITAL_CHECK(capi_reset_info(h));
    args.potrf_info = 0;
    args.pivoted = false;                // the factors about to be written are factor()'s
    const int64_t sweeps = std::max<int64_t>(1, (int64_t)args.num_iter), shifted = (int64_t)args.num_shifted;
    if (sweeps > 4 || shifted > sweeps) throw std::invalid_argument("qr::cacqr: num_iter is 1..4 sweeps, of which num_shifted <= num_iter are shifted");
    double* rec = nullptr;               // device records, 4 doubles per sweep (runs with shifted sweeps only)
    if (shifted > 0) {
      if (!&capi_dgram_equilibrate_shift || !&capi_dtri_rescale)
        throw std::logic_error("qr::cacqr: this C-ABI library has no capi_dgram_equilibrate_shift / capi_dtri_rescale: no shifted sweeps");
      args.Dscale._register_(1, n, 1, 1);
      args.SweepRec._register_(4, 4, 1, 1);
      rec = args.SweepRec.data();
    }
    // The full-width kernels' shape (n = 256, tall, whole 32-row tiles): the intermediate panels Q1 = A R1^-1, Q2, .. are never seen by the
    // caller; each is written by one sweep and read twice by the next as a panel32 image -- one contiguous stream per pass instead of 256
    // column streams (CAPITAL_NO_PANEL32: column-major throughout, A/B).  The arithmetic, and so Q and R, are the same bit for bit.
    const bool q1_tiled = sweeps > 1 && n == 256 && m_loc % 32 == 0 && m_loc >= 64 * n && !getenv("CAPITAL_NO_PANEL32");
    sweep_1d(A.data(), args.Q.data(), m_loc, n, args.G, args.Ginv, args.Gpacked, args, CommInfo, false, q1_tiled, shifted > 0, rec, (int64_t)A.num_rows_global());
    if (sweeps > 1) {
      args.R1._register_(n, n, 1, 1);
      capital::dev_copy(args.R1.data(), args.G.data(), n * n);                                                        // save_R_1d
      for (int64_t k = 1; k < sweeps; ++k) {
        sweep_1d(args.Q.data(), args.Q.scratch(), m_loc, n, args.G, args.Ginv, args.Gpacked, args, CommInfo, q1_tiled, q1_tiled && k + 1 < sweeps, k < shifted,
                 rec ? rec + 4 * k : nullptr, (int64_t)A.num_rows_global());
        args.Q.swap();
        // R = R_k * (R_k-1 .. R1) (cacqr.hpp:185-187): Ginv is free again and receives the product
        CAPITAL_CHECK(capi_dtrmm_oop(h, CAPI_RIGHT, CAPI_UPPER, CAPI_NOTRANS, CAPI_NONUNIT, n, n, 1.0, args.R1.data(), n, args.G.data(), n, args.Ginv.data(), n));
        if (k + 1 < sweeps) std::swap(args.R1.data(), args.Ginv.data());                                              // the product so far; the old one is overwritten next
      }
      finalize_R(args.Ginv, args, n);
    } else {
      finalize_R(args.G, args, n);   // the reference leaves the Gram matrix in R here with Serialize; R is what is documented
    }
    // one 4-byte read behind the launch chain (the reference drops LAPACK's info, lapack/interface.hpp:39,54)
    CAPITAL_CHECK(capi_get_info(h, &args.potrf_info));
    args.sweep_shift.clear(); args.sweep_trace.clear(); args.sweep_cond_bound.clear();
    if (rec) {                                                                                                      // the stream is drained: a plain copy
      double host[16];
      CAPITAL_CHECK(capi_memcpy_d2h(h, host, rec, sizeof(double) * 4 * (size_t)sweeps));
      for (int64_t k = 0; k < sweeps; ++k) {
        args.sweep_shift.push_back(k < shifted ? host[4 * k] : 0.0);
        args.sweep_trace.push_back(k < shifted ? host[4 * k + 1] : 0.0);
        args.sweep_cond_bound.push_back(host[4 * k + 2] * host[4 * k + 3]);
      }
    }
    if (args.potrf_info != 0)
      throw std::domain_error("cacqr::factor: the Gram matrix is not positive definite (pivot " + std::to_string(args.potrf_info) +
                              "): A is numerically rank deficient for CholeskyQR; Q and R are not valid");
  }

  // ---- 3-D variant, c == d (cacqr.hpp:75-116 sweep_3d, :195-215 invoke_3d) ---------------------------------------------
  // Gram matrix by SUMMA-style exchange: the A block of the row-root (x == z) is broadcast along `row`, multiplied with
  // the local block, the partial Grams are reduced over `column` onto (y == z) and broadcast over `depth` from y:
  // every rank ends with the element-cyclic (x,y) block of G = A^T A, replicated over z -- the input format of cholinv.
  template <typename Sq, typename ArgType>
  static void sweep_3d(const double* src, double* dst, int64_t m_loc, int64_t n_loc, ArgType& args, Sq& sq, matmult::arena& ws,
                       matrix<double, int64_t, rect>& G, capi_comm_t across_cubes = nullptr) {
    using CI = typename std::remove_reference<ArgType>::type::cholesky_inverse_type;
    capi_handle_t h = capital::handle();
    const int64_t mark = ws.top;
    matmult::view Aloc{const_cast<double*>(src), m_loc, m_loc, n_loc};
    CRITTER_START(CQR::gram);
    matmult::view Abc = matmult::summa::panel(sq.row, sq.x == sq.z, (int)sq.z, Aloc, ws);                           // C9 Bcast(row)
    double* part = ws.take(n_loc * n_loc);
    CAPITAL_CHECK(capi_dgemm(h, CAPI_TRANS, CAPI_NOTRANS, n_loc, n_loc, m_loc, 1.0, Abc.p, Abc.ld, src, m_loc, 0.0, part, n_loc));   // K3
    double* red = ws.take(n_loc * n_loc);
    CAPITAL_CHECK(capi_reduce_sum(sq.column, part, red, n_loc * n_loc, (int)sq.z));                                   // C9 Reduce(column)
    double* gsrc = (sq.y == sq.z) ? red : part;    // the depth root (z == y) holds the reduced block; others receive into `part`
    // tunable grid (cacqr.hpp:147): the cubes' blocks are summed over column_alt (every rank takes part; only the depth
    // roots' sums are used)
    if (across_cubes) CAPITAL_CHECK(capi_allreduce_sum(across_cubes, gsrc, n_loc * n_loc));
    CAPITAL_CHECK(capi_bcast(sq.depth, gsrc, n_loc * n_loc, (int)sq.y));                                              // C9 Bcast(depth)
    capital::dev_copy(G.data(), gsrc, n_loc * n_loc);
    CRITTER_STOP(CQR::gram);
    CRITTER_START(CQR::formR);
    CI::factor(G, args.cholesky_inverse_args, sq);                                                                   // cacqr.hpp:103
    auto Rinv = CI::construct_Rinv(args.cholesky_inverse_args, sq);
    if (args.cholesky_inverse_args.complete_inv) {
      matmult::view Tv{Rinv.data(), n_loc, n_loc, n_loc}, Cv{dst, m_loc, m_loc, n_loc};
      matmult::summa::trmm(sq, CAPI_RIGHT, CAPI_UPPER, CAPI_NOTRANS, CAPI_NONUNIT, 1.0, Tv, Aloc, Cv, ws);             // cacqr.hpp:108-112
      capital::sync();   // Rinv (a temporary) must outlive the multiply
    } else {
      // solve (cacqr.hpp:44-73): the top-level R^-1_12 was not formed, so Q = A R^-1 goes block by block over the same
      // local split cholinv used:  Q1 = A1 R11^-1,  Q2 = (A2 - Q1 R12) R22^-1.
      // (The reference passes alpha = 1, beta = -1 to the middle product, cacqr.hpp:58, which yields Q1 R12 - A2 and a
      //  sign-flipped Q2 with Q R != A; the path is outside its validated combinations, SURVEY 8c.  Built to the algebra.)
      auto Rfull = CI::construct_R(args.cholesky_inverse_args, sq);
      const int64_t s1 = n_loc >> args.cholesky_inverse_args.split, s2 = n_loc - s1;
      matmult::view X11{Rinv.data(), n_loc, s1, s1}, X22{Rinv.data() + s1 + s1 * n_loc, n_loc, s2, s2};
      matmult::view R12{Rfull.data() + s1 * n_loc, n_loc, s1, s2};
      matmult::view A1{const_cast<double*>(src), m_loc, m_loc, s1}, A2{const_cast<double*>(src) + s1 * m_loc, m_loc, m_loc, s2};
      matmult::view Q1{dst, m_loc, m_loc, s1}, Q2{dst + s1 * m_loc, m_loc, m_loc, s2};
      matmult::summa::trmm(sq, CAPI_RIGHT, CAPI_UPPER, CAPI_NOTRANS, CAPI_NONUNIT, 1.0, X11, A1, Q1, ws);
      matmult::view Tmp{ws.take(m_loc * s2), m_loc, m_loc, s2};
      capital::dev_copy(Tmp.p, A2.p, m_loc * s2);
      matmult::summa::gemm(sq, CAPI_NOTRANS, CAPI_NOTRANS, -1.0, Q1, R12, 1.0, Tmp, ws);
      matmult::summa::trmm(sq, CAPI_RIGHT, CAPI_UPPER, CAPI_NOTRANS, CAPI_NONUNIT, 1.0, X22, Tmp, Q2, ws);
      capital::sync();   // Rinv / Rfull (temporaries) must outlive the multiplies
    }
    CRITTER_STOP(CQR::formR);
    ws.top = mark;
  }

  template <typename MatrixType, typename ArgType, typename CommType>
  static void invoke_3d(const MatrixType& A, ArgType& args, CommType&& CommInfo) {
    using CI = typename std::remove_reference<ArgType>::type::cholesky_inverse_type;
    topo::square sq(CommInfo.cube, CommInfo.c, CommInfo.layout, CommInfo.num_chunks);
    const int64_t n = A.num_columns_global(), n_loc = A.num_columns_local(), m_loc = A.num_rows_local();
    matrix<double, int64_t, rect> G(n, n, CommInfo.c, CommInfo.c);
    matmult::arena& ws = matmult::summa::scratch_arena();
    ws.reserve(8 * m_loc * n_loc + 8 * n_loc * n_loc + 1024);
    capi_comm_t across = CommInfo.c < CommInfo.d ? CommInfo.column_alt : nullptr;
    sweep_3d(A.data(), args.Q.data(), m_loc, n_loc, args, sq, ws, G, across);
    matrix<double, int64_t, rect> Rfinal = CI::construct_R(args.cholesky_inverse_args, sq);
    if (args.num_iter > 1) {
      matrix<double, int64_t, rect> R1 = Rfinal;                                                                     // save_R_3d
      sweep_3d(args.Q.data(), args.Q.scratch(), m_loc, n_loc, args, sq, ws, G, across);
      args.Q.swap();
      matrix<double, int64_t, rect> R2 = CI::construct_R(args.cholesky_inverse_args, sq);
      // R = R2 * R1 on the grid (cacqr.hpp:208-211): right multiply by the triangular R1
      matmult::view Tv{R1.data(), n_loc, n_loc, n_loc}, Bv{R2.data(), n_loc, n_loc, n_loc}, Cv{Rfinal.data(), n_loc, n_loc, n_loc};
      matmult::summa::trmm(sq, CAPI_RIGHT, CAPI_UPPER, CAPI_NOTRANS, CAPI_NONUNIT, 1.0, Tv, Bv, Cv, ws);
      capital::sync();
    }
    serialize<uppertri, uppertri>::invoke(Rfinal, args.R, 0, n_loc, 0, n_loc, 0, n_loc, 0, n_loc);                    // cacqr.hpp:214
    capital::sync();
  }

  template <typename ArgType>
  static void finalize_R(matrix<double, typename ArgType::DimensionType, rect>& src, ArgType& args, int64_t n) {
    serialize<uppertri, uppertri>::invoke(src, args.R, 0, n, 0, n, 0, n, 0, n);
  }
};

}  // namespace qr

#endif  // CAPITAL_QR_CACQR_H_
