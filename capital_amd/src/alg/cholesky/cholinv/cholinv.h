// alg/cholesky/cholinv/cholinv.h -- recursive Cholesky with triangular inverse on MI355X
// (reference src/alg/cholesky/cholinv/cholinv.h:11-75, cholinv.hpp:6-183).
//
// Same call surface: cholinv<SerializePolicy,IntermediatesPolicy,BaseCasePolicy>::factor(A, args, topo),
// construct_R / construct_Rinv, and the info<T,U> pack (complete_inv, split, bc_mult_dim, dir; R, Rinv).
// Same schedule per recursion level (cholinv.hpp:107-155):
//   1. recurse on the leading block                         -> R11, R11^-1
//   2. CI::trsm   R12 = R11^-T * A12                        (trmm Left/Upper/Trans SUMMA)
//   3. CI::tmu    A22 <- A22 - R12^T R12                    (triangular-output SUMMA)
//   4. recurse on the trailing block                        -> R22, R22^-1
//   5. CI::tmu    R^-1_12 = -R11^-1 R12 R22^-1              (two trmm SUMMAs; skipped at the top level when !complete_inv)
// What is different underneath: blocks are views into the device-resident R / R^-1 (no serialize copies into per-level
// tables), every multiply runs on the fp64 MFMA tile kernel, step 3 computes only the upper triangle, and the base case
// is one fused potrf+trtri launch sequence on the aggregated block.
#ifndef CAPITAL_CHOLESKY_CHOLINV_H_
#define CAPITAL_CHOLESKY_CHOLINV_H_

#include <cfloat>

#include "./../../alg.h"
#include "./../../matmult/summa/summa.h"
#include "./policy.h"

// The thin triangular product of solve() is a weak reference, as cacqr.h has its four: a stand-in of the C-ABI without it (the CPU rehearsal
// shims of the test suite) still links and loads, factor() runs on it as before, and solve() refuses.  capi_dresid_sym is weak on its own: a
// library that has the other two but not it still solves, with capi_dresid_ts over all of A (which must then be stored symmetric).
#pragma weak capi_dtrmm_thin
#pragma weak capi_dresid_ts
#pragma weak capi_dresid_sym
// .. and so is the thin triangular solve of info::solve_by_substitution: without it solve() runs as before and refuses only that flag
#pragma weak capi_dtrsm_thin
// .. and the pieces of condition() / error_bounds(): without them factor() and solve() run as before and those two refuse
#pragma weak capi_dsym_abs
#pragma weak capi_dberr
#pragma weak capi_dcolamax
#pragma weak capi_dlacn_block
#pragma weak capi_dlacn_state_bytes
// .. and the rank-r update of the factors: without them update() refuses and everything else runs as before
#pragma weak capi_dchud
#pragma weak capi_dchud_inv
#pragma weak capi_dchud_log_bytes
// .. and the pivoted partial factorization: without them factor_pivoted() refuses and everything else runs as before
#pragma weak capi_dpchol
#pragma weak capi_dpchol_thresh
// .. and the reductions over the factors themselves: without them quadratic_forms(), log_determinant() and inverse_diagonal() refuse (apply() needs
// none of them) and everything else runs as before
#pragma weak capi_dtri_rownorm2
#pragma weak capi_dtri_logdiag
#pragma weak capi_dcolnorm2
// .. and the power-of-two equilibration: without them equilibrate() refuses and everything else runs as before
#pragma weak capi_dpoequ2
#pragma weak capi_dsym_scale2
#pragma weak capi_drow_scale2
// .. and the diagonal pieces of the low-rank operator L L^T + D: without them lowrank_prepare(), lowrank_solve() and lowrank_quadratic_forms() refuse and
// everything else runs as before
#pragma weak capi_dlr_diag
#pragma weak capi_drow_pow
#pragma weak capi_ddiag_add
#pragma weak capi_dgemtn_ts

namespace cholesky {

// which of the four triangular operators of the factorisation A = R^T R cholinv::apply applies to a block
enum class factor_op { R, Rt, Rinv, RinvT };

template <class SerializePolicy = policy::cholinv::Serialize, class IntermediatesPolicy = policy::cholinv::SaveIntermediates,
          class BaseCasePolicy = policy::cholinv::NoReplication>
class cholinv : public SerializePolicy, public IntermediatesPolicy, public BaseCasePolicy {
public:
  using SP = SerializePolicy;
  using IP = IntermediatesPolicy;
  using BP = BaseCasePolicy;

  template <typename ScalarT, typename DimensionT>
  class info {
  public:
    using ScalarType = ScalarT;
    using DimensionType = DimensionT;
    using alg_type = cholinv<SerializePolicy, IntermediatesPolicy, BaseCasePolicy>;
    using SP = SerializePolicy;
    using IP = IntermediatesPolicy;
    using BP = BaseCasePolicy;
    info(const info& p) : complete_inv(p.complete_inv), split(p.split), bc_mult_dim(p.bc_mult_dim), dir(p.dir) {}
    info(info&& p) : complete_inv(p.complete_inv), split(p.split), bc_mult_dim(p.bc_mult_dim), dir(p.dir) {}
    info(DimensionType complete_inv, DimensionType split, DimensionType bc_mult_dim, char dir)
        : complete_inv(complete_inv), split(split), bc_mult_dim(bc_mult_dim), dir(dir) {}
    // user input (cholinv.h:50-53)
    const DimensionType complete_inv, split, bc_mult_dim;
    const char dir;
    // factors (cholinv.h:55-56)
    matrix<ScalarType, DimensionType, typename SerializePolicy::structure> R, Rinv;
    // full-storage working images when the returned structure is packed
    matrix<ScalarType, DimensionType, rect> Rfull, Rinvfull;
    matmult::arena work;
    DimensionType localDimension = 0, globalDimension = 0, trueLocalDimension = 0, trueGlobalDimension = 0, bcDimension = 0;
    // bookkeeping exposed for tests / benches
    int64_t num_base_cases = 0, num_levels = 0;
    // TRSM mode (not in the reference, which has no TRSM anywhere; BASELINE north_star names the kernel): factor() runs the
    // textbook right-looking recursion -- potrf on the diagonal block, R12 = R11^-T A12 by a block TRSM, trailing SYRK -- and
    // forms NO inverse: n^3/3 executed flops instead of 5 n^3/12.  R is the same factor; Rinv is not formed (construct_Rinv
    // throws).  One GPU, or a d x d x c grid (potrf_rec_grid).  Default off: the reference-exact schedule.
    bool solve_with_trsm = false;
    // solve() by SUBSTITUTION on R (capi_dtrsm_thin, twice) instead of products with R^-1 (inverse mode) or the block TRSM (TRSM mode): row-wise
    // backward stable without refinement, reads the packed or the rect R as it lies (no full-storage image: Serialize + FlushIntermediates
    // solves in TRSM mode too), never touches Rinv.  May be switched between two solves on the same factors.  Default off.
    bool solve_by_substitution = false;
    // LAPACK info of the factorisation (the reference drops it, lapack/interface.hpp:39,54): 0, or the 1-based position,
    // inside the first diagonal block that failed, of the first non-positive pivot.  factor() throws std::domain_error then.
    int potrf_info = 0;
    // top-level overlap state: the input's right part is copied, and the finished left part packed, on the second stream
    const double* input = nullptr;
    DimensionType early_split = 0;
    DimensionType input_lead = 0;       // > 0: only this leading block of the input's left half was copied on the compute stream
    // solve(): `factored` -- the last factor() came back with valid factors; top_split -- the order h1 of the leading block when the top level
    // of the recursion split (0: it did not).  With complete_inv == 0 that is where R^-1 has its unformed block R^-1_12.
    bool factored = false, factored_trsm = false;     // factored_trsm: the mode (solve_with_trsm) that factor() ran in
    DimensionType top_split = 0;
    // the solution X (n x r) and, when asked for, ||b_j - A x_j||_2 per right-hand side
    matrix<ScalarType, DimensionType, rect> X, SolveNorm2;
    std::vector<double> solve_residual_norms;
    // condition(): ||A||_1, the reciprocal condition number 1 / (||A||_1 est ||A^-1||_1) as dpocon returns it, and the products with A^-1 that the
    // estimate took (at most 11).  error_bounds(): per column of X the componentwise backward error and the forward bound of dporfs, and the
    // products its slowest block of columns took
    double anorm1 = 0.0, rcond = 0.0;
    int lacn_applies = 0;
    std::vector<double> solve_ferr, solve_berr;
    // The work of solve(), condition(), error_bounds() and update(), apart from factor()'s `work`: each call reserves its whole need at once and takes
    // its blocks from it (ops_scope).  SaveIntermediates keeps it at its high-water mark, FlushIntermediates releases it at the end of every call.
    matmult::arena ops;
    // update(): the step of the last failed downdate (0: none)
    int update_info = 0;
    // The factors themselves.  apply(): Y (n x r) = op B for one of R, R^T, R^-1, R^-T; quadratic_forms(): quad[j] = b_j^T A^-1 b_j (Quad: its device
    // image); log_determinant(): logdet = log det A; inverse_diagonal(): inv_diag[i] = (A^-1)_ii, InvDiag its device image (n doubles).  None of
    // these is read by factor(), solve(), condition(), error_bounds() or update(), and X is not written by any of the four.
    matrix<ScalarType, DimensionType, rect> Y, Quad, InvDiag;
    std::vector<double> quad, inv_diag;
    double logdet = 0.0;
    // factor_pivoted().  Input: pivot_rtol -- the factorization stops where the largest remaining Schur diagonal entry is <= pivot_rtol trace(A); 0:
    // LAPACK dpstrf's default n u max_i a_ii; pivot_max_rank -- the most columns of L, 0: min(n, CAPI_PCHOL_MAX_RANK).  Results: Lp (n x max_rank, the
    // first pivot_rank columns valid, in A's own row ordering), pivl (host) / PivL (device: n ints in the first (n + 1) / 2 doubles): the chosen rows in
    // order, then the others ascending; Dres (n): the remaining Schur diagonal, 0 for a chosen row; resid_trace: its sum, for a PSD A the trace norm
    // of A - Lp Lp^T; pivot_thresh: the threshold the call stopped at.  None of these is read by factor(), solve(), condition() or update().
    double pivot_rtol = 0.0;
    int64_t pivot_max_rank = 0;
    matrix<ScalarType, DimensionType, rect> Lp, PivL, Dres;
    std::vector<int> pivl;
    int64_t pivot_rank = 0;
    double resid_trace = 0.0, pivot_thresh = 0.0;
    // equilibrate(): `equilibrated` -- A holds A_s = D^-1 A0 D^-1 and every operation on the factors answers for the original A0 = D A_s D; Dscale
    // (device, n doubles) / dscale (host): D's diagonal, powers of two 2^e_j; equil_exponents: the sum of the e_j (log_determinant()); scond = min d /
    // max d and amax = max a_jj as the last equilibrate() found them, whether or not it scaled
    bool equilibrated = false;
    matrix<ScalarType, DimensionType, rect> Dscale;
    std::vector<double> dscale;
    int64_t equil_exponents = 0;
    double scond = 1.0, amax = 0.0;
    // lowrank_prepare() / lowrank_solve() / lowrank_quadratic_forms(): the operator M = L L^T + D on factor_pivoted()'s L = Lp(:, 0:pivot_rank), with
    // d_i = (lowrank_shift + LrDiagIn_i) + Dres_i.  Input: lowrank_shift >= 0; LrDiagIn (device, n doubles), used when lowrank_use_diag is set;
    // lowrank_use_schur adds factor_pivoted()'s remaining Schur diagonal Dres.  Results of prepare: LrD (device, n doubles) -- d; Cap (k x k) -- R_c with
    // C = I + L^T D^-1 L = R_c^T R_c in its upper triangle; LrGram (k x k) -- G = L^T L in its upper triangle, formed by a prepare with a uniform d
    // (no LrDiagIn, no Schur diagonal) and kept for the next one on the same factor (lowrank_gram_valid); lowrank_logdet = log det M; lowrank_cnorm1 =
    // ||C||_1, the error scale of every result (times u); lowrank_dmin / lowrank_dmax; lowrank_rank -- the k that was prepared; lowrank_prepared.
    // Results of the other two: LrX (n x r) and lowrank_residual_norms; lowrank_quad and LrQuad (device: 2 r doubles, the two terms of each form).
    // factor_pivoted() discards the prepared state and G.  None of these is read by any other operation, and args.X is not written.
    double lowrank_shift = 0.0;
    bool lowrank_use_schur = false, lowrank_use_diag = false;
    matrix<ScalarType, DimensionType, rect> LrDiagIn, LrD, Cap, LrGram, LrX, LrNorm2, LrQuad;
    bool lowrank_prepared = false, lowrank_gram_valid = false;
    int64_t lowrank_rank = 0;
    double lowrank_logdet = 0.0, lowrank_cnorm1 = 0.0, lowrank_dmin = 0.0, lowrank_dmax = 0.0;
    std::vector<double> lowrank_residual_norms, lowrank_quad;
  };

  template <typename MatrixType, typename ArgType, typename CommType>
  static void factor(const MatrixType& A, ArgType& args, CommType&& CommInfo) {
    CRITTER_START(CI::factor);
    using U = typename ArgType::DimensionType;
    static_assert(std::is_same<typename MatrixType::StructureType, rect>::value, "cholinv::factor takes a rect-structured input block");
    if (!(args.split > 0) || args.dir != 'U') throw std::invalid_argument("cholinv: split > 0 and dir == 'U' required (cholinv.hpp:9)");
    if (CommInfo.d > 1 && CommInfo.d % CommInfo.c) throw std::invalid_argument("cholinv: c must divide d (or d == 1)");
    args.factored = false;
    args.factored_trsm = args.solve_with_trsm;
    args.top_split = 0;
    if (args.solve_with_trsm) { factor_trsm(A, args, CommInfo); args.factored = true; CRITTER_STOP(CI::factor); return; }
    const U localDimension = A.num_rows_local(), globalDimension = A.num_rows_global();
    CAPITAL_CHECK(capi_stream_select(capital::handle(), 0));    // (a call that threw mid-way may have left another stream selected)
    CAPITAL_CHECK(capi_reset_info(capital::handle()));
    args.potrf_info = 0;
    constexpr bool packed = !std::is_same<typename SP::structure, rect>::value;
    // cholinv.hpp:13: the upper triangle of the input becomes the working R; the rest of R and all of R^-1 are zero (working_images)
    const working w = working_images(A, args, CommInfo, true);
    double *const R = w.R, *const Ri = w.Rinv;
    const U ld = localDimension;
    set_dimensions(A, args, CommInfo);

    // Only the leading block is needed to start the left half's recursion (a chain of latency-bound kernels): the
    // rest of the input follows on the second stream and is awaited just before the top level's R12 product.
    const U h1 = localDimension >> args.split;
    args.input = A.data();
    args.early_split = 0;
    const bool will_split = splits(args, localDimension, (U)CommInfo.d);
    args.input_lead = 0;
    args.top_split = will_split ? h1 : 0;
    if (will_split && h1 > 0 && h1 < ld) {
      capi_handle_t hh = capital::handle();
      // the left spine starts on the leading blocks: when the recursion halves cleanly down to `lead`, only that block is
      // copied ahead of it; the rest of the left half follows on the second stream and is awaited by the node of order 2 lead
      U lead = h1;
      if (args.split == 1 && CommInfo.d == 1 && CommInfo.c == 1) while (lead >= 8192 && lead % 2 == 0 && (lead >> 1) * (U)CommInfo.d > args.bcDimension) lead >>= 1;
      CAPITAL_CHECK(capi_dlacpy(hh, 1, lead, lead, A.data(), ld, R, ld));
      CAPITAL_CHECK(capi_event_record(hh, EV_INPUT_HEAD));
      CAPITAL_CHECK(capi_stream_select(hh, 1));
      CAPITAL_CHECK(capi_event_wait(hh, EV_INPUT_HEAD));       // (also orders this call after the previous call's packing)
      if (lead < h1) {
        CAPITAL_CHECK(capi_dlacpy(hh, 0, lead, h1 - lead, A.data() + (int64_t)lead * ld, ld, R + (int64_t)lead * ld, ld));
        CAPITAL_CHECK(capi_dlacpy(hh, 1, h1 - lead, h1 - lead, A.data() + lead + (int64_t)lead * ld, ld, R + lead + (int64_t)lead * ld, ld));
        CAPITAL_CHECK(capi_event_record(hh, EV_INPUT_MID));
        args.input_lead = lead;
      }
      CAPITAL_CHECK(capi_dlacpy(hh, 0, h1, ld - h1, A.data() + (int64_t)h1 * ld, ld, R + (int64_t)h1 * ld, ld));
      CAPITAL_CHECK(capi_dlacpy(hh, 1, ld - h1, ld - h1, A.data() + h1 + (int64_t)h1 * ld, ld, R + h1 + (int64_t)h1 * ld, ld));
      CAPITAL_CHECK(capi_event_record(hh, EV_INPUT_REST));
      CAPITAL_CHECK(capi_stream_select(hh, 0));
      args.early_split = h1;
    } else {
      CAPITAL_CHECK(capi_dlacpy(capital::handle(), 1, ld, ld, A.data(), ld, R, ld));
    }


    // the reference's simulate() (cholinv.hpp:50-83) pre-allocates every level's tables; here ONE arena covers the
    // deepest concurrent need: panels + partial sums of the top level, or the aggregated base case
    const bool single = (CommInfo.d == 1 && CommInfo.c == 1);
    // the large launches go out one resident round at a time: same time, half the L2-to-fabric traffic (on grids: bandwidth the collectives'
    // copy kernels share).  The roofline figure is taken from the kernels' own interval stamps, which stay right when another stream (the packing,
    // a grid's collectives) runs beside a round, not from stream-ordered event brackets (capi_prof_collect_intervals).
    // CAPITAL_NO_LAUNCH_ROUNDS: one launch per product.
    capital::launch_rounds_scope rounds(true);
    const U h = localDimension - (localDimension >> args.split);
    const U agg = args.bcDimension;
    // (single GPU: one split1 x split2 block is live at a time -- W of step 2, released before step 4, then W2 of step 5 -- and
    //  split1 split2 <= h^2 at every level; the single-GPU trmm and syrk of summa.h take nothing from the arena)
    // (grids: the update's W, its exchanged copy + staging, two panels, the partial sums + their packed image, relay space and the landing
    //  half of the multi-path pair transfers, per-chunk copies of a pipelined multiply)
    //  (the K-sliced grids, d == 1, broadcast and relay nothing: 8 h^2 as in round 2 -- at n = 65536 on 1 x 1 x 2 h^2 is 8 GiB)
    int64_t need = single ? (int64_t)h * h + 1024 : (int64_t)(CommInfo.d == 1 ? 8 : 12) * h * h + 4 * (int64_t)agg * agg + 4096;
    args.work.reserve(need);

    invoke(args, CommInfo, R, Ri, ld, (U)0, localDimension, globalDimension);

    if (packed) {
      const U e = args.early_split;     // columns [0,e) of both factors and rows [0,e) of R were packed during the right half
      if (e > 0) {
        pack_block(args, CAPI_UPPERTRI, R, (double*)args.R.data(), ld, e, ld, e, ld);                                     // R22
        pack_block(args, CAPI_UPPERTRI, Ri, (double*)args.Rinv.data(), ld, e, ld, e, ld);                                 // Rinv22
        if (args.complete_inv) pack_block(args, CAPI_RECT, Ri, (double*)args.Rinv.data(), ld, e, ld, 0, e);              // Rinv12
        CAPITAL_CHECK(capi_event_wait(capital::handle(), EV_EARLY_PACK));
      } else {
        serialize<uppertri, uppertri>::invoke(args.Rfull, args.R, 0, ld, 0, ld, 0, ld, 0, ld);
        serialize<uppertri, uppertri>::invoke(args.Rinvfull, args.Rinv, 0, ld, 0, ld, 0, ld, 0, ld);
      }
    }
    if (!IP::keep_arena) {
      // FlushIntermediates (policy.h:85-156: every level's buffers are released after use instead of cached in the tables): here
      // the intermediates are the work arena and, with Serialize, the two full-storage working images of the factors -- after
      // the call only what the caller asked for stays resident (n = 65536 on one GPU: 96 GiB instead of 171 GiB beside A).
      capital::sync();
      args.work.release();
      if (packed) { args.Rfull._destroy_(); args.Rinvfull._destroy_(); }
    }
    CRITTER_STOP(CI::factor);
    // one 4-byte read behind the whole launch chain: a non-SPD input must not come back as NaN factors with status OK
    CAPITAL_CHECK(capi_get_info(capital::handle(), &args.potrf_info));
    // on a grid only the ranks that factored the failing aggregate hold its info word (layer 0 with ReplicateComp, the slice
    // root with NoReplication[Overlap]): the grid agrees before anyone unwinds, so every rank throws or none does
    const int failed = capital::ranks_with_nonzero(CommInfo.world, args.potrf_info);
    if (failed != 0)
      throw std::domain_error("cholinv::factor: the matrix is not positive definite (" +
                              (args.potrf_info != 0 ? "non-positive pivot " + std::to_string(args.potrf_info) + " of a diagonal block"
                                                    : std::string("reported by ") + std::to_string(failed) + " other rank(s) of the grid") +
                              "); R and Rinv are not valid");
    args.factored = true;
  }

  // ---- a badly scaled A (a covariance in mixed units, A0 = D0 C D0 with C well conditioned and D0 spanning many decades): LAPACK dposvx's
  // equilibration (dpoequb + dlaqsy), which the reference's cholinv lacks.  ONE rank.
  // equilibrate(): capi_dpoequ2 reads the diagonal and gives d_j = 2^e_j, e_j = floor(ex_j / 2) for a_jj = f 2^ex_j (the rule of
  // capi_dgram_equilibrate_shift, at any order), scond = min d / max d and amax = max a_jj (args.scond, args.amax).  A is scaled iff scond < thresh, or
  // amax < SMALL, or amax > LARGE with SMALL = DBL_MIN / DBL_EPSILON and LARGE = 1 / SMALL (dlaqsy's rule; thresh > 1 forces it): A's upper triangle
  // becomes that of A_s = D^-1 A D^-1 in place (capi_dsym_scale2: one pass at the rate of a copy), whose diagonal lies in [0.5, 2);
  // args.equilibrated = true, args.factored = false -- factor() then factors the A that lies there, A_s -- and true is returned.  Otherwise nothing
  // changes (valid factors stay valid) and false is returned.  A diagonal entry that is zero, negative, NaN or Inf: std::domain_error naming it, A
  // untouched.  Calling it while equilibrated: std::logic_error.
  // What it buys, and what not: the factors are homogeneous (R_s D is the Cholesky factor of A0, bit for bit where nothing over- or underflows), so no
  // bit of a solution changes; what changes is what rcond and ferr MEAN -- the condition and the error of the scaled problem, which is what governs
  // the accuracy -- and a matrix whose entries sit near the ends of the fp64 range is moved into its middle.
  // While args.equilibrated is set every operation answers for the ORIGINAL matrix A0 = D A_s D, whose factor is R0 = R_s D, through exact row scalings
  // (capi_drow_scale2): solve() runs on B_s = D^-1 B and returns X = D^-1 X_s, its residual norms are ||b - A0 x||_2 = ||D rho_s||_2; condition():
  // anorm1 and rcond of A_s, as dposvx defines them after equilibration; error_bounds() runs on (A_s, B_s, X_s = D X): berr is scale-invariant, ferr
  // bounds the error in the SCALED unknowns, ||D (x - x_true)||_inf / ||D x||_inf (it is not divided by scond as dposvx does: that turns a bound of 1e-10
  // into 1e5 on a matrix graded over 16 decades); update(V) uses D^-1 V; apply(): R: R_s (D b), Rt: D (R_s^T b), Rinv: D^-1 (R_s^-1 b), RinvT:
  // R_s^-T (D^-1 b); quadratic_forms() uses D^-1 B; log_determinant() adds 2 ln 2 sum e_j (the sum taken as an integer); inverse_diagonal() scales entry
  // i by 2^(-2 e_i); factor_pivoted() refuses (std::logic_error: its stopping rule on the scaled matrix is a design of its own).  construct_R,
  // construct_Rinv and the validators keep referring to the matrix that lies in A: R_s, R_s^-1 and A_s.
  // Memory, of args.ops: four doubles.
  template <typename MatrixType, typename ArgType, typename CommType>
  static bool equilibrate(MatrixType& A, ArgType& args, CommType&& CommInfo, double thresh = 0.1) {
    static_assert(std::is_same<typename MatrixType::StructureType, rect>::value, "cholinv::equilibrate takes a rect-structured A");
    if (CommInfo.size > 1) throw std::logic_error("cholinv::equilibrate is built for one rank: on a grid the matrix is element-cyclic");
    require_equil_abi();
    if (args.equilibrated) throw std::logic_error("cholinv::equilibrate: A is already equilibrated: unequilibrate() first");
    const int64_t n = A.num_rows_local();
    if (A.num_columns_local() != n || !(thresh == thresh)) throw std::invalid_argument("cholinv::equilibrate: A n x n, thresh not NaN");
    if (n == 0) return false;
    CRITTER_START(CI::equilibrate);
    capi_handle_t h = capital::handle();
    CAPITAL_CHECK(capi_stream_select(h, 0));
    args.Dscale._register_(1, n, 1, 1);
    double rec[4];
    {
      ops_scope ops(args.ops, 0, n, 4);
      double* const drec = ops.piece(4);
      CAPITAL_CHECK(capi_dpoequ2(h, n, A.data(), n, args.Dscale.data(), drec));
      CAPITAL_CHECK(capi_memcpy_d2h(h, rec, drec, sizeof(rec)));
    }
    bool scale = false;
    if (rec[3] == 0.0) {
      args.scond = rec[0]; args.amax = rec[1];
      const double SMALL = DBL_MIN / DBL_EPSILON, LARGE = 1.0 / SMALL;
      scale = args.scond < thresh || args.amax < SMALL || args.amax > LARGE || thresh > 1.0;
      if (scale) {
        CAPITAL_CHECK(capi_dsym_scale2(h, n, A.data(), n, args.Dscale.data(), 1));
        args.dscale = args.Dscale.to_host();
        args.equil_exponents = 0;
        for (double d : args.dscale) { int e; (void)std::frexp(d, &e); args.equil_exponents += e - 1; }
        args.equilibrated = true;
        args.factored = false;
      }
    }
    CRITTER_STOP(CI::equilibrate);
    if (rec[3] != 0.0)
      throw std::domain_error("cholinv::equilibrate: diagonal entry " + std::to_string((int64_t)rec[3]) + " (1-based) is zero, negative, NaN or Inf: "
                              "the matrix is not positive definite; A is unchanged");
    return scale;
  }

  // A's upper triangle <- that of D A_s D = A0, every bit as before equilibrate() (the scale factors are powers of two); args.equilibrated = false,
  // args.factored = false: the resident factors are those of A_s.  std::logic_error when A is not equilibrated.
  template <typename MatrixType, typename ArgType, typename CommType>
  static void unequilibrate(MatrixType& A, ArgType& args, CommType&& CommInfo) {
    static_assert(std::is_same<typename MatrixType::StructureType, rect>::value, "cholinv::unequilibrate takes a rect-structured A");
    if (CommInfo.size > 1) throw std::logic_error("cholinv::unequilibrate is built for one rank: on a grid the matrix is element-cyclic");
    require_equil_abi();
    if (!args.equilibrated) throw std::logic_error("cholinv::unequilibrate: A is not equilibrated");
    const int64_t n = A.num_rows_local();
    if (A.num_columns_local() != n || (int64_t)args.dscale.size() != n) throw std::invalid_argument("cholinv::unequilibrate: A must be the equilibrated matrix");
    capi_handle_t h = capital::handle();
    CAPITAL_CHECK(capi_stream_select(h, 0));
    CAPITAL_CHECK(capi_dsym_scale2(h, n, A.data(), n, args.Dscale.data(), -1));
    args.equilibrated = false;
    args.factored = false;
  }

  // A X = B on the factors factor(A, args, CommInfo) left, ONE rank: args.X (n x r) and, with `residual`, args.solve_residual_norms[j] =
  // ||b_j - A x_j||_2.  B: matrix<double, int64_t, rect>(r, n, 1, 1).  The inverse is applied by products, CAPI_TS_MAX_RHS columns at a time
  // (capi_dtrmm_thin: the factor is read once per product, packed or not, no copy of it is made):
  //   complete inverse (complete_inv != 0, or the top level did not split):  Y = R^-T B, X = R^-1 Y
  //   complete_inv == 0 and the top level split at h1 (R^-1_12 was never formed):
  //       y1 = R11^-T b1,  y2 = R22^-T (b2 - R12^T y1),  x2 = R22^-1 y2,  x1 = R11^-1 (y1 - R12 x2)      -- the same bytes as the complete form
  //   TRSM mode (no inverse exists): X = R^-1 R^-T B by capi_dtrsm on a full-storage R (Rfull where resident, or the rect structure)
  //   info::solve_by_substitution, either mode: X = R^-1 (R^-T B) by two capi_dtrsm_thin calls on R as it lies, packed or rect; no inverse is used
  // `refine` steps of fixed-precision refinement follow (rho = B - A X by capi_dresid_sym, X += solve(rho)): multiplying by an explicit inverse
  // is not backward stable in general, one step restores a backward error at the level of u for kappa u < 1.  The refinement and the residual
  // norms read A's UPPER triangle alone, as factor() does (capi_dresid_sym: a tile of the triangle serves the lines of its rows and, transposed,
  // of its columns): what lies below the diagonal is never used, in any mode.  (With a C-ABI library that lacks capi_dresid_sym both passes fall back to
  // capi_dresid_ts over all of A, which reads both triangles.)  refine == 0 and residual == false do not touch A.
  // After equilibrate() (args.equilibrated; A holds A_s = D^-1 A0 D^-1): the loop runs on B_s = D^-1 B and X = D^-1 X_s is returned, the same bytes as
  // without equilibration where nothing over- or underflows; the norms are ||b - A0 x||_2 = ||D rho_s||_2.  One n x CAPI_TS_MAX_RHS block of args.ops
  // more, three with `residual`.
  template <typename MatrixType, typename ArgType, typename CommType>
  static void solve(const MatrixType& A, const MatrixType& B, ArgType& args, CommType&& CommInfo, int refine = 1, bool residual = true) {
    static_assert(std::is_same<typename MatrixType::StructureType, rect>::value, "cholinv::solve takes rect-structured A and B");
    require_factors(args, CommInfo, "cholinv::solve");
    const int64_t n = args.localDimension, r = B.num_columns_global();
    if (r < 1 || B.num_rows_global() != n || B.num_rows_local() != n || A.num_rows_local() != n || A.num_columns_local() != n || refine < 0)
      throw std::invalid_argument("cholinv::solve: B must be n x r with r >= 1 (matrix(r, n, 1, 1)), A the factored matrix, refine >= 0");
    applier ap = make_applier(args, "cholinv::solve");
    CRITTER_START(CI::solve);
    capi_handle_t h = capital::handle();
    CAPITAL_CHECK(capi_stream_select(h, 0));
    const int64_t W = CAPI_TS_MAX_RHS;
    util::resize_columns(args.X, r, n);
    // equilibrated: the loop below runs on B_s = D^-1 B (bs) and leaves X_s, which becomes X = D^-1 X_s in place; the residual pass forms X_s = D X
    // again (xs) and rho_s (rs) and takes the norms of D rho_s
    const bool eq = args.equilibrated;
    const double* const D = eq ? args.Dscale.data() : nullptr;
    ops_scope ops(args.ops, ap.work_blocks + (refine > 0 ? 2 : 0) + (eq ? (residual ? 3 : 1) : 0), n, 0);
    take_applier_work(ap, ops);
    double* const rho = refine > 0 ? ops.block() : nullptr;
    double* const corr = refine > 0 ? ops.block() : nullptr;
    double* const bs = eq ? ops.block() : nullptr;
    double* const xs = eq && residual ? ops.block() : nullptr;
    double* const rs = eq && residual ? ops.block() : nullptr;
    auto apply = [&](const double* Bi, double* Xo, int64_t rb) { apply_inverse(ap, Bi, Xo, rb); };
    // Ro (or nothing) <- Bi - A Xi, norm2 (or nothing) <- its squared column norms, from A's upper triangle
    auto resid = [&](int64_t rb, const double* Xi, const double* Bi, double* Ro, double* norm2) {
      if (&capi_dresid_sym) { CAPITAL_CHECK(capi_dresid_sym(h, n, rb, A.data(), n, Xi, n, Bi, n, Ro, Ro ? n : 0, norm2)); }
      else { CAPITAL_CHECK(capi_dresid_ts(h, n, n, rb, A.data(), n, Xi, n, Bi, n, Ro, Ro ? n : 0, norm2)); }
    };
    for (int64_t j = 0; j < r; j += W) {
      const int64_t rb = std::min(W, r - j);
      double* Xj = args.X.data() + j * n;
      const double* Bj = B.data() + j * n;
      if (eq && n > 0) { CAPITAL_CHECK(capi_drow_scale2(h, n, rb, D, -1, Bj, n, bs, n, nullptr)); Bj = bs; }
      apply(Bj, Xj, rb);
      for (int it = 0; it < refine; ++it) {
        resid(rb, Xj, Bj, rho, nullptr);
        apply(rho, corr, rb);
        CAPITAL_CHECK(capi_dgeadd(h, 0, n, rb, 1.0, corr, n, 1.0, Xj, n));
      }
      if (eq && n > 0) CAPITAL_CHECK(capi_drow_scale2(h, n, rb, D, -1, Xj, n, Xj, n, nullptr));
    }
    args.solve_residual_norms.clear();
    if (residual)
      args.solve_residual_norms = util::residual_norms(args.SolveNorm2, r, nullptr, [&](int64_t j, int64_t rb, double* norm2) {
        if (!eq || n == 0) { resid(rb, args.X.data() + j * n, B.data() + j * n, nullptr, norm2); return; }
        CAPITAL_CHECK(capi_drow_scale2(h, n, rb, D, -1, B.data() + j * n, n, bs, n, nullptr));
        CAPITAL_CHECK(capi_drow_scale2(h, n, rb, D, 1, args.X.data() + j * n, n, xs, n, nullptr));
        resid(rb, xs, bs, rs, nullptr);
        CAPITAL_CHECK(capi_drow_scale2(h, n, rb, D, 1, rs, n, rs, n, norm2));
      });
    CRITTER_STOP(CI::solve);
  }

  // How well A is conditioned, from the factors factor(A, args, CommInfo) left (LAPACK dpocon; ONE rank, solve()'s preconditions):
  //   args.anorm1 = ||A||_1         one pass over A's upper triangle (capi_dsym_abs on a vector of ones)
  //   args.rcond  = 1 / (anorm1 est), est <= ||A^-1||_1 by the Hager-Higham estimator (capi_dlacn_block) over the operator of solve(), whichever of
  //                 its four forms the flags select: args.lacn_applies products with A^-1 on one column, at most 11; each costs what solve() pays for
  //                 one unrefined right-hand side.  0 when the estimate is Inf or NaN (or anorm1 is 0); 1 for n == 0.
  // The estimate is a lower bound of ||A^-1||_1 that is almost always within a factor 3 of it, so rcond errs on the large side.  Nothing of
  // args.X is touched.  Memory, of args.ops: the estimator's two n x CAPI_TS_MAX_RHS blocks and its state, beside the blocks of solve()'s operator.
  template <typename MatrixType, typename ArgType, typename CommType>
  static void condition(const MatrixType& A, ArgType& args, CommType&& CommInfo) {
    static_assert(std::is_same<typename MatrixType::StructureType, rect>::value, "cholinv::condition takes a rect-structured A");
    require_factors(args, CommInfo, "cholinv::condition");
    require_bounds_abi();
    const int64_t n = args.localDimension;
    if (A.num_rows_local() != n || A.num_columns_local() != n) throw std::invalid_argument("cholinv::condition: A must be the factored matrix");
    applier ap = make_applier(args, "cholinv::condition");
    args.anorm1 = 0.0; args.rcond = 1.0; args.lacn_applies = 0;
    if (n == 0) return;
    CRITTER_START(CI::condition);
    capi_handle_t h = capital::handle();
    CAPITAL_CHECK(capi_stream_select(h, 0));
    ops_scope ops(args.ops, ap.work_blocks + 2, n, estimator::tail(n));
    take_applier_work(ap, ops);
    const estimator es(ops, n);
    double* const small = es.small;
    {
      const std::vector<double> ones((size_t)n, 1.0);
      CAPITAL_CHECK(capi_memcpy_h2d(h, es.v1, ones.data(), sizeof(double) * (size_t)n));
    }
    CAPITAL_CHECK(capi_dsym_abs(h, n, 1, A.data(), n, es.v1, n, nullptr, 0, nullptr, 0, small));
    args.lacn_applies = estimate(es, ap, 1, nullptr, small + 1);
    double out[2];
    CAPITAL_CHECK(capi_memcpy_d2h(h, out, small, sizeof(out)));
    args.anorm1 = out[0];
    const double prod = out[0] * out[1];
    args.rcond = (std::isfinite(out[1]) && std::isfinite(prod) && prod > 0.0) ? 1.0 / prod : 0.0;
    CRITTER_STOP(CI::condition);
  }

  // How far the X of the last solve(A, B, ..) can be trusted (LAPACK dporfs without its refinement loop; ONE rank, solve()'s preconditions; B is the
  // B of that solve, args.X is read and never written).  CAPI_TS_MAX_RHS columns at a time:
  //   rho = B - A X (capi_dresid_sym), W = |A| |X| + |B| (capi_dsym_abs): two passes over A's upper triangle, plus one for more than 16 columns
  //   args.solve_berr[j] = max_i |rho_ij| / W_ij: the componentwise backward error of x_j -- the smallest e with (A + dA) x_j = b_j + db_j,
  //                        |dA| <= e |A|, |db_j| <= e |b_j| (capi_dberr, with dporfs's guard for tiny W_ij)
  //   args.solve_ferr[j] >= (estimated) || |A^-1| (|rho_j| + (n + 1) u W_j) ||_inf / ||x_j||_inf, which bounds ||x_j - x_true,j||_inf / ||x_j||_inf:
  //                        capi_dlacn_block runs the block's columns in lockstep over the operator of solve(), so 32 bounds cost the products of
  //                        the slowest column (args.lacn_applies, at most 11; each costs what solve() pays for an unrefined block)
  template <typename MatrixType, typename ArgType, typename CommType>
  static void error_bounds(const MatrixType& A, const MatrixType& B, ArgType& args, CommType&& CommInfo) {
    static_assert(std::is_same<typename MatrixType::StructureType, rect>::value, "cholinv::error_bounds takes rect-structured A and B");
    require_factors(args, CommInfo, "cholinv::error_bounds");
    require_bounds_abi();
    const int64_t n = args.localDimension, r = B.num_columns_global();
    if (r < 1 || B.num_rows_global() != n || B.num_rows_local() != n || A.num_rows_local() != n || A.num_columns_local() != n)
      throw std::invalid_argument("cholinv::error_bounds: B must be n x r with r >= 1 (matrix(r, n, 1, 1)), A the factored matrix");
    if (!args.X.filled() || args.X.num_columns_local() != r || args.X.num_rows_local() != n)
      throw std::invalid_argument("cholinv::error_bounds: the resident X is not that of a solve with this B (no solve yet, or another number of columns)");
    applier ap = make_applier(args, "cholinv::error_bounds");
    args.solve_ferr.assign((size_t)r, 0.0);
    args.solve_berr.assign((size_t)r, 0.0);
    args.lacn_applies = 0;
    if (n == 0) return;
    CRITTER_START(CI::error_bounds);
    capi_handle_t h = capital::handle();
    CAPITAL_CHECK(capi_stream_select(h, 0));
    const int64_t W = CAPI_TS_MAX_RHS;
    // equilibrated: everything below runs on the scaled problem (A_s, B_s = D^-1 B, X_s = D X)
    const bool eq = args.equilibrated;
    ops_scope ops(args.ops, ap.work_blocks + 4 + (eq ? 2 : 0), n, estimator::tail(n));
    take_applier_work(ap, ops);
    double *const rho = ops.block(), *const wt = ops.block();
    double *const bs = eq ? ops.block() : nullptr, *const xs = eq ? ops.block() : nullptr;
    const estimator es(ops, n);
    double* const small = es.small;
    for (int64_t j = 0; j < r; j += W) {
      const int64_t rb = std::min(W, r - j);
      const double* Xj = args.X.data() + j * n;
      const double* Bj = B.data() + j * n;
      if (eq) {
        CAPITAL_CHECK(capi_drow_scale2(h, n, rb, args.Dscale.data(), -1, Bj, n, bs, n, nullptr));
        CAPITAL_CHECK(capi_drow_scale2(h, n, rb, args.Dscale.data(), 1, Xj, n, xs, n, nullptr));
        Bj = bs; Xj = xs;
      }
      CAPITAL_CHECK(capi_dresid_sym(h, n, rb, A.data(), n, Xj, n, Bj, n, rho, n, nullptr));
      CAPITAL_CHECK(capi_dsym_abs(h, n, rb, A.data(), n, Xj, n, Bj, n, wt, n, nullptr));
      CAPITAL_CHECK(capi_dberr(h, n, rb, rho, n, wt, n, small));                               // berr; wt becomes the forward bound's weights
      CAPITAL_CHECK(capi_dcolamax(h, n, rb, Xj, n, small + 2 * W));                            // ||x_j||_inf
      args.lacn_applies = std::max(args.lacn_applies, estimate(es, ap, rb, wt, small + W));
      double out[3 * CAPI_TS_MAX_RHS];
      CAPITAL_CHECK(capi_memcpy_d2h(h, out, small, sizeof(out)));
      for (int64_t k = 0; k < rb; ++k) {
        args.solve_berr[(size_t)(j + k)] = out[k];
        const double est = out[W + k], xmax = out[2 * W + k];
        args.solve_ferr[(size_t)(j + k)] = xmax > 0.0 ? est / xmax : est;                      // (dporfs: divided where the norm is positive)
      }
    }
    CRITTER_STOP(CI::error_bounds);
  }

  // A <- A + sign V V^T (sign = +1: update, -1: downdate) on the factors factor(A, args, CommInfo) left, WITHOUT a new factorisation: O(n^2 r) instead
  // of O(n^3) (LINPACK's dchud / dchdd; ONE rank, solve()'s preconditions).  V: matrix<double, int64_t, rect>(r, n, 1, 1), any r >= 1; it is processed
  // in blocks of CAPI_TS_MAX_RHS columns from a scratch copy and is not modified.  Per block:
  //   1. R <- R' with R'^T R' = R^T R + sign V_b V_b^T (capi_dchud: n dependent steps in panels of 32 rows, each step logged)
  //   2. the info word of the block is read (the call's only synchronisation)
  //   3. R^-1 <- R'^-1 from the log (capi_dchud_inv), where an inverse exists: not in TRSM mode; with complete_inv == 0 and a top split at h1 the two
  //      diagonal blocks take the step ranges [0, h1) and [h1, n) and the unformed R^-1_12 is not touched
  // and at the end A's upper triangle takes sign V V^T (capi_dsyrk), so that solve()'s refinement, condition() and error_bounds() see the updated matrix.
  // Every resident image of the factors ends up consistent: with Serialize and SaveIntermediates the full-storage working images are updated and packed
  // again (serialize); with FlushIntermediates, which keeps no full image, the packed triangles are updated in place; NoSerialize has one image.
  // A downdate that leaves the matrix not positive definite: A is exactly as it was, args.factored = false (solve() reports that there are no valid
  // factors until the next factor()), args.update_info is the failing step (1-based, within its block of columns) and std::domain_error is thrown.
  template <typename MatrixType, typename ArgType, typename CommType>
  static void update(MatrixType& A, const MatrixType& V, ArgType& args, CommType&& CommInfo, int sign = 1) {
    static_assert(std::is_same<typename MatrixType::StructureType, rect>::value, "cholinv::update takes rect-structured A and V");
    require_factors(args, CommInfo, "cholinv::update");
    if (!&capi_dchud || !&capi_dchud_inv || !&capi_dchud_log_bytes) throw std::logic_error("cholinv: this C-ABI library has no capi_dchud / capi_dchud_inv: no update of the factors");
    const int64_t n = args.localDimension, r = V.num_columns_global();
    if (r < 1 || V.num_rows_global() != n || V.num_rows_local() != n || A.num_rows_local() != n || A.num_columns_local() != n || (sign != 1 && sign != -1))
      throw std::invalid_argument("cholinv::update: V must be n x r with r >= 1 (matrix(r, n, 1, 1)), A the factored matrix, sign +1 or -1");
    args.update_info = 0;
    if (n == 0) return;
    CRITTER_START(CI::update);
    capi_handle_t h = capital::handle();
    CAPITAL_CHECK(capi_stream_select(h, 0));
    const int64_t W = CAPI_TS_MAX_RHS, h1 = args.top_split;
    const bool inverse = !args.solve_with_trsm;
    const bool blocks = inverse && !args.complete_inv && h1 > 0 && h1 < n;
    // the images that take the steps
    const image Rw = pick_image(args.R, args.Rfull, n, image_use::in_place, "cholinv::update");
    const image Iw = inverse ? pick_image(args.Rinv, args.Rinvfull, n, image_use::in_place, "cholinv::update") : image();
    const typename image::block Rb = Rw.at(0, 0), Ib = Iw.at(0, 0);
    const int64_t log_count = (int64_t)((capi_dchud_log_bytes(n, W) + 7) / 8);
    // equilibrated: A_s + sign (D^-1 V) (D^-1 V)^T = D^-1 (A0 + sign V V^T) D^-1: the whole call runs on Vs = D^-1 V
    const bool eq = args.equilibrated;
    ops_scope ops(args.ops, 1, n, even(log_count) + (eq ? even(n * r) : 0));
    double *const v = ops.block(), *const log = ops.piece(log_count);
    const double* Vp = V.data();
    if (eq) {
      double* const Vs = ops.piece(n * r);
      CAPITAL_CHECK(capi_drow_scale2(h, n, r, args.Dscale.data(), -1, V.data(), n, Vs, n, nullptr));
      Vp = Vs;
    }
    int info = 0;
    int64_t bad_block = 0;
    for (int64_t j = 0; j < r && info == 0; j += W) {
      const int64_t rb = std::min(W, r - j);
      CAPITAL_CHECK(capi_dlacpy(h, 0, n, rb, Vp + j * n, n, v, n));
      CAPITAL_CHECK(capi_dchud(h, sign, n, rb, Rb.p, Rb.ldt, Rb.col0, v, n, log, &info));
      if (info != 0) { bad_block = j; break; }
      if (!inverse) continue;
      if (blocks) {
        CAPITAL_CHECK(capi_dchud_inv(h, sign, n, rb, Ib.p, Ib.ldt, Ib.col0, log, 0, h1));
        CAPITAL_CHECK(capi_dchud_inv(h, sign, n, rb, Ib.p, Ib.ldt, Ib.col0, log, h1, n));
      } else {
        CAPITAL_CHECK(capi_dchud_inv(h, sign, n, rb, Ib.p, Ib.ldt, Ib.col0, log, 0, n));
      }
    }
    if (info == 0) {
      // a working image took the steps: the packed factor beside it follows
      if (Rw.working) serialize<uppertri, uppertri>::invoke(args.Rfull, args.R, 0, n, 0, n, 0, n, 0, n);
      if (Iw.working) serialize<uppertri, uppertri>::invoke(args.Rinvfull, args.Rinv, 0, n, 0, n, 0, n, 0, n);
      CAPITAL_CHECK(capi_dsyrk(h, CAPI_UPPER, CAPI_NOTRANS, n, r, (double)sign, Vp, n, 1.0, A.data(), n));
    } else {
      args.factored = false;
      args.update_info = info;
    }
    CRITTER_STOP(CI::update);
    if (info != 0)
      throw std::domain_error("cholinv::update: the " + std::string(sign > 0 ? "updated" : "downdated") + " matrix is not positive definite (step " +
                              std::to_string(info) + " of " + std::to_string(n) + (r > W ? ", columns from " + std::to_string(bad_block) + " of V" : std::string()) +
                              "); A is unchanged, R and Rinv are not valid: factor() again");
  }

  // ---- the factors themselves: A = R^T R for whitening (R^-T b), sampling (R^T z ~ N(0, A), R^-1 z ~ N(0, A^-1)), the Gaussian log-likelihood
  // (b^T A^-1 b, log det A) and leave-one-out quantities (diag A^-1).  ONE rank, solve()'s preconditions (require_factors); O(n^2 r) or less on what is
  // resident; no n x n inverse is formed or stored.  After update() they work on the updated factors; after a failed downdate they refuse. ----

  // args.Y (n x r) <- op B, op one of R, R^T, R^-1, R^-T.  B: matrix<double, int64_t, rect>(r, n, 1, 1), any r >= 1, CAPI_TS_MAX_RHS columns at a time; B
  // and args.X are not written (error_bounds() after an apply() still sees the X of the last solve()).
  //   R, Rt        one capi_dtrmm_thin(CAPI_UPPERTRI) on R as it lies, packed or rect: in every mode, TRSM mode included
  //   Rinv, RinvT  one half of solve()'s operator (apply_half) in the form the flags select: substitution on R, capi_dtrsm on the full-storage R (TRSM
  //                mode), one product with the complete R^-1, or the block form; apply(Rinv, apply(RinvT, B)) is solve(B, refine = 0) bit for bit
  // Memory, of args.ops: one n x CAPI_TS_MAX_RHS block for the inverses in the block form, none otherwise.
  template <typename MatrixType, typename ArgType, typename CommType>
  static void apply(const MatrixType& B, ArgType& args, CommType&& CommInfo, factor_op op) {
    static_assert(std::is_same<typename MatrixType::StructureType, rect>::value, "cholinv::apply takes a rect-structured B");
    require_factors(args, CommInfo, "cholinv::apply");
    const int64_t n = args.localDimension, r = B.num_columns_global();
    if (r < 1 || B.num_rows_global() != n || B.num_rows_local() != n)
      throw std::invalid_argument("cholinv::apply: B must be n x r with r >= 1 (matrix(r, n, 1, 1))");
    const bool inverse = op == factor_op::Rinv || op == factor_op::RinvT;
    const int trans = (op == factor_op::Rt || op == factor_op::RinvT) ? CAPI_TRANS : CAPI_NOTRANS;
    // (R and R^T need the thin image of R alone: they run where a form of solve() has no image to run on)
    applier ap{};
    if (inverse) ap = make_applier(args, "cholinv::apply");
    const image Rw = pick_image(args.R, args.Rfull, n, image_use::thin_read, "cholinv::apply");
    CRITTER_START(CI::apply);
    capi_handle_t h = capital::handle();
    CAPITAL_CHECK(capi_stream_select(h, 0));
    const int64_t W = CAPI_TS_MAX_RHS;
    util::resize_columns(args.Y, r, n);
    // equilibrated (R0 = R_s D): R and R^-T scale the block that goes in (by D and D^-1, into a work block), R^T and R^-1 the one that comes out (by D
    // and D^-1, in place)
    const bool eq = args.equilibrated, scale_in = eq && (op == factor_op::R || op == factor_op::RinvT), scale_out = eq && !scale_in;
    const int dsign = (op == factor_op::R || op == factor_op::Rt) ? 1 : -1;
    ops_scope ops(args.ops, (inverse ? half_work_blocks(ap) : 0) + (scale_in ? 1 : 0), n, 0);
    if (inverse) take_half_work(ap, ops);
    double* const bs = scale_in ? ops.block() : nullptr;
    const typename image::block T = Rw.at(0, 0);
    for (int64_t j = 0; j < r && n > 0; j += W) {
      const int64_t rb = std::min(W, r - j);
      const double* Bj = B.data() + j * n;
      if (scale_in) { CAPITAL_CHECK(capi_drow_scale2(h, n, rb, args.Dscale.data(), dsign, Bj, n, bs, n, nullptr)); Bj = bs; }
      if (inverse) apply_half(ap, trans, Bj, args.Y.data() + j * n, rb);
      else CAPITAL_CHECK(capi_dtrmm_thin(h, CAPI_UPPERTRI, trans, n, n, rb, 1.0, T.p, T.ldt, T.col0, Bj, n, 0.0, args.Y.data() + j * n, n));
      if (scale_out) CAPITAL_CHECK(capi_drow_scale2(h, n, rb, args.Dscale.data(), dsign, args.Y.data() + j * n, n, args.Y.data() + j * n, n, nullptr));
    }
    CRITTER_STOP(CI::apply);
  }

  // args.quad[j] = b_j^T A^-1 b_j = ||R^-T b_j||^2 (the squared Mahalanobis length of b_j; args.Quad is its device image).  B as in apply().  Per block
  // of CAPI_TS_MAX_RHS columns: apply_half(R^-T) into a work block, then capi_dcolnorm2; the half-solve is not kept, B, args.X and args.Y are not written.
  // Memory, of args.ops: one n x CAPI_TS_MAX_RHS block, two in the block form.
  template <typename MatrixType, typename ArgType, typename CommType>
  static void quadratic_forms(const MatrixType& B, ArgType& args, CommType&& CommInfo) {
    static_assert(std::is_same<typename MatrixType::StructureType, rect>::value, "cholinv::quadratic_forms takes a rect-structured B");
    require_factors(args, CommInfo, "cholinv::quadratic_forms");
    if (!&capi_dcolnorm2) throw std::logic_error("cholinv: this C-ABI library has no capi_dcolnorm2: no quadratic forms");
    const int64_t n = args.localDimension, r = B.num_columns_global();
    if (r < 1 || B.num_rows_global() != n || B.num_rows_local() != n)
      throw std::invalid_argument("cholinv::quadratic_forms: B must be n x r with r >= 1 (matrix(r, n, 1, 1))");
    applier ap = make_applier(args, "cholinv::quadratic_forms");
    CRITTER_START(CI::quadratic_forms);
    capi_handle_t h = capital::handle();
    CAPITAL_CHECK(capi_stream_select(h, 0));
    const int64_t W = CAPI_TS_MAX_RHS;
    util::resize_columns(args.Quad, r, 1);
    {
      // equilibrated: b^T A0^-1 b = ||R_s^-T (D^-1 b)||^2
      const bool eq = args.equilibrated;
      ops_scope ops(args.ops, half_work_blocks(ap) + 1 + (eq ? 1 : 0), n, 0);
      take_half_work(ap, ops);
      double* const y = ops.block();
      double* const bs = eq ? ops.block() : nullptr;
      for (int64_t j = 0; j < r; j += W) {
        const int64_t rb = std::min(W, r - j);
        const double* Bj = B.data() + j * n;
        if (eq && n > 0) { CAPITAL_CHECK(capi_drow_scale2(h, n, rb, args.Dscale.data(), -1, Bj, n, bs, n, nullptr)); Bj = bs; }
        if (n > 0) apply_half(ap, CAPI_TRANS, Bj, y, rb);
        CAPITAL_CHECK(capi_dcolnorm2(h, n, rb, y, std::max<int64_t>(n, 1), args.Quad.data() + j));
      }
      args.quad = args.Quad.to_host();
    }
    CRITTER_STOP(CI::quadratic_forms);
  }

  // args.logdet = log det A = 2 sum_i log r_ii: capi_dtri_logdiag on R as it lies, packed or rect; in every mode.  Memory, of args.ops: two doubles.
  template <typename ArgType, typename CommType>
  static void log_determinant(ArgType& args, CommType&& CommInfo) {
    require_factors(args, CommInfo, "cholinv::log_determinant");
    if (!&capi_dtri_logdiag) throw std::logic_error("cholinv: this C-ABI library has no capi_dtri_logdiag: no log-determinant");
    const int64_t n = args.localDimension;
    const image Rw = pick_image(args.R, args.Rfull, n, image_use::thin_read, "cholinv::log_determinant");
    CRITTER_START(CI::log_determinant);
    capi_handle_t h = capital::handle();
    CAPITAL_CHECK(capi_stream_select(h, 0));
    double half = 0.0;
    {
      ops_scope ops(args.ops, 0, n, 2);
      double* const out = ops.piece(2);
      const typename image::block T = Rw.at(0, 0);
      CAPITAL_CHECK(capi_dtri_logdiag(h, n, T.p, T.ldt, T.col0, out));
      CAPITAL_CHECK(capi_memcpy_d2h(h, &half, out, sizeof(double)));
    }
    args.logdet = 2.0 * half;
    // equilibrated: det A0 = det(D)^2 det A_s, and det D = 2^(sum e_j), the sum an integer
    if (args.equilibrated) args.logdet += 2.0 * 0.6931471805599453094 * (double)args.equil_exponents;
    CRITTER_STOP(CI::log_determinant);
  }

  // args.inv_diag[i] (host; args.InvDiag: device, n doubles) = (A^-1)_ii = the sum of squares of row i of R^-1 (leave-one-out residuals, predictive
  // variances).  capi_dtri_rownorm2 reads R^-1 once, as it lies, packed or rect:
  //   complete inverse (complete_inv != 0, or the top level did not split): one pass over the triangle, no extra memory
  //   complete_inv == 0 and the top level split at h1: the two diagonal blocks are reduced as sub-triangles, and the block that factor() never formed,
  //       R^-1_12 = -R11^-1 R12 R22^-1 (h1 x h2; its step 5), is formed in args.ops by two triangular products on the tile kernels, added into the
  //       leading h1 entries (CAPI_RECT, beta = 1) and released.  This form costs the skipped products, h1 h2 n flops, each time it is called -- a
  //       caller who wants the diagonal more than once factors with complete_inv = 1 -- and h1 h2 doubles of args.ops, n^2 / 4 at an even split.
  //       With Serialize + FlushIntermediates only packed factors are resident: R11^-1, R12 and R22^-1 are first unpacked into args.ops
  //       (capi_serialize), h1^2 + h1 h2 + h2^2 doubles more.
  //   TRSM mode: there is no inverse; std::logic_error.
  // info::solve_by_substitution plays no part: the inverse is resident either way.
  template <typename ArgType, typename CommType>
  static void inverse_diagonal(ArgType& args, CommType&& CommInfo) {
    require_factors(args, CommInfo, "cholinv::inverse_diagonal");
    if (args.solve_with_trsm)
      throw std::logic_error("cholinv::inverse_diagonal: the TRSM mode forms no inverse (info::solve_with_trsm): factor in inverse mode for diag(A^-1)");
    if (!&capi_dtri_rownorm2) throw std::logic_error("cholinv: this C-ABI library has no capi_dtri_rownorm2: no diagonal of the inverse");
    const int64_t n = args.localDimension, h1 = args.top_split, h2 = n - h1;
    const bool blocks = !args.complete_inv && h1 > 0 && h1 < n;
    constexpr bool packed = !std::is_same<typename SP::structure, rect>::value;
    const char* const who = "cholinv::inverse_diagonal";
    const image Ip = pick_image(args.Rinv, args.Rinvfull, n, image_use::thin_read, who);
    args.inv_diag.clear();
    CRITTER_START(CI::inverse_diagonal);
    capi_handle_t h = capital::handle();
    CAPITAL_CHECK(capi_stream_select(h, 0));
    args.InvDiag._register_(1, std::max<int64_t>(n, 1), 1, 1);
    double* const out = args.InvDiag.data();
    auto rownorm2 = [&](int shape, int64_t m, int64_t k, const typename image::block& T, double beta, double* o) {
      CAPITAL_CHECK(capi_dtri_rownorm2(h, shape, m, k, T.p, T.ldt, T.col0, beta, o));
    };
    if (!blocks) {
      rownorm2(CAPI_UPPERTRI, n, n, Ip.at(0, 0), 0.0, out);
    } else {
      rownorm2(CAPI_UPPERTRI, h1, h1, Ip.at(0, 0), 0.0, out);
      rownorm2(CAPI_UPPERTRI, h2, h2, Ip.at(h1, h1), 0.0, out + h1);
      // the operands of the two products in column-major storage: the working images, the rect structure, or copies unpacked from the packed factors
      const bool have_full = !packed || (IP::keep_arena && args.Rfull.filled() && args.Rinvfull.filled());
      const int64_t c12 = even(h1 * h2), c11 = even(h1 * h1), c22 = even(h2 * h2);
      ops_scope ops(args.ops, 0, n, c12 + (have_full ? 0 : c11 + c12 + c22));
      double* const I12 = ops.piece(h1 * h2);
      const double *I11, *R12, *I22;
      int64_t ld11, ld12, ld22;
      if (have_full) {
        const double* const Rf = packed ? args.Rfull.data() : (const double*)args.R.data();
        const double* const If = packed ? args.Rinvfull.data() : (const double*)args.Rinv.data();
        I11 = If; R12 = Rf + h1 * n; I22 = If + h1 + h1 * n;
        ld11 = ld12 = ld22 = n;
      } else {
        double *const u11 = ops.piece(h1 * h1), *const u12 = ops.piece(h1 * h2), *const u22 = ops.piece(h2 * h2);
        auto unpack = [&](int shape, const double* src, double* dst, int64_t dx, int64_t dy, int64_t x0, int64_t x1, int64_t y0, int64_t y1) {
          CAPITAL_CHECK(capi_serialize_shape(h, shape, CAPI_UPPERTRI, CAPI_RECT, src, n, n, dst, dx, dy, x0, x1, y0, y1, 0, x1 - x0, 0, y1 - y0));
        };
        // (the products read the upper triangles of u11 and u22 alone: what the arena holds below their diagonals is never used)
        unpack(CAPI_UPPERTRI, (const double*)args.Rinv.data(), u11, h1, h1, 0, h1, 0, h1);
        unpack(CAPI_RECT, (const double*)args.R.data(), u12, h2, h1, h1, n, 0, h1);
        unpack(CAPI_UPPERTRI, (const double*)args.Rinv.data(), u22, h2, h2, h1, n, h1, n);
        I11 = u11; R12 = u12; I22 = u22;
        ld11 = h1; ld12 = h1; ld22 = h2;
      }
      CAPITAL_CHECK(capi_dtrmm_oop(h, CAPI_LEFT, CAPI_UPPER, CAPI_NOTRANS, CAPI_NONUNIT, h1, h2, 1.0, I11, ld11, R12, ld12, I12, h1));
      CAPITAL_CHECK(capi_dtrmm(h, CAPI_RIGHT, CAPI_UPPER, CAPI_NOTRANS, CAPI_NONUNIT, h1, h2, -1.0, I22, ld22, I12, h1));
      rownorm2(CAPI_RECT, h1, h2, typename image::block{I12, h1, 0}, 1.0, out);
    }
    // equilibrated: A0^-1 = D^-1 A_s^-1 D^-1: entry i takes 2^(-2 e_i), in two exact steps of 2^-e_i (the first result is a normal number)
    if (args.equilibrated && n > 0)
      for (int k = 0; k < 2; ++k) CAPITAL_CHECK(capi_drow_scale2(h, n, 1, args.Dscale.data(), -1, out, n, out, n, nullptr));
    args.inv_diag.resize((size_t)n);
    if (n > 0) CAPITAL_CHECK(capi_memcpy_d2h(h, args.inv_diag.data(), out, sizeof(double) * (size_t)n));
    CRITTER_STOP(CI::inverse_diagonal);
  }

  // A ~= Lp Lp^T by a diagonally pivoted, PARTIAL Cholesky (capi_dpchol), for a symmetric A that is only positive SEMIdefinite or numerically low-rank --
  // where factor() throws on the first non-positive pivot -- or of which k << n columns are wanted: O(n k^2), not O(n^3).  ONE rank.  Swap-free: Lp
  // (n x max_rank) is in A's own row ordering, column j belongs to the row args.pivl[j]; rows chosen before step j are exactly zero in column j.  It stops
  // at rank k where the largest remaining Schur diagonal entry is <= args.pivot_thresh = pivot_rtol trace(A) (pivot_rtol == 0: LAPACK dpstrf's default
  // n u max_i a_ii), or at max_rank = args.pivot_max_rank (0: min(n, CAPI_PCHOL_MAX_RANK)).  args.Dres is the Schur diagonal that remains and
  // args.resid_trace its sum: for a PSD A the trace norm of A - Lp Lp^T.  Like factor(), only A's upper triangle is read.
  // Independent of factor(): R, R^-1, `factored` and A are neither read nor changed; solve(), condition() and update() behave afterwards as before.
  // std::domain_error at rank 0 (A is zero or not finite), as qr::cacqr::factor_pivoted.
  template <typename MatrixType, typename ArgType, typename CommType>
  static void factor_pivoted(const MatrixType& A, ArgType& args, CommType&& CommInfo) {
    static_assert(std::is_same<typename MatrixType::StructureType, rect>::value, "cholinv::factor_pivoted takes a rect-structured input block");
    if (CommInfo.size > 1) throw std::logic_error("cholinv::factor_pivoted is built for one rank: on a grid the matrix is element-cyclic");
    if (!&capi_dpchol || !&capi_dpchol_thresh) throw std::logic_error("cholinv: this C-ABI library has no capi_dpchol: no pivoted factorization");
    if (args.equilibrated)
      throw std::logic_error("cholinv::factor_pivoted: A is equilibrated (its stopping rule on the scaled matrix is a design of its own): unequilibrate() first");
    const int64_t n = A.num_rows_local();
    const int64_t cap = std::min<int64_t>(n, CAPI_PCHOL_MAX_RANK), kmax = args.pivot_max_rank == 0 ? cap : args.pivot_max_rank;
    if (n < 1 || A.num_columns_local() != n || kmax < 1 || kmax > cap || !(args.pivot_rtol >= 0.0))
      throw std::invalid_argument("cholinv::factor_pivoted: A n x n with n >= 1, 0 <= pivot_max_rank <= min(n, CAPI_PCHOL_MAX_RANK), pivot_rtol >= 0");
    args.pivot_rank = 0;
    args.resid_trace = args.pivot_thresh = 0.0;
    args.pivl.clear();
    args.lowrank_prepared = args.lowrank_gram_valid = false;       // (what lowrank_prepare() left belongs to the factor that is about to go)
    CRITTER_START(CI::factor_pivoted);
    capi_handle_t h = capital::handle();
    CAPITAL_CHECK(capi_stream_select(h, 0));
    util::resize_columns(args.Lp, kmax, n);
    args.PivL._register_(1, (n + 1) / 2, 1, 1);
    args.Dres._register_(1, n, 1, 1);
    int* const piv = reinterpret_cast<int*>(args.PivL.data());
    const double tol = args.pivot_rtol == 0.0 ? -1.0 : args.pivot_rtol;
    int rank = 0;
    CAPITAL_CHECK(capi_dpchol_thresh(h, n, A.data(), n, tol, &args.pivot_thresh));
    CAPITAL_CHECK(capi_dpchol(h, n, A.data(), n, tol, kmax, args.Lp.data(), n, piv, args.Dres.data(), &rank, &args.resid_trace));
    args.pivl.resize((size_t)n);
    CAPITAL_CHECK(capi_memcpy_d2h(h, args.pivl.data(), piv, sizeof(int) * (size_t)n));
    args.pivot_rank = rank;
    CRITTER_STOP(CI::factor_pivoted);
    if (rank == 0)
      throw std::domain_error("cholinv::factor_pivoted: numerical rank 0: no diagonal entry exceeds the threshold (A is zero or not finite)");
  }

  // ---- M = L L^T + D on the pivoted partial factor: what a user of factor_pivoted() solves with.  L = args.Lp(:, 0:k), k = args.pivot_rank, is the
  // factor of a kernel or covariance matrix that is semidefinite or numerically low-rank -- where factor() refuses, so that solve(), log_determinant() and
  // quadratic_forms() are closed -- and D a positive diagonal: D = sigma^2 I is Nystroem / subset-of-regressors regression, D = sigma^2 I + diag(A - L L^T)
  // (lowrank_use_schur) is FITC.  Woodbury's identity on the k x k capacitance matrix C = I + L^T D^-1 L (SPD, lambda_min >= 1):
  //   M^-1 B = D^-1 (B - L T),  T = C^-1 (L^T (D^-1 B));    log det M = sum log d_i + log det C;    b^T M^-1 b = sum b_i^2 / d_i - ||R_c^-T L^T D^-1 b||^2
  // in O(n k^2) for prepare and O(n k r) per block of right-hand sides; no n x n matrix is formed and A is not read.  ONE rank.
  // The form is NOT backward stable: its error scale is ||C||_1 u, u = 2^-53 -- not kappa(C) u: at n = k = 1 kappa(C) = 1 and the error is ||C||_1 u all the
  // same (cancellation in B - L T) -- which is why args.lowrank_cnorm1 is handed out with every prepare.
  // Independent of factor(), as factor_pivoted() is: R, R^-1, `factored`, `equilibrated`, args.X and A are neither read nor written. ----

  // d_i = (args.lowrank_shift + LrDiagIn_i) + Dres_i (capi_dlr_diag; the vectors where args.lowrank_use_diag / lowrank_use_schur ask for them), then
  // C = R_c^T R_c (capi_dpotrf, k <= CAPI_PCHOL_MAX_RANK) into args.Cap, args.lowrank_logdet and args.lowrank_cnorm1 (capi_dsym_abs on a vector of ones,
  // from C's upper triangle, as condition() takes ||A||_1).  C is formed in one of two ways:
  //   a general d     C = I + L_s^T L_s, L_s = D^-1/2 L: an n x k piece of args.ops written once by capi_drow_pow and read by capi_dsyrk
  //   a uniform d     (no vector, no Schur diagonal): C = I + G / sigma^2 with G = L^T L by capi_dsyrk on L itself; no copy of L is made, and G stays in
  //                   args.LrGram: the next uniform prepare on the same factor costs a k^2 scaling and the k x k factorization, no pass over L
  // std::logic_error without a successful factor_pivoted(); std::invalid_argument for a shift that is not finite or < 0 or a vector of another length;
  // std::domain_error naming the first d_i that is not a finite number > 0, or when capi_dpotrf meets a pivot on C (overflow or NaN only: lambda_min(C) >= 1).
  // After any of them args.lowrank_prepared is false.  Memory, of args.ops: n k + k + 8 doubles for a general d, k + 8 for a uniform one.
  template <typename ArgType, typename CommType>
  static void lowrank_prepare(ArgType& args, CommType&& CommInfo) {
    require_lowrank(args, CommInfo, "cholinv::lowrank_prepare", false);
    args.lowrank_prepared = false;
    const int64_t n = args.Lp.num_rows_local(), k = args.pivot_rank;
    const double shift = args.lowrank_shift;
    if (!std::isfinite(shift) || shift < 0.0) throw std::invalid_argument("cholinv::lowrank_prepare: lowrank_shift must be finite and >= 0");
    if (args.lowrank_use_diag && (!args.LrDiagIn.filled() || (int64_t)args.LrDiagIn.num_elems() != n))
      throw std::invalid_argument("cholinv::lowrank_prepare: lowrank_use_diag needs LrDiagIn with n entries");
    const bool uniform = !args.lowrank_use_diag && !args.lowrank_use_schur;
    CRITTER_START(CI::lowrank_prepare);
    capi_handle_t h = capital::handle();
    CAPITAL_CHECK(capi_stream_select(h, 0));
    args.LrD._register_(1, n, 1, 1);
    util::resize_columns(args.Cap, k, k);
    double* const d = args.LrD.data();
    double* const C = args.Cap.data();
    const double* const L = args.Lp.data();
    double rec[4], cnorm = 0.0, half = 0.0;
    int info = 0;
    {
      ops_scope ops(args.ops, 0, n, (uniform ? 0 : even(n * k)) + even(k) + 8);
      double* const Ls = uniform ? nullptr : ops.piece(n * k);
      double* const ones = ops.piece(k);
      double* const drec = ops.piece(4);
      double* const small = ops.piece(4);                  // ||C||_1, sum log (R_c)_ii
      CAPITAL_CHECK(capi_dlr_diag(h, n, shift, args.lowrank_use_diag ? args.LrDiagIn.data() : nullptr, args.lowrank_use_schur ? args.Dres.data() : nullptr, d, drec));
      CAPITAL_CHECK(capi_memcpy_d2h(h, rec, drec, sizeof(rec)));
      if (rec[3] == 0.0) {
        if (uniform) {
          if (!args.lowrank_gram_valid || !args.LrGram.filled() || args.LrGram.num_rows_local() != k) {
            util::resize_columns(args.LrGram, k, k);
            CAPITAL_CHECK(capi_dsyrk(h, CAPI_UPPER, CAPI_TRANS, k, n, 1.0, L, n, 0.0, args.LrGram.data(), k));
            args.lowrank_gram_valid = true;
          }
          CAPITAL_CHECK(capi_dgeadd(h, 1, k, k, 1.0 / shift, args.LrGram.data(), k, 0.0, C, k));
        } else {
          CAPITAL_CHECK(capi_drow_pow(h, n, k, -0.5, d, 1.0, L, n, 0.0, Ls, n, nullptr));
          CAPITAL_CHECK(capi_dsyrk(h, CAPI_UPPER, CAPI_TRANS, k, n, 1.0, Ls, n, 0.0, C, k));
        }
        CAPITAL_CHECK(capi_ddiag_add(h, k, 1.0, C, k));
        {
          const std::vector<double> one((size_t)k, 1.0);
          CAPITAL_CHECK(capi_memcpy_h2d(h, ones, one.data(), sizeof(double) * (size_t)k));
        }
        CAPITAL_CHECK(capi_dsym_abs(h, k, 1, C, k, ones, k, nullptr, 0, nullptr, 0, small));
        // (the handle's info word is factor()'s too: factor() resets it before it starts and has read it when it returns, and args.potrf_info is not touched)
        CAPITAL_CHECK(capi_reset_info(h));
        CAPITAL_CHECK(capi_dpotrf(h, CAPI_UPPER, k, C, k));
        CAPITAL_CHECK(capi_get_info(h, &info));
        if (info != 0) CAPITAL_CHECK(capi_reset_info(h));
        CAPITAL_CHECK(capi_dtri_logdiag(h, k, C, k, 0, small + 1));
        double out[2];
        CAPITAL_CHECK(capi_memcpy_d2h(h, out, small, sizeof(out)));
        cnorm = out[0]; half = out[1];
      }
    }
    CRITTER_STOP(CI::lowrank_prepare);
    if (rec[3] != 0.0)
      throw std::domain_error("cholinv::lowrank_prepare: d_" + std::to_string((int64_t)rec[3]) + " (1-based) = shift + diag + schur is zero, negative, NaN or Inf: "
                              "D must be a positive diagonal (a row that factor_pivoted() chose has Schur diagonal 0: give a shift > 0)");
    if (info != 0)
      throw std::domain_error("cholinv::lowrank_prepare: the capacitance matrix I + L^T D^-1 L is not positive definite in fp64 (pivot " + std::to_string(info) +
                              "): it overflowed or holds a NaN");
    args.lowrank_logdet = rec[0] + 2.0 * half;
    args.lowrank_cnorm1 = cnorm;
    args.lowrank_dmin = rec[1]; args.lowrank_dmax = rec[2];
    args.lowrank_rank = k;
    args.lowrank_prepared = true;
  }

  // args.LrX (n x r) <- M^-1 B on what lowrank_prepare() left, and, with `residual`, args.lowrank_residual_norms[j] = ||b_j - M x_j||_2 with
  // M x = L (L^T x) + D x, from L and d alone.  B: matrix<double, int64_t, rect>(r, n, 1, 1), any r >= 1, CAPI_TS_MAX_RHS columns at a time, as solve():
  //   W = D^-1 B (capi_drow_pow, by division), T = L^T W (capi_dgemtn_ts on L as it lies), T <- R_c^-1 R_c^-T T (capi_dtrsm_thin twice, ldt = k),
  //   X = B - L T (capi_dresid_ts), X <- D^-1 X (in place)
  // L is read twice per block (twice more for the residual norms) and never copied or scaled; B and args.X are not written.
  // Memory, of args.ops: one n x CAPI_TS_MAX_RHS block and k x CAPI_TS_MAX_RHS doubles.
  template <typename MatrixType, typename ArgType, typename CommType>
  static void lowrank_solve(const MatrixType& B, ArgType& args, CommType&& CommInfo, bool residual = true) {
    static_assert(std::is_same<typename MatrixType::StructureType, rect>::value, "cholinv::lowrank_solve takes a rect-structured B");
    require_lowrank(args, CommInfo, "cholinv::lowrank_solve", true);
    const int64_t n = args.Lp.num_rows_local(), k = args.lowrank_rank, r = B.num_columns_global();
    if (r < 1 || B.num_rows_global() != n || B.num_rows_local() != n)
      throw std::invalid_argument("cholinv::lowrank_solve: B must be n x r with r >= 1 (matrix(r, n, 1, 1))");
    CRITTER_START(CI::lowrank_solve);
    capi_handle_t h = capital::handle();
    CAPITAL_CHECK(capi_stream_select(h, 0));
    const int64_t W = CAPI_TS_MAX_RHS;
    util::resize_columns(args.LrX, r, n);
    const double *const L = args.Lp.data(), *const d = args.LrD.data(), *const Rc = args.Cap.data();
    ops_scope ops(args.ops, 1, n, even(k * W));
    double* const w = ops.block();
    double* const T = ops.piece(k * W);
    // T (k x rb) <- C^-1 (L^T V) for an n x rb block V
    auto capacitance = [&](const double* V, int64_t rb) {
      CAPITAL_CHECK(capi_dgemtn_ts(h, n, k, rb, 1.0, L, n, V, n, 0.0, T, k));
      CAPITAL_CHECK(capi_dtrsm_thin(h, CAPI_TRANS, k, rb, Rc, k, 0, T, k));
      CAPITAL_CHECK(capi_dtrsm_thin(h, CAPI_NOTRANS, k, rb, Rc, k, 0, T, k));
    };
    for (int64_t j = 0; j < r; j += W) {
      const int64_t rb = std::min(W, r - j);
      const double* Bj = B.data() + j * n;
      double* Xj = args.LrX.data() + j * n;
      CAPITAL_CHECK(capi_drow_pow(h, n, rb, -1.0, d, 1.0, Bj, n, 0.0, w, n, nullptr));
      capacitance(w, rb);
      CAPITAL_CHECK(capi_dresid_ts(h, n, k, rb, L, n, T, k, Bj, n, Xj, n, nullptr));
      CAPITAL_CHECK(capi_drow_pow(h, n, rb, -1.0, d, 1.0, Xj, n, 0.0, Xj, n, nullptr));
    }
    args.lowrank_residual_norms.clear();
    if (residual)
      args.lowrank_residual_norms = util::residual_norms(args.LrNorm2, r, nullptr, [&](int64_t j, int64_t rb, double* norm2) {
        const double* Xj = args.LrX.data() + j * n;
        CAPITAL_CHECK(capi_dgemtn_ts(h, n, k, rb, 1.0, L, n, Xj, n, 0.0, T, k));                            // L^T x
        CAPITAL_CHECK(capi_dresid_ts(h, n, k, rb, L, n, T, k, B.data() + j * n, n, w, n, nullptr));         // b - L (L^T x)
        CAPITAL_CHECK(capi_drow_pow(h, n, rb, 1.0, d, -1.0, Xj, n, 1.0, w, n, norm2));                      // .. - D x, and its squared norms
      });
    CRITTER_STOP(CI::lowrank_solve);
  }

  // args.lowrank_quad[j] = b_j^T M^-1 b_j = sum_i b_ij^2 / d_i - ||R_c^-T L^T D^-1 b_j||^2: half of a lowrank_solve() -- one pass over L and one
  // substitution.  B as there.  The two terms lie in args.LrQuad (device, 2 r doubles: the first sums, then the norms) and are subtracted on the host.
  // sum b^2 / d is capi_drow_pow(power -1/2) with its column norms, into a work block that D^-1 B then overwrites.  B, args.X and args.LrX are not written.
  // Memory, of args.ops: lowrank_solve()'s.
  template <typename MatrixType, typename ArgType, typename CommType>
  static void lowrank_quadratic_forms(const MatrixType& B, ArgType& args, CommType&& CommInfo) {
    static_assert(std::is_same<typename MatrixType::StructureType, rect>::value, "cholinv::lowrank_quadratic_forms takes a rect-structured B");
    require_lowrank(args, CommInfo, "cholinv::lowrank_quadratic_forms", true);
    if (!&capi_dcolnorm2) throw std::logic_error("cholinv: this C-ABI library has no capi_dcolnorm2: no quadratic forms");
    const int64_t n = args.Lp.num_rows_local(), k = args.lowrank_rank, r = B.num_columns_global();
    if (r < 1 || B.num_rows_global() != n || B.num_rows_local() != n)
      throw std::invalid_argument("cholinv::lowrank_quadratic_forms: B must be n x r with r >= 1 (matrix(r, n, 1, 1))");
    CRITTER_START(CI::lowrank_quadratic_forms);
    capi_handle_t h = capital::handle();
    CAPITAL_CHECK(capi_stream_select(h, 0));
    const int64_t W = CAPI_TS_MAX_RHS;
    util::resize_columns(args.LrQuad, 2 * r, 1);
    const double *const L = args.Lp.data(), *const d = args.LrD.data(), *const Rc = args.Cap.data();
    {
      ops_scope ops(args.ops, 1, n, even(k * W));
      double* const w = ops.block();
      double* const T = ops.piece(k * W);
      for (int64_t j = 0; j < r; j += W) {
        const int64_t rb = std::min(W, r - j);
        const double* Bj = B.data() + j * n;
        CAPITAL_CHECK(capi_drow_pow(h, n, rb, -0.5, d, 1.0, Bj, n, 0.0, w, n, args.LrQuad.data() + j));
        CAPITAL_CHECK(capi_drow_pow(h, n, rb, -1.0, d, 1.0, Bj, n, 0.0, w, n, nullptr));
        CAPITAL_CHECK(capi_dgemtn_ts(h, n, k, rb, 1.0, L, n, w, n, 0.0, T, k));
        CAPITAL_CHECK(capi_dtrsm_thin(h, CAPI_TRANS, k, rb, Rc, k, 0, T, k));
        CAPITAL_CHECK(capi_dcolnorm2(h, k, rb, T, k, args.LrQuad.data() + r + j));
      }
      const std::vector<double> terms = args.LrQuad.to_host();
      args.lowrank_quad.resize((size_t)r);
      for (int64_t j = 0; j < r; ++j) args.lowrank_quad[(size_t)j] = terms[(size_t)j] - terms[(size_t)(r + j)];
    }
    CRITTER_STOP(CI::lowrank_quadratic_forms);
  }

  // ---- TRSM mode -----------------------------------------------------------------------------------------------------------
  // R = chol(A) with the same split rule and base-case size as the reference recursion (cholinv.hpp:15-18,93,107), but
  //   2'. R12 = R11^-T A12 by capi_dtrsm (block TRSM: products on the MFMA tile kernel, 256-blocks inverted on the fly)
  //   3.  A22 <- A22 - R12^T R12 by capi_dsyrk (upper triangle only)
  // and no step 5; the base case is capi_dpotrf alone.  Nothing of R^-1 is formed.
  template <typename MatrixType, typename ArgType, typename CommType>
  static void factor_trsm(const MatrixType& A, ArgType& args, CommType&& CommInfo) {
    using U = typename ArgType::DimensionType;
    capi_handle_t h = capital::handle();
    const U ld = A.num_rows_local();
    CAPITAL_CHECK(capi_stream_select(h, 0));
    CAPITAL_CHECK(capi_reset_info(h));
    args.potrf_info = 0;
    constexpr bool packed = !std::is_same<typename SP::structure, rect>::value;
    double* const R = working_images(A, args, CommInfo, false).R;
    CAPITAL_CHECK(capi_dlacpy(h, 1, ld, ld, A.data(), ld, R, ld));                                   // cholinv.hpp:13
    set_dimensions(A, args, CommInfo);
    if (CommInfo.d == 1) {
      potrf_rec(args, R, ld, (U)0, ld);                 // (d == 1, c > 1: every layer holds the whole matrix and factors it)
    } else {
      // d x d x c grid (round 3): the arena holds, at the top level, the assembled R11 and R12 (4 h^2 each), the gathered pieces behind
      // them (4 h^2 each) and what the trailing update's SUMMA needs
      const U hh = ld - (ld >> args.split);
      args.work.reserve((int64_t)32 * hh * hh + 4 * (int64_t)args.bcDimension * args.bcDimension + 4096);
      potrf_rec_grid(args, CommInfo, R, ld, (U)0, ld);
    }
    if (packed) serialize<uppertri, uppertri>::invoke(args.Rfull, args.R, 0, ld, 0, ld, 0, ld, 0, ld);
    CAPITAL_CHECK(capi_get_info(h, &args.potrf_info));
    const int failed = capital::ranks_with_nonzero(CommInfo.world, args.potrf_info);       // (replicated base cases: all ranks see it; agreed on anyway)
    if (failed != 0)
      throw std::domain_error("cholinv::factor (TRSM mode): the matrix is not positive definite (non-positive pivot " + std::to_string(args.potrf_info) + " of a diagonal block)");
  }

  // TRSM mode on a d x d x c grid (d > 1).  The element-cyclic layout has block size ONE, so a triangular solve cannot be pipelined over
  // block rows the way ScaLAPACK does it; instead the solve is made LOCAL:
  //   2'. every rank assembles R11 (all-gather of the d^2 pieces over `slice`, re-indexed cyclic -> global: the base case's machinery at
  //       the order of a recursion level) and the whole A12; the P = d^2 c ranks of the grid each solve S2 / P global COLUMNS of
  //       R11^T X = A12 with the block TRSM (capi_dtrsm: no flop is done twice), the solved column ranges are all-gathered IN PLACE over
  //       the world communicator (they are contiguous column blocks of the global image), and every rank keeps its own cyclic piece;
  //   3.  A22 -= R12^T R12 by the triangular-output SUMMA of the reference schedule (partner exchange, row / column broadcasts, depth sum).
  // Base case: the aggregate is gathered and factored on every rank (ReplicateCommComp's pattern, policy.h:160-224, without the inverse).
  // Bytes per rank and level: ~7 h^2 for step 2' against 3 h^2 for the reference's TRMM SUMMA -- this mode trades communication for
  // arithmetic (n^3/3 executed, no inverse); on one node's mesh with multi-path transfers for the update it is the cheaper of the two
  // only when the links are not the limit.  Parity: R is unique, so the assembled factor must equal the one-GPU factor (tests).
  template <typename ArgType, typename CommType, typename U>
  static void potrf_rec_grid(ArgType& args, CommType&& t, double* R, U ld, U start, U dim) {
    using matmult::view;
    capi_handle_t h = capital::handle();
    matmult::arena& ws = args.work;
    const int64_t d = (int64_t)t.d, P = (int64_t)t.size, me = (int64_t)t.x + d * (int64_t)t.y;
    const U split1 = dim >> args.split;
    double* R11 = R + start + start * ld;
    if (!splits(args, dim, (U)t.d)) {
      CRITTER_START(CI::factor_diag);
      const int64_t L = dim, agg = L * d;
      const int64_t span = ((start + dim) != args.trueLocalDimension) ? agg : agg - (args.trueLocalDimension * d - args.trueGlobalDimension);
      const int64_t mark = ws.top;
      double* mine = ws.take(L * L);
      double* blocked = ws.take(L * L * d * d);
      double* cyc = ws.take(agg * agg);
      CAPITAL_CHECK(capi_dlacpy(h, 0, L, L, R11, ld, mine, L));
      CAPITAL_CHECK(capi_allgather(t.slice, mine, blocked, L * L));
      util::block_to_cyclic_rect(blocked, cyc, L, L, d);
      CAPITAL_CHECK(capi_dpotrf(h, CAPI_UPPER, span, cyc, agg));
      CAPITAL_CHECK(capi_dtrizero(h, CAPI_UPPER, agg, cyc, agg));
      util::cyclic_to_block_rect(blocked, cyc, L, L, d);
      CAPITAL_CHECK(capi_dlacpy(h, 0, L, L, blocked + me * L * L, L, R11, ld));
      ws.top = mark;
      ++args.num_base_cases;
      CRITTER_STOP(CI::factor_diag);
      return;
    }
    ++args.num_levels;
    const U split2 = dim - split1;
    double* R12 = R + start + (start + split1) * ld;
    view A22{R + (start + split1) + (start + split1) * ld, ld, split2, split2};
    potrf_rec_grid(args, t, R, ld, start, split1);
    CRITTER_START(CI::trsm);
    const int64_t mark = ws.top;
    view W{ws.take((int64_t)split1 * split2), split1, split1, split2};                                 // this rank's piece of R12, contiguous
    {
      const int64_t L1 = split1, L2 = split2, S1 = L1 * d, S2 = L2 * d;
      const int64_t ncw = (((S2 + P - 1) / P) + 1) & ~(int64_t)1, S2p = ncw * P;                       // columns per rank (even), padded width
      const int64_t inner = ws.top;
      double* Rf = ws.take(S1 * S1);
      double* Xf = ws.take(S1 * S2p);
      double* mine = ws.take(L1 * std::max(L1, L2));
      double* blocked = ws.take(L1 * std::max(L1, L2) * d * d);
      CAPITAL_CHECK(capi_dlacpy(h, 0, L1, L1, R11, ld, mine, L1));
      CAPITAL_CHECK(capi_allgather(t.slice, mine, blocked, L1 * L1));
      util::block_to_cyclic_rect(blocked, Rf, L1, L1, d);                                             // (zeroes the strictly lower part)
      CAPITAL_CHECK(capi_dlacpy(h, 0, L1, L2, R12, ld, mine, L1));
      CAPITAL_CHECK(capi_allgather(t.slice, mine, blocked, L1 * L2));
      if (S2p > S2) capital::dev_zero(Xf + S1 * S2, S1 * (S2p - S2));
      CAPITAL_CHECK(capi_block_to_cyclic_full(h, blocked, Xf, L1, L2, d));
      // this rank's columns: [rank ncw, (rank + 1) ncw) of the global block -- every layer holds the same image, so the P ranks share the work
      double* Xw = Xf + (int64_t)t.rank * ncw * S1;
      CAPITAL_CHECK(capi_dtrsm(h, CAPI_LEFT, CAPI_UPPER, CAPI_TRANS, CAPI_NONUNIT, S1, ncw, 1.0, Rf, S1, Xw, S1));
      CAPITAL_CHECK(capi_allgather(t.world, Xw, Xf, S1 * ncw));                                        // in place: send = recv + rank * count
      CAPITAL_CHECK(capi_cyclic_to_block(h, blocked, Xf, L1, L2, d));
      CAPITAL_CHECK(capi_dlacpy(h, 0, L1, L2, blocked + me * L1 * L2, L1, W.p, W.ld));
      CAPITAL_CHECK(capi_dlacpy(h, 0, L1, L2, W.p, W.ld, R12, ld));
      ws.top = inner;
    }
    CRITTER_STOP(CI::trsm);
    CRITTER_START(CI::tmu);
    {
      view Wx{ws.take(W.count()), split1, split1, split2};
      capital::dev_copy(Wx.p, W.p, W.count());
      util::transpose_raw(Wx.p, Wx.count(), ws.take(Wx.count()), t, matmult::summa::relay_space(t, Wx.count(), ws));
      matmult::summa::syrk(t, CAPI_UPPER, CAPI_TRANS, -1.0, W, Wx, 1.0, A22, ws);
    }
    ws.top = mark;
    CRITTER_STOP(CI::tmu);
    potrf_rec_grid(args, t, R, ld, start + split1, split2);
  }

  template <typename ArgType, typename U>
  static void potrf_rec(ArgType& args, double* R, U ld, U start, U dim) {
    capi_handle_t h = capital::handle();
    const U split1 = dim >> args.split;
    double* R11 = R + start + start * ld;
    if (!splits(args, dim, (U)1)) {
      CRITTER_START(CI::factor_diag);
      CAPITAL_CHECK(capi_dpotrf(h, CAPI_UPPER, dim, R11, ld));
      CRITTER_STOP(CI::factor_diag);
      ++args.num_base_cases;
      return;
    }
    ++args.num_levels;
    const U split2 = dim - split1;
    double* R12 = R + start + (start + split1) * ld;
    double* R22 = R + (start + split1) + (start + split1) * ld;
    potrf_rec(args, R, ld, start, split1);
    CRITTER_START(CI::trsm);
    CAPITAL_CHECK(capi_dtrsm(h, CAPI_LEFT, CAPI_UPPER, CAPI_TRANS, CAPI_NONUNIT, split1, split2, 1.0, R11, ld, R12, ld));
    CRITTER_STOP(CI::trsm);
    CRITTER_START(CI::tmu);
    CAPITAL_CHECK(capi_dsyrk(h, CAPI_UPPER, CAPI_TRANS, split2, split1, -1.0, R12, ld, 1.0, R22, ld));
    CRITTER_STOP(CI::tmu);
    potrf_rec(args, R, ld, start + split1, split2);
  }

  // full local images of the factors (cholinv.hpp:30-46)
  template <typename ArgType, typename CommType>
  static matrix<typename ArgType::ScalarType, typename ArgType::DimensionType, rect> construct_R(ArgType& args, CommType&& CommInfo) {
    return construct(args.R, CommInfo);
  }
  template <typename ArgType, typename CommType>
  static matrix<typename ArgType::ScalarType, typename ArgType::DimensionType, rect> construct_Rinv(ArgType& args, CommType&& CommInfo) {
    if (args.solve_with_trsm) throw std::logic_error("cholinv: the TRSM mode forms no inverse (info::solve_with_trsm)");
    return construct(args.Rinv, CommInfo);
  }

private:
  // ---- what solve(), condition() and error_bounds() share: the resident factors seen as the operator A^-1 on a thin block ----
  // One resident image of a factor: column-major with leading dimension ld, or, ld == 0, the packed upper triangle.
  struct image {
    double* p = nullptr;
    int64_t ld = 0;
    bool working = false;          // the full-storage working image that SaveIntermediates keeps BESIDE the packed factor
    // the block whose first element is (i0, j0) as the thin entry points take it: a view into the packed triangle has ldt == 0 and its first column
    struct block { double* p; int64_t ldt, col0; };
    block at(int64_t i0, int64_t j0) const { return ld > 0 ? block{p + i0 + j0 * ld, ld, 0} : block{p + j0 * (j0 + 1) / 2 + i0, 0, j0}; }
  };
  enum class image_use { thin_read, full_storage, in_place };
  // Which image of a factor an operation touches: `structured` is R or Rinv as factor() returns it, `full` its full-storage working image.
  //   thin_read      the thin kernels read the factor as it lies, packed or rect
  //   full_storage   capi_dtrsm takes column-major storage: the working image, or the rect structure; refused where neither exists
  //   in_place       update() steps the working image where one is resident (and packs it again), else the factor itself, packed or rect
  // (FlushIntermediates promises that no working image outlives factor(): none is relied on there, whatever is still allocated)
  template <typename S, typename F>
  static image pick_image(S& structured, F& full, int64_t n, image_use use, const char* who) {
    constexpr bool packed = !std::is_same<typename SP::structure, rect>::value;
    if (use != image_use::thin_read && packed && IP::keep_arena && full.filled()) return image{full.data(), n, true};
    if (use == image_use::full_storage && packed)
      throw std::logic_error(std::string(who) + ": TRSM mode with Serialize + FlushIntermediates leaves only the packed R, and capi_dtrsm takes full "
                             "storage: use SaveIntermediates or NoSerialize with solve_with_trsm");
    return image{(double*)structured.data(), packed ? 0 : n, false};
  }

  static int64_t even(int64_t count) { return (count + 1) & ~(int64_t)1; }        // what arena::take makes of a count
  // The work of one operation on the factors, from args.ops: `blocks` blocks of n x CAPI_TS_MAX_RHS doubles and `tail` doubles (a sum of even() counts)
  // of odd-sized pieces.  The whole need is reserved here, before any pointer is held (reserve may free and allocate anew).  The blocks are taken FIRST:
  // each is 256 n bytes, so every one lies at a multiple of 256 bytes from the arena's base -- no operand is less aligned than in an allocation of its
  // own -- and the pieces follow them.  Nothing is zeroed and nothing needs to be: no kernel of these operations reads work that it or a kernel before it
  // in the same call has not written (beta == 0 products do not read C; capi_dresid_sym, capi_dsym_abs and capi_dlacn_block(init) only store to their
  // outputs; capi_dchud reads r columns of V and capi_dchud_inv only logged steps; the rows of w2 above h1 are never addressed; the blocks that an
  // equilibrated operation adds -- B_s, X_s, rho_s, D^-1 V -- are each written whole by capi_drow_scale2 or capi_dresid_sym before anything reads them).  On every exit,
  // exceptions included, FlushIntermediates drains the stream and releases the arena (a failure of that drain shows at the next checked call);
  // SaveIntermediates keeps the arena at its high-water mark.
  struct ops_scope {
    matmult::arena& a;
    const int64_t blk;
    ops_scope(matmult::arena& a, int64_t blocks, int64_t n, int64_t tail) : a(a), blk(n * (int64_t)CAPI_TS_MAX_RHS) { a.reserve(std::max<int64_t>(blocks * blk + tail, 2)); }
    ops_scope(const ops_scope&) = delete;
    ops_scope& operator=(const ops_scope&) = delete;
    ~ops_scope() {
      if (IP::keep_arena) return;
      if (capital::ctx().handle) (void)capi_sync(capital::ctx().handle);
      a.release();
    }
    double* block() { return a.take(blk); }
    double* piece(int64_t count) { return a.take(count); }
  };

  // ---- what solve(), condition() and error_bounds() share: the resident factors seen as the operator A^-1 on a thin block ----
  struct applier {
    capi_handle_t h;
    int64_t n, h1;
    bool subst, trsm, blocks;
    image R, Rinv, Rfull;            // Rfull: TRSM mode without substitution only
    int work_blocks;                 // n x CAPI_TS_MAX_RHS blocks of the form that the flags select
    double *w1 = nullptr, *w2 = nullptr;
  };
  // `who` opens the refusal of a form that has no image to run on
  template <typename ArgType>
  static applier make_applier(ArgType& args, const char* who) {
    const int64_t n = args.localDimension, h1 = args.top_split;
    applier c;
    c.h = capital::handle();
    c.n = n; c.h1 = h1;
    c.subst = args.solve_by_substitution; c.trsm = args.solve_with_trsm;
    c.blocks = !c.subst && !c.trsm && !args.complete_inv && h1 > 0 && h1 < n;
    c.R = pick_image(args.R, args.Rfull, n, image_use::thin_read, who);
    if (!c.trsm) c.Rinv = pick_image(args.Rinv, args.Rinvfull, n, image_use::thin_read, who);
    if (c.trsm && !c.subst) c.Rfull = pick_image(args.R, args.Rfull, n, image_use::full_storage, who);
    c.work_blocks = (c.subst || c.trsm) ? 0 : (c.blocks ? 2 : 1);
    return c;
  }
  static void take_applier_work(applier& c, ops_scope& ops) {
    if (c.work_blocks > 0) c.w1 = ops.block();
    if (c.work_blocks > 1) c.w2 = ops.block();
  }
  // the work of ONE half (apply_half) on a caller's block: the block form builds its right-hand side in w2; w1 belongs to apply_inverse
  static int half_work_blocks(const applier& c) { return c.blocks ? 1 : 0; }
  static void take_half_work(applier& c, ops_scope& ops) {
    if (c.blocks) c.w2 = ops.block();
  }
  // Xo (n x rb, ld n) <- A^-1 Bi; Bi is not written and Xo != Bi.  The two halves of apply_half, R^-T first: by substitution and in TRSM mode the
  // second runs in place on Xo, by products it reads the first half's result from the work block w1
  static void apply_inverse(const applier& c, const double* Bi, double* Xo, int64_t rb) {
    double* const y = (c.subst || c.trsm) ? Xo : c.w1;
    apply_half(c, CAPI_TRANS, Bi, y, rb);
    apply_half(c, CAPI_NOTRANS, y, Xo, rb);
  }
  // Xo (n x rb, ld n) <- R^-T Bi (trans == CAPI_TRANS) or R^-1 Bi (CAPI_NOTRANS): one half of the operator A^-1 = R^-1 R^-T, in the form the flags select.
  //   substitution / TRSM mode   Bi is copied to Xo, which is solved in place (Bi == Xo: no copy); no work block
  //   complete inverse           one product with R^-1, Xo != Bi; no work block
  //   block form (complete_inv == 0 and a top split at h1), Xo != Bi:
  //       R^-T:  y1 = R11^-T b1, y2 = R22^-T (b2 - R12^T y1)      b2 - R12^T y1 is built in the work block w2
  //       R^-1:  x2 = R22^-1 y2, x1 = R11^-1 (y1 - R12 x2)        y1 - R12 x2 is built in w2, on a copy of y1 -- or, where Bi is the work block w1
  //                                                               (apply_inverse's second half), in w1's own leading rows, which are then spent
  // A caller's Bi is never written.
  static void apply_half(const applier& c, int trans, const double* Bi, double* Xo, int64_t rb) {
    capi_handle_t h = c.h;
    const int64_t n = c.n, h1 = c.h1;
    const image &Rp = c.R, &Ip = c.Rinv;
    auto thin = [&](const image& F, int shape, int trans, int64_t i0, int64_t j0, int64_t m, int64_t k, int64_t rb, double alpha, const double* Bp,
                    double beta, double* Cp) {
      const typename image::block T = F.at(i0, j0);
      CAPITAL_CHECK(capi_dtrmm_thin(h, shape, trans, m, k, rb, alpha, T.p, T.ldt, T.col0, Bp, n, beta, Cp, n));
    };
    if (c.subst) {
      const typename image::block T = Rp.at(0, 0);
      if (Bi != Xo) CAPITAL_CHECK(capi_dlacpy(h, 0, n, rb, Bi, n, Xo, n));
      CAPITAL_CHECK(capi_dtrsm_thin(h, trans, n, rb, T.p, T.ldt, T.col0, Xo, n));
    } else if (c.trsm) {
      if (Bi != Xo) CAPITAL_CHECK(capi_dlacpy(h, 0, n, rb, Bi, n, Xo, n));
      CAPITAL_CHECK(capi_dtrsm(h, CAPI_LEFT, CAPI_UPPER, trans, CAPI_NONUNIT, n, rb, 1.0, c.Rfull.p, c.Rfull.ld, Xo, n));
    } else if (!c.blocks) {
      thin(Ip, CAPI_UPPERTRI, trans, 0, 0, n, n, rb, 1.0, Bi, 0.0, Xo);
    } else if (trans == CAPI_TRANS) {
      const int64_t h2 = n - h1;
      double* w2 = c.w2;
      thin(Ip, CAPI_UPPERTRI, CAPI_TRANS, 0, 0, h1, h1, rb, 1.0, Bi, 0.0, Xo);                          // y1 = R11^-T b1
      CAPITAL_CHECK(capi_dlacpy(h, 0, h2, rb, Bi + h1, n, w2 + h1, n));
      thin(Rp, CAPI_RECT, CAPI_TRANS, 0, h1, h1, h2, rb, -1.0, Xo, 1.0, w2 + h1);                      // b2 - R12^T y1
      thin(Ip, CAPI_UPPERTRI, CAPI_TRANS, h1, h1, h2, h2, rb, 1.0, w2 + h1, 0.0, Xo + h1);             // y2 = R22^-T (..)
    } else {
      const int64_t h2 = n - h1;
      double* t = c.w1;
      if (Bi != c.w1) { t = c.w2; CAPITAL_CHECK(capi_dlacpy(h, 0, h1, rb, Bi, n, t, n)); }
      thin(Ip, CAPI_UPPERTRI, CAPI_NOTRANS, h1, h1, h2, h2, rb, 1.0, Bi + h1, 0.0, Xo + h1);           // x2 = R22^-1 y2
      thin(Rp, CAPI_RECT, CAPI_NOTRANS, 0, h1, h1, h2, rb, -1.0, Xo + h1, 1.0, t);                     // y1 - R12 x2
      thin(Ip, CAPI_UPPERTRI, CAPI_NOTRANS, 0, 0, h1, h1, rb, 1.0, t, 0.0, Xo);                        // x1 = R11^-1 (..)
    }
  }
  // the preconditions of everything that uses the factors; `who` opens the message
  template <typename ArgType, typename CommType>
  static void require_factors(ArgType& args, CommType&& CommInfo, const std::string& who) {
    if (CommInfo.size > 1) throw std::logic_error(who + " is built for one rank: on a grid the factors are element-cyclic (factor there, solve on one rank)");
    if (!&capi_dtrmm_thin || !&capi_dresid_ts) throw std::logic_error("cholinv: this C-ABI library has no capi_dtrmm_thin / capi_dresid_ts: no solve");
    if (args.solve_by_substitution && !&capi_dtrsm_thin) throw std::logic_error("cholinv: this C-ABI library has no capi_dtrsm_thin: no solve by substitution");
    if (!args.factored || args.potrf_info != 0 || !args.R.filled() || (!args.solve_with_trsm && !args.Rinv.filled()))
      throw std::logic_error(who + ": factor() has not run or did not succeed: there are no valid factors to solve with");
    if (args.factored_trsm != args.solve_with_trsm)
      throw std::logic_error(who + ": solve_with_trsm was changed after factor(): the resident factors are those of the other mode; factor() again");
  }
  // the preconditions of the operations on L L^T + D; `who` opens the message
  template <typename ArgType, typename CommType>
  static void require_lowrank(ArgType& args, CommType&& CommInfo, const std::string& who, bool prepared) {
    if (CommInfo.size > 1) throw std::logic_error(who + " is built for one rank: on a grid the factors are element-cyclic (factor there, solve on one rank)");
    if (!&capi_dlr_diag || !&capi_drow_pow || !&capi_ddiag_add)
      throw std::logic_error("cholinv: this C-ABI library has no capi_dlr_diag / capi_drow_pow / capi_ddiag_add: no solve on the low-rank factor");
    if (!&capi_dgemtn_ts || !&capi_dresid_ts || !&capi_dtrsm_thin || !&capi_dtri_logdiag || !&capi_dsym_abs)
      throw std::logic_error("cholinv: this C-ABI library has no capi_dgemtn_ts / capi_dresid_ts / capi_dtrsm_thin / capi_dtri_logdiag / capi_dsym_abs: no solve on the low-rank factor");
    if (args.pivot_rank < 1 || !args.Lp.filled() || args.pivl.empty())
      throw std::logic_error(who + ": factor_pivoted() has not run or did not succeed: there is no low-rank factor");
    if (prepared && (!args.lowrank_prepared || args.lowrank_rank != args.pivot_rank || !args.Cap.filled() || !args.LrD.filled()))
      throw std::logic_error(who + ": lowrank_prepare() has not run on this factor or did not succeed");
  }
  static void require_equil_abi() {
    if (!&capi_dpoequ2 || !&capi_dsym_scale2 || !&capi_drow_scale2)
      throw std::logic_error("cholinv: this C-ABI library has no capi_dpoequ2 / capi_dsym_scale2 / capi_drow_scale2: no equilibration");
  }
  static void require_bounds_abi() {
    if (!&capi_dsym_abs || !&capi_dberr || !&capi_dcolamax || !&capi_dlacn_block || !&capi_dlacn_state_bytes || !&capi_dresid_sym)
      throw std::logic_error("cholinv: this C-ABI library has no capi_dsym_abs / capi_dberr / capi_dcolamax / capi_dlacn_block: no condition estimate, no error bounds");
  }
  // the work of the estimator: its two n x CAPI_TS_MAX_RHS blocks, then its state and the 4 CAPI_TS_MAX_RHS small results of condition() / error_bounds()
  struct estimator {
    double *v1, *v2, *state, *small;
    static int64_t state_count(int64_t n) { return (int64_t)((capi_dlacn_state_bytes(n, CAPI_TS_MAX_RHS) + 7) / 8); }
    static int64_t tail(int64_t n) { return even(state_count(n)) + 4 * (int64_t)CAPI_TS_MAX_RHS; }
    estimator(ops_scope& ops, int64_t n) : v1(ops.block()), v2(ops.block()), state(ops.piece(state_count(n))), small(ops.piece(4 * (int64_t)CAPI_TS_MAX_RHS)) {}
  };
  // the estimator's loop over the shared operator: est (device, rb doubles) <- the estimates for the weight columns Wt (or none).  Returns the products
  static int estimate(const estimator& es, const applier& ap, int64_t rb, const double* Wt, double* est) {
    const int64_t n = ap.n;
    double *v = es.v1, *y = es.v2;
    int active = 0, applies = 0;
    CAPITAL_CHECK(capi_dlacn_block(ap.h, 1, n, rb, v, n, Wt, n, es.state, est, &active));
    while (active > 0) {
      apply_inverse(ap, v, y, rb);
      ++applies;
      std::swap(v, y);
      CAPITAL_CHECK(capi_dlacn_block(ap.h, 0, n, rb, v, n, Wt, n, es.state, est, &active));
    }
    return applies;
  }

  // event slots of the top-level overlap (matmult::summa's pipe uses slots below 1000)
  static constexpr int EV_INPUT_HEAD = 1020, EV_INPUT_REST = 1021, EV_TOP_R12 = 1022, EV_EARLY_PACK = 1023, EV_INPUT_MID = 1019;
  static constexpr int EV_BC_POTRF = 1008, EV_BC_SCATTER = 1009;      // NoReplicationOverlap: scatter of R beside trtri

  // cholinv.hpp:93: a block of local order dim on a d x d slice splits unless its aggregate fits the base case or its leading part is shorter than the split
  template <typename ArgType, typename U>
  static bool splits(const ArgType& args, U dim, U d) { return !(((dim * d) <= args.bcDimension) || ((dim >> args.split) < args.split)); }

  // the base-case size rule (cholinv.hpp:15-18) and the dimension fields of a factorisation of A, either mode
  template <typename MatrixType, typename ArgType, typename CommType>
  static void set_dimensions(const MatrixType& A, ArgType& args, CommType&& CommInfo) {
    using U = typename ArgType::DimensionType;
    const U localDimension = A.num_rows_local();
    U bcDimLocal = (U)(CommInfo.c * CommInfo.d);
    U bcMult = args.bc_mult_dim;
    if (bcMult < 0) { bcMult = -bcMult; for (U i = 0; i < bcMult; ++i) bcDimLocal *= 2; } else { for (U i = 0; i < bcMult; ++i) bcDimLocal /= 2; }
    bcDimLocal = std::max<U>(1, bcDimLocal);
    bcDimLocal = std::min<U>(localDimension, bcDimLocal);
    bcDimLocal = localDimension / bcDimLocal;
    args.localDimension = args.trueLocalDimension = localDimension;
    args.globalDimension = args.trueGlobalDimension = A.num_rows_global();
    args.bcDimension = (U)CommInfo.d * bcDimLocal;
    args.num_base_cases = args.num_levels = 0;
  }

  // Registers R and, with_inverse, R^-1 for a factorisation of A, with their full-storage images when the returned structure is packed, and
  // returns the images that the recursion works in.  No memset follows: a registered block is zero from matrix::allocate, and no
  // factorisation ever stores a non-zero where the result must be zero (strictly-lower parts; the skipped R^-1_12 at the top level), so a block
  // that an earlier call left registered is still zero there.
  struct working { double *R = nullptr, *Rinv = nullptr; };
  template <typename MatrixType, typename ArgType, typename CommType>
  static working working_images(const MatrixType& A, ArgType& args, CommType&& CommInfo, bool with_inverse) {
    constexpr bool packed = !std::is_same<typename SP::structure, rect>::value;
    auto reg = [&](auto& m) { m._register_(A.num_columns_global(), A.num_rows_global(), CommInfo.d, CommInfo.d); };
    reg(args.R);
    if (with_inverse) reg(args.Rinv);
    if (packed) { reg(args.Rfull); if (with_inverse) reg(args.Rinvfull); }
    working w;
    w.R = packed ? args.Rfull.data() : (double*)args.R.data();
    if (with_inverse) w.Rinv = packed ? args.Rinvfull.data() : (double*)args.Rinv.data();
    return w;
  }

  // columns [x0,x1), rows [y0,y1) of a full local image into the packed (uppertri) factor; shape = what is copied per column
  template <typename ArgType>
  static void pack_block(ArgType&, int shape, const double* full, double* packed_dst, int64_t ld, int64_t x0, int64_t x1, int64_t y0,
                         int64_t y1) {
    CAPITAL_CHECK(capi_serialize_shape(capital::handle(), shape, CAPI_RECT, CAPI_UPPERTRI, full, ld, ld, packed_dst, ld, ld,
                                       x0, x1, y0, y1, x0, x1, y0, y1));
  }

  template <typename M, typename CommType>
  static matrix<typename M::ScalarType, typename M::DimensionType, rect> construct(M& src, CommType&& CommInfo) {
    const auto ld = src.num_rows_local();
    matrix<typename M::ScalarType, typename M::DimensionType, rect> ret(src.num_columns_global(), src.num_rows_global(), CommInfo.d, CommInfo.d);
    serialize<typename SP::structure, rect>::invoke(src, ret, 0, ld, 0, ld, 0, ld, 0, ld);
    return ret;
  }

  template <typename ArgType, typename CommType, typename U>
  static void invoke(ArgType& args, CommType&& t, double* R, double* Ri, U ld, U start, U localDim, U globalDim) {
    using matmult::view;
    capi_handle_t h = capital::handle();
    const U split1 = localDim >> args.split;
    if (!splits(args, localDim, (U)t.d)) {
      CRITTER_START(CI::factor_diag);
      base_case(args, t, R, Ri, ld, start, localDim);
      CRITTER_STOP(CI::factor_diag);
      return;
    }
    ++args.num_levels;
    const U split2 = localDim - split1;
    const bool single = (t.d == 1 && t.c == 1);
    matmult::arena& ws = args.work;
    // local blocks (column-major, column index first in the reference's (X,Y) convention)
    view R11i{Ri + start + start * ld, ld, split1, split1};
    view A12{R + start + (start + split1) * ld, ld, split1, split2};
    view A22{R + (start + split1) + (start + split1) * ld, ld, split2, split2};
    view R22i{Ri + (start + split1) + (start + split1) * ld, ld, split2, split2};
    view I12{Ri + start + (start + split1) * ld, ld, split1, split2};

    invoke(args, t, R, Ri, ld, start, split1, globalDim >> 1);                          // 1
    if (start == 0 && args.input_lead > 0 && split1 == args.input_lead) CAPITAL_CHECK(capi_event_wait(h, EV_INPUT_MID));   // rest of the input's left half

    const bool top = (localDim == args.localDimension) && args.early_split == split1;
    if (top) CAPITAL_CHECK(capi_event_wait(h, EV_INPUT_REST));                          // the input's right part has landed
    CRITTER_START(CI::trsm);                                                            // 2
    const int64_t mark = ws.top;
    {
      view W{ws.take((int64_t)split1 * split2), split1, split1, split2};
      if (single) {
        CAPITAL_CHECK(capi_dtrmm_oop(h, CAPI_LEFT, CAPI_UPPER, CAPI_TRANS, CAPI_NONUNIT, split1, split2, 1.0, R11i.p, ld, A12.p, ld, W.p, W.ld));
      } else {
        // partner-exchanged copy of R11^-1 (cholinv.hpp:116-117)
        view Tx{ws.take((int64_t)split1 * split1), split1, split1, split1};
        // (on a grid that relays every rank joins the exchange with the same, packed, count: the diagonal ranks carry other pairs' units)
        const int64_t np = matmult::summa::tri_count(split1);
        if ((t.x == t.y && !t.multipath) || !matmult::summa::packed_comm()) {
          CAPITAL_CHECK(capi_dlacpy(h, 0, split1, split1, R11i.p, ld, Tx.p, Tx.ld));
          util::transpose_raw(Tx.p, Tx.count(), ws.take(Tx.count()), t, matmult::summa::relay_space(t, Tx.count(), ws));
        } else if (t.x == t.y) {
          CAPITAL_CHECK(capi_dlacpy(h, 0, split1, split1, R11i.p, ld, Tx.p, Tx.ld));
          util::transpose_raw(nullptr, np, nullptr, t, matmult::summa::relay_space(t, np, ws));
        } else {
          // the exchanged block is upper triangular: it crosses the link packed (n(n+1)/2) and is unpacked on arrival;
          // the strictly-lower half of Tx is never read (TRMM masks by selection)
          double* pk = ws.take(np);
          matmult::summa::pack_tri(R11i, CAPI_UPPER, pk);
          util::transpose_raw(pk, np, ws.take(np), t, matmult::summa::relay_space(t, np, ws));
          matmult::summa::unpack_tri(pk, CAPI_UPPER, Tx);
        }
        matmult::summa::trmm(t, CAPI_LEFT, CAPI_UPPER, CAPI_TRANS, CAPI_NONUNIT, 1.0, Tx, A12, W, ws);
      }
      CAPITAL_CHECK(capi_dlacpy(h, 0, split1, split2, W.p, W.ld, A12.p, ld));              // R12 into R (cholinv.hpp:122)
      CRITTER_STOP(CI::trsm);

      CRITTER_START(CI::tmu);                                                           // 3
      if (single) {
        CAPITAL_CHECK(capi_dgemmt(h, CAPI_UPPER, CAPI_TRANS, CAPI_NOTRANS, split2, split1, -1.0, W.p, W.ld, W.p, W.ld, 1.0, A22.p, ld));
      } else {
        view Wx{ws.take(W.count()), split1, split1, split2};
        capital::dev_copy(Wx.p, W.p, W.count());
        util::transpose_raw(Wx.p, Wx.count(), ws.take(Wx.count()), t, matmult::summa::relay_space(t, Wx.count(), ws));
        matmult::summa::syrk(t, CAPI_UPPER, CAPI_TRANS, -1.0, W, Wx, 1.0, A22, ws);
      }
      // R11, R12 and Rinv11 are final after step 2: with packed factors the top level packs them on the second stream, at once, beside
      // the trailing update and the trailing block's recursion (factor() packs the rest and joins EV_EARLY_PACK)
      if (top && !std::is_same<typename SP::structure, rect>::value) {
        CAPITAL_CHECK(capi_event_record(h, EV_TOP_R12));
        CAPITAL_CHECK(capi_stream_select(h, 1));
        CAPITAL_CHECK(capi_event_wait(h, EV_TOP_R12));
        pack_block(args, CAPI_UPPERTRI, R, (double*)args.R.data(), ld, (U)0, split1, (U)0, split1);
        pack_block(args, CAPI_RECT, R, (double*)args.R.data(), ld, split1, ld, (U)0, split1);
        pack_block(args, CAPI_UPPERTRI, Ri, (double*)args.Rinv.data(), ld, (U)0, split1, (U)0, split1);
        CAPITAL_CHECK(capi_event_record(h, EV_EARLY_PACK));
        CAPITAL_CHECK(capi_stream_select(h, 0));
      }
      ws.top = mark;
      CRITTER_STOP(CI::tmu);
    }

    invoke(args, t, R, Ri, ld, start + split1, split2, split2 * (U)t.d);                // 4

    CRITTER_START(CI::tmu);                                                             // 5
    if (!(!args.complete_inv && (globalDim == args.trueGlobalDimension))) {
      const int64_t mark = ws.top;
      view W2{ws.take((int64_t)split1 * split2), split1, split1, split2};
      matmult::summa::trmm(t, CAPI_LEFT, CAPI_UPPER, CAPI_NOTRANS, CAPI_NONUNIT, 1.0, R11i, A12, W2, ws);
      if (single) {
        matmult::summa::trmm(t, CAPI_RIGHT, CAPI_UPPER, CAPI_NOTRANS, CAPI_NONUNIT, -1.0, R22i, W2, I12, ws);
      } else {
        view W3{ws.take(W2.count()), split1, split1, split2};
        matmult::summa::trmm(t, CAPI_RIGHT, CAPI_UPPER, CAPI_NOTRANS, CAPI_NONUNIT, -1.0, R22i, W2, W3, ws);
        CAPITAL_CHECK(capi_dlacpy(h, 0, split1, split2, W3.p, W3.ld, I12.p, ld));
      }
      ws.top = mark;
    }
    CRITTER_STOP(CI::tmu);
  }

  // cholinv.hpp:170-183 + policy.h:160-514
  template <typename ArgType, typename CommType, typename U>
  static void base_case(ArgType& args, CommType&& t, double* R, double* Ri, U ld, U start, U localDim) {
    capi_handle_t h = capital::handle();
    ++args.num_base_cases;
    double* Rb = R + start + start * ld;
    double* Ib = Ri + start + start * ld;
    if (t.d == 1) {
      // the whole diagonal block is local: factor and invert it in place (every layer holds the same block)
      CAPITAL_CHECK(capi_dpotrf_trtri(h, localDim, Rb, ld, Ib, ld));
      return;
    }
    const int64_t d = (int64_t)t.d, L = (int64_t)localDim, agg = L * d;
    // `span`: the aggregate minus the global padding when this is the last block (policy.h:196)
    const int64_t span = ((start + localDim) != args.trueLocalDimension) ? agg : agg - (args.trueLocalDimension * d - args.trueGlobalDimension);
    // With Serialize the pieces travel PACKED, L (L + 1) / 2 doubles instead of L^2 (policy.h:176: the messages are
    // base_case_table[...].num_elems() of an uppertri block) and are re-indexed by the triangle forms (util.hpp:57-102,167-201).
    constexpr bool packed_msg = !std::is_same<typename SP::structure, rect>::value;
    const int64_t piece = packed_msg ? L * (L + 1) / 2 : L * L;
    auto pack_piece = [&](const double* blk, double* dst) {          // local block (ld) -> message piece
      if (packed_msg) CAPITAL_CHECK(capi_serialize_shape(h, CAPI_UPPERTRI, CAPI_RECT, CAPI_UPPERTRI, blk, ld, ld, dst, L, L, 0, L, 0, L, 0, L, 0, L));
      else CAPITAL_CHECK(capi_dlacpy(h, 0, L, L, blk, ld, dst, L));
    };
    auto unpack_piece = [&](const double* src, double* blk) {        // message piece -> local block (ld); strictly-lower part stays zero
      if (packed_msg) CAPITAL_CHECK(capi_serialize_shape(h, CAPI_UPPERTRI, CAPI_UPPERTRI, CAPI_RECT, src, L, L, blk, ld, ld, 0, L, 0, L, 0, L, 0, L));
      else CAPITAL_CHECK(capi_dlacpy(h, 0, L, L, src, L, blk, ld));
    };
    auto to_cyclic = [&](const double* blocked, double* cyc) {
      if (packed_msg) CAPITAL_CHECK(capi_block_to_cyclic_tri(h, blocked, cyc, L, d));
      else util::block_to_cyclic_rect(blocked, cyc, L, L, d);
    };
    auto to_blocked = [&](double* blocked, const double* cyc) {
      if (packed_msg) CAPITAL_CHECK(capi_cyclic_to_block_tri(h, blocked, cyc, L, d));
      else util::cyclic_to_block_rect(blocked, cyc, L, L, d);
    };
    matmult::arena& ws = args.work;
    const int64_t mark = ws.top;
    double* mine = ws.take(piece);        // this rank's piece of A (in), then of R (out)
    double* minei = ws.take(piece);       // this rank's piece of R^-1 (out)
    const int64_t me = (int64_t)t.x + d * (int64_t)t.y;            // rank inside `slice` (topology.h:85,93-94)
    const bool worker = BP::every_layer || t.z == 0;
    if (BP::gather_all) {
      // ReplicateCommComp (policy.h:160-224) / ReplicateComp (:226-305): Allgather over the slice, every rank of the (or of
      // layer 0's) slice re-indexes, factors and inverts the aggregate and keeps its own piece
      double* blocked = ws.take(piece * d * d);
      double* cyc = ws.take(agg * agg);
      double* cyci = ws.take(agg * agg);
      if (worker) {
        pack_piece(Rb, mine);
        CAPITAL_CHECK(capi_allgather(t.slice, mine, blocked, piece));                      // C5, policy.h:176,240
        to_cyclic(blocked, cyc);
        capital::dev_zero(cyci, agg * agg);
        CAPITAL_CHECK(capi_dpotrf_trtri(h, span, cyc, agg, cyci, agg));                    // policy.h:199-201
      }
      if (!BP::every_layer) {                                                              // C7, policy.h:288-289: the aggregates travel
        CAPITAL_CHECK(capi_bcast(t.depth, cyc, agg * agg, 0));
        CAPITAL_CHECK(capi_bcast(t.depth, cyci, agg * agg, 0));
      }
      // util::cyclic_to_local (util.hpp:131-164): this rank's element-cyclic piece of both factors
      to_blocked(blocked, cyc);
      unpack_piece(blocked + me * piece, Rb);
      to_blocked(blocked, cyci);
      unpack_piece(blocked + me * piece, Ib);
    } else {
      // NoReplication (policy.h:307-414) / NoReplicationOverlap (:416-514): layer 0 gathers the pieces on the slice's rank 0,
      // which alone factors the aggregate and scatters the pieces of R and of R^-1; every rank then hands its two pieces down
      // its depth fibre.  Overlap: R's pieces are scattered (stream 1) WHILE the root inverts (compute stream) -- the
      // reference's MPI_Iscatter around trtri (:470-488).
      const bool root = worker && me == 0;
      double *blocked = nullptr, *cyc = nullptr, *cyci = nullptr;
      if (root) { blocked = ws.take(piece * d * d); cyc = ws.take(agg * agg); cyci = ws.take(agg * agg); }
      double* blockedi = (root && BP::overlap) ? ws.take(piece * d * d) : blocked;         // R's pieces are still in flight while R^-1's are cut
      if (worker) {
        pack_piece(Rb, mine);
        CAPITAL_CHECK(capi_gather(t.slice, mine, blocked, piece, 0));                      // C6, policy.h:322-332
        if (!BP::overlap) {
          if (root) {
            to_cyclic(blocked, cyc);
            capital::dev_zero(cyci, agg * agg);
            CAPITAL_CHECK(capi_dpotrf_trtri(h, span, cyc, agg, cyci, agg));                // :353,367 (the two scatters carry finished factors)
            to_blocked(blocked, cyc);
          }
          CAPITAL_CHECK(capi_scatter(t.slice, blocked, mine, piece, 0));                   // :361-365
          if (root) to_blocked(blocked, cyci);
          CAPITAL_CHECK(capi_scatter(t.slice, blocked, minei, piece, 0));                  // :373-377
        } else {
          if (root) {
            to_cyclic(blocked, cyc);
            CAPITAL_CHECK(capi_dpotrf(h, CAPI_UPPER, span, cyc, agg));                     // :462
            capital::dev_zero(cyci, agg * agg);
            CAPITAL_CHECK(capi_dlacpy(h, 1, span, span, cyc, agg, cyci, agg));             // :463 (memcpy to scratch; upper part is all trtri reads)
            to_blocked(blocked, cyc);
          }
          // every rank of the slice posts the scatter of R on stream 1, behind what the compute stream has queued so far
          CAPITAL_CHECK(capi_event_record(h, EV_BC_POTRF));
          CAPITAL_CHECK(capi_stream_select(h, 1));
          CAPITAL_CHECK(capi_event_wait(h, EV_BC_POTRF));
          CAPITAL_CHECK(capi_scatter(t.slice, blocked, mine, piece, 0));                   // :470-474 (MPI_Iscatter)
          CAPITAL_CHECK(capi_event_record(h, EV_BC_SCATTER));
          CAPITAL_CHECK(capi_stream_select(h, 0));
          if (root) {
            CAPITAL_CHECK(capi_dtrtri(h, CAPI_UPPER, CAPI_NONUNIT, span, cyci, agg));      // :476, beside the scatter
            CAPITAL_CHECK(capi_dtrizero(h, CAPI_UPPER, agg, cyci, agg));
            to_blocked(blockedi, cyci);
          }
          // one communicator, one stream at a time: the second scatter is issued only behind the first (MPI_Wait, :488)
          CAPITAL_CHECK(capi_event_wait(h, EV_BC_SCATTER));
          CAPITAL_CHECK(capi_scatter(t.slice, blockedi, minei, piece, 0));                 // :480-484
        }
      }
      CAPITAL_CHECK(capi_bcast(t.depth, mine, piece, 0));                                  // C7, policy.h:398-399,491,505: own pieces travel
      CAPITAL_CHECK(capi_bcast(t.depth, minei, piece, 0));
      unpack_piece(mine, Rb);
      unpack_piece(minei, Ib);
    }
    ws.top = mark;
  }
};

}  // namespace cholesky

#endif  // CAPITAL_CHOLESKY_CHOLINV_H_
