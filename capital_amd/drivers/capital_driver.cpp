// capital_driver.cpp -- C-ABI over the host-side C++ layer (capital_amd/src): what bench.py, the parity tests and a
// foreign-language caller bind.  It plays the part of the reference's bench mains (bench/cholesky/cholinv.cpp:8-71,
// bench/qr/cacqr.cpp:8-77) split into create / generate / factor / validate steps so that a launcher can time factor()
// alone.  Policy templates are instantiated for every combination the reference exposes.
#include <memory>

#include "../src/alg/cholesky/cholinv/cholinv.h"
#include "../src/alg/qr/cacqr/cacqr.h"
#include "../test/cholesky/validate.h"
#include "../test/qr/validate.h"

namespace {

CAPITAL_RANK_LOCAL std::string g_err;      // (per rank: thread-local in the ranks-as-threads rehearsal build)
template <typename F>
int guarded(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

using T = double;
using U = int64_t;
using MatrixType = matrix<T, U, rect>;

// the local block of M, as it lies on the device, into host memory
template <class M>
void fetch(const M& m, double* host) {
  CAPITAL_CHECK(capi_memcpy_d2h(capital::handle(), host, m.data(), sizeof(double) * (size_t)m.num_elems()));
}

struct cholinv_problem {
  virtual ~cholinv_problem() {}
  virtual void generate() = 0;
  virtual void set_A(const double* host) = 0;
  virtual void factor() = 0;
  virtual double residual() = 0;
  virtual void get(int which, double* host) = 0;
  virtual void get_rows(int which, int64_t count, const int64_t* rows, double* host) = 0;
  virtual void dims(int64_t* nloc, int* x, int* y, int* z, int* d, int* c) = 0;
  virtual void stats(int64_t* bc, int64_t* levels, int64_t* bcdim) = 0;
  virtual void set_trsm_mode(bool on) = 0;
  virtual void set_solve_substitution(bool on) = 0;
  virtual void solve(int64_t r, const double* B_host, double* X_host, double* resnorm_host, int refine) = 0;
  virtual void rcond(double* rcond, double* anorm1, int* applies) = 0;
  virtual void error_bounds(int64_t r, const double* B_host, double* ferr_host, double* berr_host, int* applies) = 0;
  virtual void update(int64_t r, const double* V_host, int sign) = 0;
  virtual void factor_pivoted(double rtol, int64_t max_rank, int64_t* rank, double* resid_trace, double* thresh) = 0;
  virtual void get_pivoted(double* L_host, int* piv_host, double* d_host) = 0;
  virtual void apply(int op, int64_t r, const double* B_host, double* Y_host) = 0;
  virtual void quadratic_forms(int64_t r, const double* B_host, double* q_host) = 0;
  virtual void logdet(double* v) = 0;
  virtual void inverse_diagonal(double* d_host) = 0;
  virtual void equilibrate(double thresh, int* scaled, double* scond, double* amax, double* dscale_host) = 0;
  virtual void unequilibrate() = 0;
  virtual void lowrank_prepare(double shift, const double* diag_host, int use_schur, double* logdet, double* cnorm1) = 0;
  virtual void lowrank_solve(int64_t r, const double* B_host, double* X_host, double* resnorm_host) = 0;
  virtual void lowrank_quadratic_forms(int64_t r, const double* B_host, double* q_host) = 0;
};

template <class Alg>
struct cholinv_impl : cholinv_problem {
  topo::square grid;
  MatrixType A;
  typename Alg::template info<T, U> pack;
  cholinv_impl(int64_t n, int c, int layout, int chunks, int complete_inv, int split, int bc_mult)
      : grid(capital::world(), (size_t)c, (size_t)layout, (size_t)chunks), A(n, n, grid.d, grid.d), pack(complete_inv, split, bc_mult, 'U') {}
  // (a new matrix is not equilibrated, whatever the one before it was)
  void generate() override { A.distribute_symmetric(grid.x, grid.y, grid.d, grid.d, grid.rank / grid.c, true); pack.equilibrated = false; }   // bench/cholesky/cholinv.cpp:40
  void set_A(const double* host) override { A.from_host(host); pack.equilibrated = false; }
  void factor() override { Alg::factor(A, pack, grid); }
  double residual() override { return cholesky::validate<Alg>::residual(A, pack, grid); }
  void get(int which, double* host) override {
    if (which == 0) { fetch(A, host); return; }
    fetch(which == 1 ? Alg::construct_R(pack, grid) : Alg::construct_Rinv(pack, grid), host);
  }
  // local rows rows[0..count) of R (which = 1) or R^-1 (2), column-major count x n_loc: a sample of a factor that is too large
  // to fetch whole (n = 65536 on one GPU: 32 GiB)
  void get_rows(int which, int64_t count, const int64_t* rows, double* host) override {
    if (which != 1 && which != 2) throw std::invalid_argument("cholinv get_rows: which must be 1 (R) or 2 (Rinv)");
    auto M = which == 1 ? Alg::construct_R(pack, grid) : Alg::construct_Rinv(pack, grid);
    const int64_t m = M.num_rows_local(), n = M.num_columns_local();
    for (int64_t k = 0; k < count; ++k)
      if (rows[k] < 0 || rows[k] >= m) throw std::invalid_argument("cholinv get_rows: row outside the local block");
    if (count <= 0) return;
    double* tmp = capital::dev_alloc(count * n);
    for (int64_t k = 0; k < count; ++k) CAPITAL_CHECK(capi_dlacpy(capital::handle(), 0, 1, n, M.data() + rows[k], m, tmp + k, count));
    CAPITAL_CHECK(capi_memcpy_d2h(capital::handle(), host, tmp, sizeof(double) * (size_t)(count * n)));
    capital::dev_free(tmp);
  }
  void dims(int64_t* nloc, int* x, int* y, int* z, int* d, int* c) override {
    *nloc = A.num_rows_local(); *x = (int)grid.x; *y = (int)grid.y; *z = (int)grid.z; *d = (int)grid.d; *c = (int)grid.c;
  }
  void stats(int64_t* bc, int64_t* levels, int64_t* bcdim) override { *bc = pack.num_base_cases; *levels = pack.num_levels; *bcdim = pack.bcDimension; }
  void set_trsm_mode(bool on) override { pack.solve_with_trsm = on; }
  void set_solve_substitution(bool on) override { pack.solve_by_substitution = on; }
  // A X = B on the factors of the last factor(): B_host n x r column-major, X_host receives n x r, resnorm_host (may be NULL: no residual
  // pass) the r norms ||b_j - A x_j||_2
  void solve(int64_t r, const double* B_host, double* X_host, double* resnorm_host, int refine) override {
    if (r < 1 || !B_host || !X_host) throw std::invalid_argument("cholinv solve: r >= 1 right-hand sides, B and X expected");
    MatrixType B(r, A.num_rows_global(), 1, 1);
    B.from_host(B_host);
    Alg::solve(A, B, pack, grid, refine, resnorm_host != nullptr);
    fetch(pack.X, X_host);
    if (resnorm_host) std::memcpy(resnorm_host, pack.solve_residual_norms.data(), sizeof(double) * (size_t)r);
  }
  void rcond(double* rcond, double* anorm1, int* applies) override {
    if (!rcond) throw std::invalid_argument("cholinv rcond: a place for the result expected");
    Alg::condition(A, pack, grid);
    *rcond = pack.rcond;
    if (anorm1) *anorm1 = pack.anorm1;
    if (applies) *applies = pack.lacn_applies;
  }
  // bounds for the X that the last solve left on the device, B_host the n x r right-hand sides of that solve
  void error_bounds(int64_t r, const double* B_host, double* ferr_host, double* berr_host, int* applies) override {
    if (r < 1 || !B_host || !ferr_host || !berr_host) throw std::invalid_argument("cholinv error_bounds: r >= 1 right-hand sides, B, ferr and berr expected");
    MatrixType B(r, A.num_rows_global(), 1, 1);
    B.from_host(B_host);
    Alg::error_bounds(A, B, pack, grid);
    std::memcpy(ferr_host, pack.solve_ferr.data(), sizeof(double) * (size_t)r);
    std::memcpy(berr_host, pack.solve_berr.data(), sizeof(double) * (size_t)r);
    if (applies) *applies = pack.lacn_applies;
  }
  // A <- A + sign V V^T on the factors of the last factor(): V_host n x r column-major
  void update(int64_t r, const double* V_host, int sign) override {
    if (r < 1 || !V_host) throw std::invalid_argument("cholinv update: r >= 1 columns and V expected");
    MatrixType V(r, A.num_rows_global(), 1, 1);
    V.from_host(V_host);
    Alg::update(A, V, pack, grid, sign);
  }
  // A ~= L L^T by the pivoted partial Cholesky; rtol 0: LAPACK's default threshold, max_rank 0: min(n, CAPI_PCHOL_MAX_RANK)
  void factor_pivoted(double rtol, int64_t max_rank, int64_t* rank, double* resid_trace, double* thresh) override {
    if (max_rank < 0) throw std::invalid_argument("cholinv factor_pivoted: max_rank >= 0 expected (0: the default)");
    pack.pivot_rtol = rtol;
    pack.pivot_max_rank = max_rank;
    // (the results are handed out whether or not the call throws at rank 0)
    auto hand_out = [&] { if (rank) *rank = pack.pivot_rank; if (resid_trace) *resid_trace = pack.resid_trace; if (thresh) *thresh = pack.pivot_thresh; };
    try { Alg::factor_pivoted(A, pack, grid); } catch (...) { hand_out(); throw; }
    hand_out();
  }
  // of the last factor_pivoted(): L n x rank column-major, piv n ints, d n doubles (each may be NULL)
  void get_pivoted(double* L_host, int* piv_host, double* d_host) override {
    if (pack.pivot_rank < 1 || !pack.Lp.filled() || pack.pivl.empty()) throw std::logic_error("cholinv get_pivoted: factor_pivoted() has not run or did not succeed");
    const int64_t n = A.num_rows_local();
    if (L_host) CAPITAL_CHECK(capi_memcpy_d2h(capital::handle(), L_host, pack.Lp.data(), sizeof(double) * (size_t)(n * pack.pivot_rank)));
    if (piv_host) std::memcpy(piv_host, pack.pivl.data(), sizeof(int) * (size_t)n);
    if (d_host) fetch(pack.Dres, d_host);
  }
  // Y = op B on the factors of the last factor(): op 0 R, 1 R^T, 2 R^-1, 3 R^-T; B_host n x r column-major, Y_host receives n x r
  void apply(int op, int64_t r, const double* B_host, double* Y_host) override {
    if (op < 0 || op > 3 || r < 1 || !B_host || !Y_host) throw std::invalid_argument("cholinv apply: op 0..3 (R, RT, Rinv, RinvT), r >= 1 columns, B and Y expected");
    static const cholesky::factor_op ops[4] = {cholesky::factor_op::R, cholesky::factor_op::Rt, cholesky::factor_op::Rinv, cholesky::factor_op::RinvT};
    MatrixType B(r, A.num_rows_global(), 1, 1);
    B.from_host(B_host);
    Alg::apply(B, pack, grid, ops[op]);
    fetch(pack.Y, Y_host);
  }
  // q_host[j] = b_j^T A^-1 b_j
  void quadratic_forms(int64_t r, const double* B_host, double* q_host) override {
    if (r < 1 || !B_host || !q_host) throw std::invalid_argument("cholinv quadratic_forms: r >= 1 columns, B and a place for the r results expected");
    MatrixType B(r, A.num_rows_global(), 1, 1);
    B.from_host(B_host);
    Alg::quadratic_forms(B, pack, grid);
    std::memcpy(q_host, pack.quad.data(), sizeof(double) * (size_t)r);
  }
  void logdet(double* v) override {
    if (!v) throw std::invalid_argument("cholinv logdet: a place for the result expected");
    Alg::log_determinant(pack, grid);
    *v = pack.logdet;
  }
  void inverse_diagonal(double* d_host) override {
    if (!d_host) throw std::invalid_argument("cholinv inverse_diagonal: a place for the n results expected");
    Alg::inverse_diagonal(pack, grid);
    std::memcpy(d_host, pack.inv_diag.data(), sizeof(double) * pack.inv_diag.size());
  }
  // A <- D^-1 A D^-1 where dlaqsy's rule asks for it: *scaled, the scond and amax the call found, and (dscale_host may be NULL) the n scale factors in
  // force afterwards: D's diagonal when it scaled, ones when it did not
  void equilibrate(double thresh, int* scaled, double* scond, double* amax, double* dscale_host) override {
    const bool did = Alg::equilibrate(A, pack, grid, thresh);
    if (scaled) *scaled = did ? 1 : 0;
    if (scond) *scond = pack.scond;
    if (amax) *amax = pack.amax;
    if (dscale_host) {
      const size_t n = (size_t)A.num_rows_local();
      if (did) std::memcpy(dscale_host, pack.dscale.data(), sizeof(double) * n);
      else std::fill(dscale_host, dscale_host + n, 1.0);
    }
  }
  void unequilibrate() override { Alg::unequilibrate(A, pack, grid); }
  // M = L L^T + D on the factor of the last factor_pivoted(): d = shift + diag_host (n doubles, may be NULL) + (use_schur: its remaining Schur diagonal)
  void lowrank_prepare(double shift, const double* diag_host, int use_schur, double* logdet, double* cnorm1) override {
    pack.lowrank_shift = shift;
    pack.lowrank_use_schur = use_schur != 0;
    pack.lowrank_use_diag = diag_host != nullptr;
    if (diag_host) {
      pack.LrDiagIn._register_(1, A.num_rows_local(), 1, 1);
      pack.LrDiagIn.from_host(diag_host);
    }
    Alg::lowrank_prepare(pack, grid);
    if (logdet) *logdet = pack.lowrank_logdet;
    if (cnorm1) *cnorm1 = pack.lowrank_cnorm1;
  }
  // X_host (n x r) <- M^-1 B_host; resnorm_host (may be NULL: no residual pass) the r norms ||b_j - M x_j||_2
  void lowrank_solve(int64_t r, const double* B_host, double* X_host, double* resnorm_host) override {
    if (r < 1 || !B_host || !X_host) throw std::invalid_argument("cholinv lowrank_solve: r >= 1 right-hand sides, B and X expected");
    MatrixType B(r, A.num_rows_global(), 1, 1);
    B.from_host(B_host);
    Alg::lowrank_solve(B, pack, grid, resnorm_host != nullptr);
    fetch(pack.LrX, X_host);
    if (resnorm_host) std::memcpy(resnorm_host, pack.lowrank_residual_norms.data(), sizeof(double) * (size_t)r);
  }
  // q_host[j] = b_j^T M^-1 b_j
  void lowrank_quadratic_forms(int64_t r, const double* B_host, double* q_host) override {
    if (r < 1 || !B_host || !q_host) throw std::invalid_argument("cholinv lowrank_quadratic_forms: r >= 1 columns, B and a place for the r results expected");
    MatrixType B(r, A.num_rows_global(), 1, 1);
    B.from_host(B_host);
    Alg::lowrank_quadratic_forms(B, pack, grid);
    std::memcpy(q_host, pack.lowrank_quad.data(), sizeof(double) * (size_t)r);
  }
};

template <class SP, class IP>
cholinv_problem* make_cholinv(int bc_policy, int64_t n, int c, int layout, int chunks, int ci, int split, int bcm) {
  namespace P = cholesky::policy::cholinv;
  switch (bc_policy) {
    case 0: return new cholinv_impl<cholesky::cholinv<SP, IP, P::ReplicateCommComp>>(n, c, layout, chunks, ci, split, bcm);
    case 1: return new cholinv_impl<cholesky::cholinv<SP, IP, P::ReplicateComp>>(n, c, layout, chunks, ci, split, bcm);
    case 2: return new cholinv_impl<cholesky::cholinv<SP, IP, P::NoReplication>>(n, c, layout, chunks, ci, split, bcm);
    case 3: return new cholinv_impl<cholesky::cholinv<SP, IP, P::NoReplicationOverlap>>(n, c, layout, chunks, ci, split, bcm);
  }
  throw std::invalid_argument("base-case policy id must be 0..3 (policy.h get_id)");
}

struct cacqr_problem {
  virtual ~cacqr_problem() {}
  virtual void generate() = 0;
  virtual void set_A(const double* host) = 0;
  virtual void factor() = 0;
  virtual double residual() = 0;
  virtual double orthogonality() = 0;
  virtual void get(int which, double* host) = 0;
  virtual void dims(int64_t* mloc, int64_t* n) = 0;
  virtual void get_rows(int which, int64_t row0, int64_t nrows, double* host) = 0;
  virtual void set_shift(int num_shifted, double shift_scale) = 0;
  virtual void sweep_stats(int k, double* out3) = 0;
  virtual void lstsq(int64_t r, const double* B_host, double* X_host, double* resnorm_host) = 0;
  virtual void svd(bool want_left, double* U_host, double* s_host, double* V_host, int* sweeps) = 0;
  virtual void factor_pivoted(double rtol, double tol_scale, int* rank) = 0;
  virtual void get_piv(int64_t* piv_host) = 0;
};

template <class Alg>
struct cacqr_impl : cacqr_problem {
  using CI = cholesky::cholinv<cholesky::policy::cholinv::Serialize, cholesky::policy::cholinv::SaveIntermediates, cholesky::policy::cholinv::NoReplication>;
  topo::rect grid;
  MatrixType A;
  typename Alg::template info<T, U, CI> pack;
  cacqr_impl(int64_t m, int64_t n, int c, int variant, int layout, int chunks, int ci, int split, int bcm)
      : grid(capital::world(), (size_t)c, (size_t)layout, (size_t)chunks), A(n, m, grid.c, grid.d),
        pack((size_t)variant, typename CI::template info<T, U>(ci, split, bcm, 'U')) {}
  void generate() override { A.distribute_random(grid.x, grid.y, grid.c, grid.d, grid.rank / grid.c); }             // bench/qr/cacqr.cpp:34
  void set_A(const double* host) override { A.from_host(host); }
  void factor() override { Alg::factor(A, pack, grid); }
  void set_shift(int num_shifted, double shift_scale) override {
    if (num_shifted < 0 || (size_t)num_shifted > std::max<size_t>(1, pack.num_iter) || !(shift_scale >= 0.0) || !(shift_scale <= 1.79e308))
      throw std::invalid_argument("cacqr set_shift: 0 <= num_shifted <= the number of sweeps and a finite shift_scale >= 0 expected");
    pack.num_shifted = (size_t)num_shifted;
    pack.shift_scale = shift_scale;
  }
  // out3 = shift s, trace of the equilibrated Gram matrix, cond bound of sweep k of the last factor() (info::sweep_* in cacqr.h)
  void sweep_stats(int k, double* out3) override {
    if (k < 0 || (size_t)k >= pack.sweep_cond_bound.size()) throw std::invalid_argument("cacqr sweep_stats: no record of that sweep (records are kept by runs with shifted sweeps)");
    out3[0] = pack.sweep_shift[k]; out3[1] = pack.sweep_trace[k]; out3[2] = pack.sweep_cond_bound[k];
  }
  // min ||A X - B||_F on the factors of the last factor(): B_host is this rank's m_loc x r block (column-major, rows dealt as A's), X_host
  // receives the n x r solution, resnorm_host (may be NULL: no residual pass) the r norms ||b_j - A x_j||_2
  void lstsq(int64_t r, const double* B_host, double* X_host, double* resnorm_host) override {
    if (r < 1 || !B_host || !X_host) throw std::invalid_argument("cacqr lstsq: r >= 1 right-hand sides, B and X expected");
    MatrixType B(r, A.num_rows_global(), grid.c, grid.d);
    B.from_host(B_host);
    Alg::least_squares(A, B, pack, grid, resnorm_host != nullptr);
    fetch(pack.X, X_host);
    if (resnorm_host) std::memcpy(resnorm_host, pack.ls_residual_norms.data(), sizeof(double) * (size_t)r);
  }
  // A = U diag(s) V^T on the factors of the last factor(): s_host receives the n singular values (descending), V_host (may be NULL) the n x n V,
  // U_host, with want_left, this rank's m_loc x n block of U (column-major, rows dealt as A's); want_left == false touches no m x n memory
  void svd(bool want_left, double* U_host, double* s_host, double* V_host, int* sweeps) override {
    if (!s_host || (want_left && !U_host)) throw std::invalid_argument("cacqr svd: a place for the singular values, and for U with want_left, expected");
    Alg::svd(pack, grid, want_left);
    std::memcpy(s_host, pack.singular_values.data(), sizeof(double) * pack.singular_values.size());
    if (V_host) fetch(pack.V, V_host);
    if (want_left) fetch(pack.U, U_host);
    if (sweeps) *sweeps = pack.svd_sweeps;
  }
  // column-pivoted CholeskyQR (qr::cacqr::factor_pivoted): rtol = the user's tolerance relative to ||A||_F (0: the floor alone), tol_scale multiplies
  // the tolerance; *rank (may be NULL) receives the numerical rank, also when the call throws behind capi_dpstrf
  void factor_pivoted(double rtol, double tol_scale, int* rank) override {
    pack.pivot_rtol = rtol;
    pack.pivot_tol_scale = tol_scale;
    if (rank) *rank = 0;
    try {
      Alg::factor_pivoted(A, pack, grid);
    } catch (...) {
      if (rank) *rank = (int)pack.rank;
      throw;
    }
    if (rank) *rank = (int)pack.rank;
  }
  void get_piv(int64_t* piv_host) override {
    if (!piv_host || pack.piv.empty()) throw std::invalid_argument("cacqr get_piv: factor_pivoted has not run (or no place for the n indices)");
    for (size_t j = 0; j < pack.piv.size(); ++j) piv_host[j] = pack.piv[j];
  }
  // the validators and which = 2 / 3 of get() read factor()'s pair (a square R, n columns of Q): not what factor_pivoted leaves
  void plain_factors_only(const char* what) const {
    if (pack.pivoted) throw std::logic_error(std::string("cacqr ") + what + ": the resident factors are factor_pivoted's; use get which = 4 (Rp), 1 (Q) and get_piv");
  }
  double residual() override { plain_factors_only("residual"); return qr::validate<Alg>::residual(A, pack, grid); }
  double orthogonality() override { plain_factors_only("orthogonality"); return qr::validate<Alg>::orthogonality(A, pack, grid); }
  void get(int which, double* host) override {
    if (which == 0) { fetch(A, host); return; }
    if (which == 2 || which == 3) plain_factors_only("get");
    if (which == 1) { fetch(Alg::construct_Q(pack, grid), host); return; }
    if (which == 3) {                                     // Q^T Q (summed over the ranks), n x n
      matrix<double, int64_t, rect> I(A.num_columns_global(), A.num_columns_global(), 1, 1);
      qr::validate<Alg>::gram_of_Q(pack, grid, I);
      fetch(I, host);
      return;
    }
    if (which == 4) {                                     // Rp of factor_pivoted, n x n: rows < rank hold R, the rest is zero
      if (!pack.pivoted || !pack.Rp.filled()) throw std::invalid_argument("cacqr get: which = 4 (Rp) needs a successful factor_pivoted");
      fetch(pack.Rp, host);
      return;
    }
    fetch(Alg::construct_R(pack, grid), host);
  }
  void dims(int64_t* mloc, int64_t* n) override { *mloc = A.num_rows_local(); *n = A.num_columns_local(); }
  // local rows [row0, row0 + nrows) of A (which = 0) or Q (1), column-major nrows x n: a bounded window of a panel that is
  // too large to fetch whole (config 5: 64 GiB per GPU)
  void get_rows(int which, int64_t row0, int64_t nrows, double* host) override {
    const int64_t m = A.num_rows_local(), n = A.num_columns_local();
    if (row0 < 0 || nrows < 0 || row0 + nrows > m || (which != 0 && which != 1)) throw std::invalid_argument("cacqr get_rows: window outside the local panel");
    const double* src = (which == 0 ? A.data() : pack.Q.data()) + row0;
    double* tmp = capital::dev_alloc(nrows * n);
    CAPITAL_CHECK(capi_dlacpy(capital::handle(), 0, nrows, n, src, m, tmp, nrows));
    CAPITAL_CHECK(capi_memcpy_d2h(capital::handle(), host, tmp, sizeof(double) * (size_t)(nrows * n)));
    capital::dev_free(tmp);
  }
};

// ---- one SUMMA multiply on the current world (capital_summa_gemm / _trmm / _syrk below) ----------------------------------------------
using matmult::summa;
using matmult::view;

// the d x d x c grid of the multiplies: its four sub-communicators are kept between calls while c, layout and CAPITAL_MULTIPATH (read when
// a grid is built) stay what they were; num_chunks is set per call
struct summa_grid_cache {
  std::unique_ptr<topo::square> grid;
  int c = 0, layout = 0;
  std::string multipath;
};
CAPITAL_RANK_LOCAL summa_grid_cache g_summa_grid;

topo::square& summa_grid(int c, int layout, int num_chunks) {
  if (c < 1 || layout < 0 || num_chunks < 0) throw std::invalid_argument("summa: c >= 1, layout >= 0 and num_chunks >= 0 expected");
  if (!capital::world()) throw std::runtime_error("no world communicator: call capital_drv_init first");
  const char* mp = getenv("CAPITAL_MULTIPATH");
  summa_grid_cache& g = g_summa_grid;
  if (!g.grid || g.c != c || g.layout != layout || g.multipath != (mp ? mp : "")) {
    capital::sync();
    g.grid.reset();
    g.grid.reset(new topo::square(capital::world(), (size_t)c, (size_t)layout, 0));
    g.c = c; g.layout = layout; g.multipath = mp ? mp : "";
  }
  g.grid->num_chunks = (size_t)num_chunks;
  return *g.grid;
}
void summa_grid_where(const topo::square& t, int* xyzdc) {
  if (!xyzdc) return;
  xyzdc[0] = (int)t.x; xyzdc[1] = (int)t.y; xyzdc[2] = (int)t.z; xyzdc[3] = (int)t.d; xyzdc[4] = (int)t.c;
}

// a rows x cols block on the device with leading dimension rows + pad; the pad rows below every column hold `fill`
struct padded_block {
  double* p = nullptr;
  int64_t rows, cols, ld;
  padded_block(const double* host, int64_t rows_, int64_t cols_, int64_t pad, double fill) : rows(rows_), cols(cols_), ld(rows_ + pad) {
    std::vector<double> img((size_t)(ld * cols), fill);
    for (int64_t j = 0; j < cols; ++j) std::memcpy(&img[(size_t)(j * ld)], host + j * rows, sizeof(double) * (size_t)rows);
    p = capital::dev_alloc(ld * cols);
    CAPITAL_CHECK(capi_memcpy_h2d(capital::handle(), p, img.data(), sizeof(double) * img.size()));
  }
  padded_block(const padded_block&) = delete;
  padded_block& operator=(const padded_block&) = delete;
  ~padded_block() { capital::dev_free(p); }
  view v() const { return view{p, ld, rows, cols}; }
  // the block into block_host (rows x cols) and its pad rows into pad_host ((ld - rows) x cols), both column-major; either may be NULL
  void fetch(double* block_host, double* pad_host) const {
    std::vector<double> img((size_t)(ld * cols));
    CAPITAL_CHECK(capi_memcpy_d2h(capital::handle(), img.data(), p, sizeof(double) * img.size()));
    const int64_t pad = ld - rows;
    for (int64_t j = 0; j < cols; ++j) {
      if (block_host) std::memcpy(block_host + j * rows, &img[(size_t)(j * ld)], sizeof(double) * (size_t)rows);
      if (pad_host && pad > 0) std::memcpy(pad_host + j * pad, &img[(size_t)(j * ld + rows)], sizeof(double) * (size_t)pad);
    }
  }
};

// a matrix<> of the given LOCAL extents filled from the host (what the public summa::invoke overloads take)
MatrixType local_matrix(const double* host, int64_t rows, int64_t cols) {
  MatrixType m(nullptr, cols, rows, 1, 1);
  m.from_host(host);
  return m;
}

// the arena of a view-level call: the public overloads' rules over the padded extents, the relay space of a grid of pairs and, for syrk, the
// exchanged copy with its staging on top
matmult::arena& summa_view_arena(int64_t a, int64_t b, int64_t c) {
  matmult::arena& ws = summa::scratch_arena();
  ws.reserve(6 * (a + b + c) + 1024);
  return ws;
}

}  // namespace

extern "C" {

const char* capital_drv_last_error(void) { return g_err.c_str(); }

// stream != NULL: run on the caller's HIP stream (e.g. torch's current stream); uid: 128-byte RCCL id when size > 1
int capital_drv_init(int device, int rank, int size, const void* uid, void* stream) {
  return guarded([&] {
    if (stream) {
      capi_handle_t h;
      if (capi_create_on_stream(&h, device, stream) != CAPI_OK) throw std::runtime_error("capi_create_on_stream failed");
      capital::ctx().owns_handle = true;
      capital::ctx().device = device;
      capital::init_with_handle(h, rank, size, uid);
    } else {
      capital::init(device, rank, size, uid);
    }
  });
}
int capital_drv_finalize(void) {
  return guarded([] {
    if (g_summa_grid.grid) {                                     // (its sub-communicators go before the world they were split from)
      if (capital::ctx().handle) capital::sync();
      g_summa_grid.grid.reset();
    }
    capital::finalize();
  });
}
int capital_drv_sync(void) { return guarded([] { capital::sync(); }); }
void* capital_drv_handle(void) { return capital::ctx().handle; }
// rank and size of the world communicator as RCCL itself reports them (a launcher prints them next to its own)
int capital_drv_world_query(int* rank, int* size) {
  return guarded([&] {
    if (!capital::world()) throw std::runtime_error("no world communicator: call capital_drv_init first");
    CAPITAL_CHECK(capi_comm_query(capital::world(), rank, size));
  });
}

// serialize_: 0 NoSerialize, 1 Serialize; + 2: FlushIntermediates instead of SaveIntermediates (policy.h:21-156)
void* capital_cholinv_create(int64_t n, int c, int layout, int num_chunks, int complete_inv, int split, int bc_mult, int serialize_, int bc_policy) {
  cholinv_problem* p = nullptr;
  int rc = guarded([&] {
    namespace P = cholesky::policy::cholinv;
    const bool ser = (serialize_ & 1) != 0, flush = (serialize_ & 2) != 0;
    if (ser && flush) p = make_cholinv<P::Serialize, P::FlushIntermediates>(bc_policy, n, c, layout, num_chunks, complete_inv, split, bc_mult);
    else if (ser) p = make_cholinv<P::Serialize, P::SaveIntermediates>(bc_policy, n, c, layout, num_chunks, complete_inv, split, bc_mult);
    else if (flush) p = make_cholinv<P::NoSerialize, P::FlushIntermediates>(bc_policy, n, c, layout, num_chunks, complete_inv, split, bc_mult);
    else p = make_cholinv<P::NoSerialize, P::SaveIntermediates>(bc_policy, n, c, layout, num_chunks, complete_inv, split, bc_mult);
  });
  return rc ? nullptr : p;
}
int capital_cholinv_generate(void* p) { return guarded([&] { ((cholinv_problem*)p)->generate(); }); }
int capital_cholinv_set_A(void* p, const double* host) { return guarded([&] { ((cholinv_problem*)p)->set_A(host); }); }
int capital_cholinv_factor(void* p) { return guarded([&] { ((cholinv_problem*)p)->factor(); }); }
int capital_cholinv_residual(void* p, double* out) { return guarded([&] { *out = ((cholinv_problem*)p)->residual(); }); }
int capital_cholinv_get(void* p, int which, double* host) { return guarded([&] { ((cholinv_problem*)p)->get(which, host); }); }
int capital_cholinv_get_rows(void* p, int which, int64_t count, const int64_t* rows, double* host) {
  return guarded([&] { ((cholinv_problem*)p)->get_rows(which, count, rows, host); });
}
int capital_cholinv_dims(void* p, int64_t* nloc, int* x, int* y, int* z, int* d, int* c) { return guarded([&] { ((cholinv_problem*)p)->dims(nloc, x, y, z, d, c); }); }
int capital_cholinv_stats(void* p, int64_t* bc, int64_t* levels, int64_t* bcdim) { return guarded([&] { ((cholinv_problem*)p)->stats(bc, levels, bcdim); }); }
// TRSM mode (info::solve_with_trsm): potrf + block TRSM + SYRK recursion, no inverse formed (one GPU, or a d x d x c grid: potrf_rec_grid)
int capital_cholinv_set_trsm_mode(void* p, int on) { return guarded([&] { ((cholinv_problem*)p)->set_trsm_mode(on != 0); }); }
// info::solve_by_substitution: solve() by two thin triangular solves on R (capi_dtrsm_thin), in either mode; takes effect at the next solve()
int capital_cholinv_set_solve_substitution(void* p, int on) { return guarded([&] { ((cholinv_problem*)p)->set_solve_substitution(on != 0); }); }
// A X = B on the factors (cholesky::cholinv::solve): after capital_cholinv_factor, one rank; resnorm_host_or_null == NULL skips the residual pass.
// Refinement and residual read A's upper triangle alone, as the factorization does: A need not be stored symmetric
int capital_cholinv_solve(void* p, int64_t r, const double* B_host, double* X_host, double* resnorm_host_or_null, int refine) {
  return guarded([&] { ((cholinv_problem*)p)->solve(r, B_host, X_host, resnorm_host_or_null, refine); });
}
// How far to trust a solve (cholesky::cholinv::condition / error_bounds; one rank, after capital_cholinv_factor).
// rcond: the reciprocal 1-norm condition number as LAPACK's dpocon estimates it; anorm1_or_null receives ||A||_1
int capital_cholinv_rcond(void* p, double* rcond, double* anorm1_or_null) {
  return guarded([&] { ((cholinv_problem*)p)->rcond(rcond, anorm1_or_null, nullptr); });
}
// the same with the number of products with A^-1 that the estimate took (at most 11)
int capital_cholinv_rcond_applies(void* p, double* rcond, double* anorm1_or_null, int* applies_or_null) {
  return guarded([&] { ((cholinv_problem*)p)->rcond(rcond, anorm1_or_null, applies_or_null); });
}
// dporfs's bounds for the X that the last capital_cholinv_solve[_expert] left on the device: B_host must be that solve's right-hand sides (r must
// match the resident X).  ferr_host[j] bounds ||x_j - x_true,j||_inf / ||x_j||_inf, berr_host[j] is the componentwise backward error
int capital_cholinv_error_bounds(void* p, int64_t r, const double* B_host, double* ferr_host, double* berr_host) {
  return guarded([&] { ((cholinv_problem*)p)->error_bounds(r, B_host, ferr_host, berr_host, nullptr); });
}
// capital_cholinv_solve, then capital_cholinv_error_bounds on its X (LAPACK's dposvx without equilibration)
int capital_cholinv_solve_expert(void* p, int64_t r, const double* B_host, double* X_host, double* resnorm_host_or_null, int refine, double* ferr_host,
                                 double* berr_host) {
  return guarded([&] {
    if (!ferr_host || !berr_host) throw std::invalid_argument("cholinv solve_expert: ferr and berr expected");
    ((cholinv_problem*)p)->solve(r, B_host, X_host, resnorm_host_or_null, refine);
    ((cholinv_problem*)p)->error_bounds(r, B_host, ferr_host, berr_host, nullptr);
  });
}
// A <- A + sign V V^T (sign = +1 update, -1 downdate) WITHOUT a new factorisation (cholesky::cholinv::update; one rank, after capital_cholinv_factor):
// V_host n x r column-major, any r >= 1.  R, R^-1 where one exists, and A's upper triangle are updated on the device.  -1 with the failing step in
// capital_drv_last_error when a downdate leaves the matrix not positive definite: A is then unchanged and the factors are invalid until the next factor.
int capital_cholinv_update(void* p, int64_t r, const double* V_host, int sign) {
  return guarded([&] { ((cholinv_problem*)p)->update(r, V_host, sign); });
}
// A ~= L L^T, L n x rank, by a diagonally pivoted partial Cholesky (cholesky::cholinv::factor_pivoted; one rank): for a matrix that is only positive
// semidefinite or numerically low-rank, where capital_cholinv_factor fails.  rtol: stop where the largest remaining Schur diagonal entry is <= rtol trace(A)
// (0: LAPACK dpstrf's default); max_rank: 0 = min(n, CAPI_PCHOL_MAX_RANK).  The factors of capital_cholinv_factor, if any, are not touched.
int capital_cholinv_factor_pivoted(void* p, double rtol, int64_t max_rank, int64_t* rank, double* resid_trace, double* thresh) {
  return guarded([&] { ((cholinv_problem*)p)->factor_pivoted(rtol, max_rank, rank, resid_trace, thresh); });
}
int capital_cholinv_get_pivoted(void* p, double* L_host /* n x rank */, int* piv_host /* n */, double* d_host /* n */) {
  return guarded([&] { ((cholinv_problem*)p)->get_pivoted(L_host, piv_host, d_host); });
}
// The factors themselves (cholesky::cholinv::apply / quadratic_forms / log_determinant / inverse_diagonal; one rank, after capital_cholinv_factor, also
// after capital_cholinv_update).  capital_cholinv_apply: Y_host (n x r) <- op B_host, op = 0 R, 1 R^T, 2 R^-1, 3 R^-T (A = R^T R); the X of the last
// solve stays as it is
int capital_cholinv_apply(void* p, int op, int64_t r, const double* B_host, double* Y_host) {
  return guarded([&] { ((cholinv_problem*)p)->apply(op, r, B_host, Y_host); });
}
// q_host[j] <- b_j^T A^-1 b_j, r results
int capital_cholinv_quadratic_forms(void* p, int64_t r, const double* B_host, double* q_host) {
  return guarded([&] { ((cholinv_problem*)p)->quadratic_forms(r, B_host, q_host); });
}
// *v <- log det A
int capital_cholinv_logdet(void* p, double* v) { return guarded([&] { ((cholinv_problem*)p)->logdet(v); }); }
// d_host[i] <- (A^-1)_ii, n results; -1 in TRSM mode, which has no inverse
int capital_cholinv_inverse_diagonal(void* p, double* d_host) { return guarded([&] { ((cholinv_problem*)p)->inverse_diagonal(d_host); }); }
// Badly scaled matrices (cholesky::cholinv::equilibrate / unequilibrate; one rank): A <- D^-1 A D^-1 with D = diag(2^e_j) from A's diagonal, iff scond < thresh
// or amax lies outside [SMALL, LARGE] (dlaqsy's rule; thresh > 1 forces it).  *scaled: 1 when it scaled -- capital_cholinv_factor then factors the scaled
// matrix and every operation on the factors answers for the original one -- 0 when nothing changed.  dscale_host_or_null: n doubles.
int capital_cholinv_equilibrate(void* p, double thresh, int* scaled, double* scond, double* amax, double* dscale_host_or_null) {
  return guarded([&] { ((cholinv_problem*)p)->equilibrate(thresh, scaled, scond, amax, dscale_host_or_null); });
}
int capital_cholinv_unequilibrate(void* p) { return guarded([&] { ((cholinv_problem*)p)->unequilibrate(); }); }
// The regularised low-rank operator M = L L^T + D on the factor of capital_cholinv_factor_pivoted (cholesky::cholinv::lowrank_prepare / lowrank_solve /
// lowrank_quadratic_forms; one rank): d = shift + diag_host_or_null (n doubles) + (use_schur: the remaining Schur diagonal of that factorization), every
// d_i a finite number > 0.  prepare factors the k x k matrix C = I + L^T D^-1 L; *logdet (may be NULL) <- log det M, *cnorm1 (may be NULL) <- ||C||_1:
// the results below carry errors of ||C||_1 2^-53.  The factors of capital_cholinv_factor and A are not touched.
int capital_cholinv_lowrank_prepare(void* p, double shift, const double* diag_host_or_null, int use_schur, double* logdet, double* cnorm1) {
  return guarded([&] { ((cholinv_problem*)p)->lowrank_prepare(shift, diag_host_or_null, use_schur, logdet, cnorm1); });
}
// X_host (n x r) <- M^-1 B_host; resnorm_host_or_null: the r norms ||b_j - M x_j||_2, from L and d alone
int capital_cholinv_lowrank_solve(void* p, int64_t r, const double* B_host, double* X_host, double* resnorm_host_or_null) {
  return guarded([&] { ((cholinv_problem*)p)->lowrank_solve(r, B_host, X_host, resnorm_host_or_null); });
}
// q_host[j] <- b_j^T M^-1 b_j, r results
int capital_cholinv_lowrank_quadratic_forms(void* p, int64_t r, const double* B_host, double* q_host) {
  return guarded([&] { ((cholinv_problem*)p)->lowrank_quadratic_forms(r, B_host, q_host); });
}
int capital_cholinv_destroy(void* p) { return guarded([&] { capital::sync(); delete (cholinv_problem*)p; }); }

void* capital_cacqr_create(int64_t m, int64_t n, int c, int variant, int layout, int num_chunks, int complete_inv, int split, int bc_mult, int serialize_) {
  cacqr_problem* p = nullptr;
  int rc = guarded([&] {
    namespace P = qr::policy::cacqr;
    if (serialize_) p = new cacqr_impl<qr::cacqr<P::Serialize, P::SaveIntermediates>>(m, n, c, variant, layout, num_chunks, complete_inv, split, bc_mult);
    else p = new cacqr_impl<qr::cacqr<P::NoSerialize, P::SaveIntermediates>>(m, n, c, variant, layout, num_chunks, complete_inv, split, bc_mult);
  });
  return rc ? nullptr : p;
}
int capital_cacqr_generate(void* p) { return guarded([&] { ((cacqr_problem*)p)->generate(); }); }
int capital_cacqr_set_A(void* p, const double* host) { return guarded([&] { ((cacqr_problem*)p)->set_A(host); }); }
// shifted CholeskyQR (cacqr.h): the first num_shifted of the `variant` sweeps are shifted sweeps; call before factor
int capital_cacqr_set_shift(void* p, int num_shifted, double shift_scale) { return guarded([&] { ((cacqr_problem*)p)->set_shift(num_shifted, shift_scale); }); }
int capital_cacqr_sweep_stats(void* p, int k, double* out3) { return guarded([&] { ((cacqr_problem*)p)->sweep_stats(k, out3); }); }
// least squares on the factors (qr::cacqr::least_squares): after capital_cacqr_factor; resnorm_host_or_null == NULL skips the residual pass
int capital_cacqr_lstsq(void* p, int64_t r, const double* B_host_local, double* X_host, double* resnorm_host_or_null) {
  return guarded([&] { ((cacqr_problem*)p)->lstsq(r, B_host_local, X_host, resnorm_host_or_null); });
}
// singular values and vectors on the factors (qr::cacqr::svd): after capital_cacqr_factor, c == 1.  A = U diag(s) V^T; s_host: n doubles; V_host_or_null:
// n x n; U_host_local_or_null: this rank's m_loc x n rows of U, written with want_left != 0; sweeps (may be NULL): the Jacobi sweeps on R
int capital_cacqr_svd(void* p, int want_left, double* U_host_local_or_null, double* s_host, double* V_host_or_null, int* sweeps) {
  return guarded([&] { ((cacqr_problem*)p)->svd(want_left != 0, U_host_local_or_null, s_host, V_host_or_null, sweeps); });
}
// column-pivoted CholeskyQR for panels that may be rank deficient (qr::cacqr::factor_pivoted, c == 1): *rank (may be NULL) receives the numerical rank;
// afterwards capital_cacqr_get_piv gives the n column indices (column j of A P is column piv[j] of A), capital_cacqr_get which = 4 the n x n Rp
// and which = 1 Q (its first rank columns), and capital_cacqr_lstsq the basic least-squares solution
int capital_cacqr_factor_pivoted(void* p, double rtol, double tol_scale, int* rank) {
  return guarded([&] { ((cacqr_problem*)p)->factor_pivoted(rtol, tol_scale, rank); });
}
int capital_cacqr_get_piv(void* p, int64_t* piv_host) { return guarded([&] { ((cacqr_problem*)p)->get_piv(piv_host); }); }
int capital_cacqr_factor(void* p) { return guarded([&] { ((cacqr_problem*)p)->factor(); }); }
int capital_cacqr_residual(void* p, double* out) { return guarded([&] { *out = ((cacqr_problem*)p)->residual(); }); }
int capital_cacqr_orthogonality(void* p, double* out) { return guarded([&] { *out = ((cacqr_problem*)p)->orthogonality(); }); }
int capital_cacqr_get(void* p, int which, double* host) { return guarded([&] { ((cacqr_problem*)p)->get(which, host); }); }
int capital_cacqr_get_rows(void* p, int which, int64_t row0, int64_t nrows, double* host) { return guarded([&] { ((cacqr_problem*)p)->get_rows(which, row0, nrows, host); }); }
int capital_cacqr_dims(void* p, int64_t* mloc, int64_t* n) { return guarded([&] { ((cacqr_problem*)p)->dims(mloc, n); }); }
int capital_cacqr_destroy(void* p) { return guarded([&] { capital::sync(); delete (cacqr_problem*)p; }); }

// One matmult::summa multiply on the d x d x c grid over the current world (every rank calls, with the same arguments but its own blocks):
// what cholinv and cacqr issue many of, alone -- any form, any alpha and beta.  All extents are LOCAL, all host blocks column-major without
// padding; the flags are the C-ABI's (CAPI_TRANS, CAPI_LEFT, CAPI_UPPER, CAPI_UNIT ...).  INTEGRATION.md, "SUMMA on a grid", says which block of
// the global operands a rank passes.  pad == 0: through the public summa::invoke overloads on matrix<> objects (their arena sizing, the in-place
// TRMM, the SYRK that exchanges with the transpose partner itself).  pad > 0: through the view-level gemm / trmm / syrk on device blocks of
// leading dimension rows + pad whose pad rows hold `fill`; pad_host (pad x columns, may be NULL) then receives the pad rows of the block named
// below as they are after the call.  xyzdc (may be NULL) receives this rank's x, y, z and the grid's d, c.
// C_host (M x N): in C0, out alpha op(A) op(B) + beta C0; A_host is M x K (transA: K x M), B_host K x N (transB: N x K); pad_host: C's pad rows
int capital_summa_gemm(int c, int layout, int num_chunks, int transA, int transB, int64_t M, int64_t N, int64_t K, double alpha, double beta,
                       const double* A_host, const double* B_host, double* C_host, int64_t pad, double fill, double* pad_host, int* xyzdc) {
  return guarded([&] {
    if (M < 1 || N < 1 || K < 1 || pad < 0 || !A_host || !B_host || !C_host) throw std::invalid_argument("summa gemm: positive extents, pad >= 0 and the three blocks expected");
    topo::square& t = summa_grid(c, layout, num_chunks);
    summa_grid_where(t, xyzdc);
    const int64_t ar = transA ? K : M, ac = transA ? M : K, br = transB ? N : K, bc = transB ? K : N;
    if (pad == 0) {
      MatrixType A = local_matrix(A_host, ar, ac), B = local_matrix(B_host, br, bc), C = local_matrix(C_host, M, N);
      blas::ArgPack_gemm<T> pack(blas::Order::AblasColumnMajor, transA ? blas::Transpose::AblasTrans : blas::Transpose::AblasNoTrans,
                                 transB ? blas::Transpose::AblasTrans : blas::Transpose::AblasNoTrans, alpha, beta);
      summa::invoke(A, B, C, t, pack);
      capital::sync();
      fetch(C, C_host);
      return;
    }
    padded_block A(A_host, ar, ac, pad, fill), B(B_host, br, bc, pad, fill), C(C_host, M, N, pad, fill);
    matmult::arena& ws = summa_view_arena(A.ld * ac, B.ld * bc, C.ld * N);
    summa::gemm(t, transA ? CAPI_TRANS : CAPI_NOTRANS, transB ? CAPI_TRANS : CAPI_NOTRANS, alpha, A.v(), B.v(), beta, C.v(), ws);
    capital::sync();
    C.fetch(C_host, pad_host);
  });
}
// C_host (M x N): in what the output block holds before the call (view mode: the output is a block of its own, contiguous as summa.h asks; the
// public overload multiplies in place), out alpha op(T) B (side Left, T of order M) or alpha B op(T) (Right, order N); pad_host: B's pad rows
int capital_summa_trmm(int c, int layout, int num_chunks, int side, int uplo, int trans, int diag, int64_t M, int64_t N, double alpha,
                       const double* T_host, const double* B_host, double* C_host, int64_t pad, double fill, double* pad_host, int* xyzdc) {
  return guarded([&] {
    if (M < 1 || N < 1 || pad < 0 || !T_host || !B_host || !C_host) throw std::invalid_argument("summa trmm: positive extents, pad >= 0 and the three blocks expected");
    topo::square& t = summa_grid(c, layout, num_chunks);
    summa_grid_where(t, xyzdc);
    const int64_t nt = side == CAPI_LEFT ? M : N;
    if (pad == 0) {
      MatrixType A = local_matrix(T_host, nt, nt), B = local_matrix(B_host, M, N);
      blas::ArgPack_trmm<T> pack(blas::Order::AblasColumnMajor, side == CAPI_LEFT ? blas::Side::AblasLeft : blas::Side::AblasRight,
                                 uplo == CAPI_UPPER ? blas::UpLo::AblasUpper : blas::UpLo::AblasLower,
                                 trans ? blas::Transpose::AblasTrans : blas::Transpose::AblasNoTrans,
                                 diag == CAPI_UNIT ? blas::Diag::AblasUnit : blas::Diag::AblasNonUnit, alpha);
      summa::invoke(A, B, t, pack);
      capital::sync();
      fetch(B, C_host);
      return;
    }
    padded_block Tb(T_host, nt, nt, pad, fill), B(B_host, M, N, pad, fill), Cout(C_host, M, N, 0, fill);
    matmult::arena& ws = summa_view_arena(Tb.ld * nt, B.ld * N, M * N);
    summa::trmm(t, side, uplo, trans ? CAPI_TRANS : CAPI_NOTRANS, diag, alpha, Tb.v(), B.v(), Cout.v(), ws);
    capital::sync();
    Cout.fetch(C_host, nullptr);
    B.fetch(nullptr, pad_host);
  });
}
// C_host (N x N): in C0, out -- in its `uplo` triangle alone -- alpha A^T A + beta C0 (trans; A_host K x N) or alpha A A^T + beta C0 (A_host N x K);
// the second operand is this rank's A exchanged with the transpose partner, as cholinv.h prepares it (view mode) or as the public overload does;
// pad_host: C's pad rows
int capital_summa_syrk(int c, int layout, int num_chunks, int uplo, int trans, int64_t N, int64_t K, double alpha, double beta,
                       const double* A_host, double* C_host, int64_t pad, double fill, double* pad_host, int* xyzdc) {
  return guarded([&] {
    if (N < 1 || K < 1 || pad < 0 || !A_host || !C_host) throw std::invalid_argument("summa syrk: positive extents, pad >= 0 and the two blocks expected");
    topo::square& t = summa_grid(c, layout, num_chunks);
    summa_grid_where(t, xyzdc);
    const int64_t ar = trans ? K : N, ac = trans ? N : K;
    if (pad == 0) {
      MatrixType A = local_matrix(A_host, ar, ac), C = local_matrix(C_host, N, N);
      blas::ArgPack_syrk<T> pack(blas::Order::AblasColumnMajor, uplo == CAPI_UPPER ? blas::UpLo::AblasUpper : blas::UpLo::AblasLower,
                                 trans ? blas::Transpose::AblasTrans : blas::Transpose::AblasNoTrans, alpha, beta);
      summa::invoke(A, C, t, pack);
      capital::sync();
      fetch(C, C_host);
      return;
    }
    padded_block A(A_host, ar, ac, pad, fill), C(C_host, N, N, pad, fill);
    matmult::arena& ws = summa_view_arena(A.ld * ac, 0, C.ld * N);
    view Ax{ws.take(ar * ac), ar, ar, ac};
    CAPITAL_CHECK(capi_dlacpy(capital::handle(), 0, ar, ac, A.p, A.ld, Ax.p, Ax.ld));
    util::transpose_raw(Ax.p, Ax.count(), ws.take(Ax.count()), t, summa::relay_space(t, Ax.count(), ws));
    summa::syrk(t, uplo, trans ? CAPI_TRANS : CAPI_NOTRANS, alpha, A.v(), Ax, beta, C.v(), ws);
    capital::sync();
    C.fetch(C_host, pad_host);
  });
}

}  // extern "C"
