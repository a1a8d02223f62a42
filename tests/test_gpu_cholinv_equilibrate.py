"""cholesky::cholinv::equilibrate through driver.Cholinv on one GPU: a covariance in mixed units, A = D0 C D0 (upper triangle mirrored) with
C = f1_spectrum(n, kappa, seed=3) and D0 = 10^uniform(-8, 8) from default_rng(n) -- 16 decades of grading -- is scaled to A_s = D^-1 A D^-1 with
D = diag(2^e) (tests/_equil_ref.py), factored, and every operation on the factors must answer for the ORIGINAL A.  u = 2^-53.

Right-hand sides: B = ldexp(A_s X0, e) = D (A_s X0) with the integer X0 of tests/test_gpu_cholinv_bounds.py (default_rng(n).integers(-8, 9), zeros set
to 1; 40 columns, the first 5 for everything that needs a longdouble reference), so that the scaled problem is A_s X_s = B_s = A_s X0 and X = D^-1 X_s.

What is asserted, and where each bound comes from:
 1. equilibrate() scales (order 1: forced by thresh > 1); scond, amax, scale() and the upper triangle of A() equal the restatement bit for bit;
    unequilibrate() restores A bit for bit.
 2. an ungraded f1_spectrum is left alone by the default thresh, with its factors still valid.
 3. rcond() is that of A_s: 0.9 <= rcond / rcond_true(A_s) <= 3 and within a factor 2 of scipy's dpocon on A_s -- the rules of
    tests/test_gpu_cholinv_bounds.py (on the CPU dpocon gives 1.13 .. 1.36 rcond_true on these inputs).
 4. equivariance, bit for bit: X == ldexp(X', -e) with X' from a second handle that was given A_s and B_s, and X == X'' from a plain handle on (A, B):
    Cholesky, the triangular inverse, the thin products and the residual are homogeneous under power-of-two gradings.  The same for every other
    operation (apply, quadratic_forms, logdet, inverse_diagonal, solve_expert's bounds, update): the equilibrated handle against the handle on A_s, mapped by D.
 5. solve_expert: berr <= 10 max(berr_ref, u) and ||D (x - x_true)||_inf / ||D x||_inf <= ferr <= 10 ferr_ref with scipy's dposvx(fact='N') on
    (A_s, B_s) and x_true from six longdouble refinement steps (the bounds test's rule); the residual norms equal ||B - A X||_2 in longdouble on the
    original A to 1e-10 relative plus n u ||A||_2 ||x||_2.
 6. the operations against scipy's Cholesky factor Rn of A_s, in longdouble, mapped by D, under the rules of tests/test_gpu_cholinv_apply.py:
    R and R^T are products of n terms, componentwise within 1.01 (n + 1) u |R_s| |.| on the device's own factor; R^-1 and R^-T where the complete
    inverse runs likewise on the fetched R_s^-1, and in the solving forms eta <= 10 max(eta_ref, u) on the normwise backward error, eta_ref from the
    form's numpy restatement on Rn; quadratic_forms within (n + 1) u of the longdouble column norms of its own half-solve, and within
    fwd = 4 (n + 1) u / rcond_true(A_s) of b_s^T x_true_s (to first order: the factor's backward error gamma_(n + 1), the half-solve's gamma_n counted twice
    in the square, n more roundings in the norm, all times kappa); logdet against slogdet(A_s) + 2 ln 2 sum e within 10 n u S,
    S = 2 sum |log r_ii| (the apply test's rule) plus 4 u of the added term; inverse_diagonal, scaled back by 2^(2 e_i), within 2 fwd of
    diag(cho_solve(I)) on A_s (each of the two is within fwd of the exact entry by the same count); update(V), V = D (0.25 N(0, 1)), then solve:
    the normwise backward error on A0 + V V^T (formed in the scaled variables, in longdouble) <= 10 max(that of scipy's cho_solve, u).
 7. state: a second equilibrate(), factor_pivoted while equilibrated, solve before the new factor() raise; set_A clears the flag; a zero on the
    diagonal raises and leaves A as it was.
 8. workspace: solve, solve_expert, apply and quadratic_forms give the same bytes after calls on all-NaN blocks, which leave NaN in every work block
    that an equilibrated solve and apply take from the operations' arena (tests/test_gpu_ops_workspace.py's method)."""
import numpy as np
import pytest
import scipy.linalg as sla
from scipy.linalg import lapack

import _apply_ref as aref
import _conditioning as cond
import _equil_ref as ref

pytestmark = pytest.mark.gpu
U64 = 2.0 ** -53
LD = np.longdouble
OPS = ("R", "RT", "Rinv", "RinvT")


@pytest.fixture(scope="module")
def drv():
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    yield driver
    driver.finalize()


_REF = {}


def reference(n, kappa):
    """the graded problem and everything of the host that the checks share, once per (n, kappa), read-only"""
    if (n, kappa) not in _REF:
        A, C, D0 = ref.graded(n, kappa)
        e = ref.exponents(np.diag(A))
        As = ref.sym_scale(A, e, 1)
        assert np.array_equal(As, As.T)
        X0 = np.random.default_rng(n).integers(-8, 9, (n, 40)).astype(np.float64)
        X0[X0 == 0] = 1.0
        Bs = np.asfortranarray(As @ X0)
        B = np.asfortranarray(ref.row_scale(Bs, e, 1))
        anorm = np.linalg.norm(As, 1)
        rcond_true = 1.0 / (anorm * np.linalg.norm(np.linalg.inv(As), 1))
        c, info = lapack.dpotrf(As, lower=0)
        rcond_lapack, info2 = lapack.dpocon(c, anorm, uplo="U")
        assert info == 0 and info2 == 0 and lapack.dpotrf(A, lower=0)[1] == 0
        # x_true of the scaled problem (six longdouble refinement steps on cho_solve) and dposvx's bounds, first five columns
        r = 5
        cf = sla.cho_factor(As)
        Al, Bl = As.astype(LD), Bs[:, :r].astype(LD)
        xt = sla.cho_solve(cf, Bs[:, :r]).astype(LD)
        for _ in range(6):
            xt = xt + sla.cho_solve(cf, (Bl - Al @ xt).astype(np.float64))
        out = lapack.dposvx(As, np.asfortranarray(Bs[:, :r]), fact="N", lower=0)
        assert out[9] == 0
        Rn = aref.chol_upper(As)
        rf = {"A": A, "As": As, "e": e, "B": B, "Bs": Bs, "rcond_true": rcond_true, "rcond_lapack": rcond_lapack, "xt_s": xt, "ferr_ref": out[7],
              "berr_ref": out[8], "normA2": np.linalg.norm(A, 2) if n > 1 else abs(A[0, 0]), "cf": cf, "Rn": Rn, "normR2": np.linalg.norm(Rn, 2), "eta": {}}
        for v in rf.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[(n, kappa)] = rf
    return _REF[(n, kappa)]


def eta_ref(rf, form, h1, trans):
    key = (form, h1, trans)
    if key not in rf["eta"]:
        Y = aref.half(rf["Rn"], rf["Bs"][:, :5], trans, form, h1=h1)
        rf["eta"][key] = aref.eta_half(rf["Rn"], rf["normR2"], rf["Bs"][:, :5], Y, trans)
    return rf["eta"][key]


POLICIES = [
    ("complete-inverse", 1000, dict(complete_inv=1, bc_mult=-2), 1e2, "complete"),
    ("complete-inverse", 1000, dict(complete_inv=1, bc_mult=-2), 1e6, "complete"),
    ("blocks-R12-packed", 2048, dict(complete_inv=0, split=1, bc_mult=-2), 1e6, "block"),
    ("trsm", 1000, dict(bc_mult=-2, trsm_mode=True), 1e2, "trsm"),
    ("substitution", 1000, dict(bc_mult=-2, substitution=True), 1e2, "subst"),
    ("no-split", 512, dict(complete_inv=0), 1e2, "complete"),
    ("order-one", 1, dict(), 1e2, "complete"),
]
IDS = [f"{c[0]}-kappa{c[3]:.0e}" for c in POLICIES]


def equilibrated(drv, rf, kw, factor=True):
    """a handle on the graded A, equilibrated (order 1 has nothing to grade: forced) and factored"""
    n = rf["A"].shape[0]
    p = drv.Cholinv(n, **kw)
    p.set_A(rf["A"])
    scaled, scond, amax = p.equilibrate(0.1 if n > 1 else 2.0)
    assert scaled
    if factor:
        p.factor()
    return p, scond, amax


def check_product(what, T, B, Y):
    n = T.shape[0]
    want = T.astype(LD) @ B.astype(LD)
    bound = 1.01 * (n + 1) * U64 * (np.abs(T) @ np.abs(B))
    err = np.abs(Y.astype(LD) - want)
    print(f"  {what}: max err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(err <= bound), what


@pytest.mark.parametrize("name,n,kw,kappa,form", POLICIES, ids=IDS)
def test_equilibrate_scales_exactly_and_back(drv, name, n, kw, kappa, form):
    rf = reference(n, kappa)
    A, e = rf["A"], rf["e"]
    p, scond, amax = equilibrated(drv, rf, kw, factor=False)
    try:
        want_ds, want_rec = ref.poequ2(np.diag(A))
        assert scond == want_rec[0] and amax == want_rec[1]
        assert p.scale().tobytes() == want_ds.tobytes()
        got = p.A()
        assert np.triu(got).tobytes() == np.triu(rf["As"]).tobytes()
        assert np.tril(got, -1).tobytes() == np.tril(A, -1).tobytes()              # below the diagonal nothing changes
        p.unequilibrate()
        assert p.A().tobytes() == A.tobytes()
        assert np.all(p.scale() == 1.0)
        with pytest.raises(drv.DriverError, match="not equilibrated"):
            p.unequilibrate()
    finally:
        p.close()


def test_a_well_scaled_matrix_is_left_alone(drv):
    n = 1000
    C = cond.f1_spectrum(n, 1e2, seed=3)
    B = np.asfortranarray(C @ np.ones((n, 2)))
    p = drv.Cholinv(n, complete_inv=1, bc_mult=-2)
    try:
        p.set_A(C)
        p.factor()
        X0, res0 = p.solve(B)
        scaled, scond, amax = p.equilibrate()
        want = ref.poequ2(np.diag(C))[1]
        assert not scaled and scond == want[0] and amax == want[1] and scond >= 0.1
        assert p.A().tobytes() == C.tobytes() and np.all(p.scale() == 1.0)
        X1, res1 = p.solve(B)                                                      # the factors are still valid
        assert X1.tobytes() == X0.tobytes() and res1.tobytes() == res0.tobytes()
        assert p.equilibrate(0.1)[0] is False                                      # not equilibrated: asking again is no misuse
    finally:
        p.close()


@pytest.mark.parametrize("name,n,kw,kappa,form", POLICIES, ids=IDS)
def test_solve_rcond_and_bounds_answer_for_the_original_matrix(drv, name, n, kw, kappa, form):
    rf = reference(n, kappa)
    A, As, e, B, Bs = rf["A"], rf["As"], rf["e"], rf["B"], rf["Bs"]
    r = 5
    p, _, _ = equilibrated(drv, rf, kw)
    q = drv.Cholinv(n, **kw)                                                       # the scaled problem on a handle of its own
    w = drv.Cholinv(n, **kw)                                                       # the original problem without equilibration
    try:
        q.set_A(As)
        q.factor()
        w.set_A(A)
        w.factor()
        assert (p.stats()["levels"] >= 1) == (n > 512)
        # 3. rcond is that of A_s
        rc = p.rcond()
        print(f"equilibrate {name} n={n} kappa={kappa:.0e}: rcond {rc:.4e} = {rc / rf['rcond_true']:.3f} rcond_true(A_s) = {rc / rf['rcond_lapack']:.3f} dpocon's; "
              f"plain handle on A: {w.rcond():.3e}")
        assert 0.9 <= rc / rf["rcond_true"] <= 3
        assert 0.5 <= rc / rf["rcond_lapack"] <= 2
        assert rc == q.rcond()
        # 4. equivariance, bit for bit, 5 and 40 columns
        for cols in (5, 40):
            X, res = p.solve(B[:, :cols])
            Xq, resq = q.solve(Bs[:, :cols])
            Xw, resw = w.solve(B[:, :cols])
            assert X.tobytes() == ref.row_scale(Xq, e, -1).tobytes(), cols
            assert X.tobytes() == Xw.tobytes(), cols
        # 5. solve_expert
        X, res, ferr, berr = p.solve_expert(B[:, :r], refine=1)
        Xq, resq, ferrq, berrq = q.solve_expert(Bs[:, :r], refine=1)
        assert X.tobytes() == ref.row_scale(Xq, e, -1).tobytes() and ferr.tobytes() == ferrq.tobytes() and berr.tobytes() == berrq.tobytes()
        Xs = ref.row_scale(X, e, 1)                                                # D x
        err = (np.abs(Xs.astype(LD) - rf["xt_s"]).max(axis=0) / np.abs(Xs).max(axis=0)).astype(np.float64)
        print(f"equilibrate {name}: berr {berr.max():.2e} (dposvx {rf['berr_ref'].max():.2e}), ferr {ferr.min():.2e} .. {ferr.max():.2e} "
              f"(dposvx {rf['ferr_ref'].min():.2e} .. {rf['ferr_ref'].max():.2e}), scaled true error {err.max():.2e}")
        assert np.all(berr <= 10 * np.maximum(rf["berr_ref"], U64)), (berr, rf["berr_ref"])
        assert np.all(err <= ferr) and np.all(ferr <= 10 * rf["ferr_ref"]), (err, ferr, rf["ferr_ref"])
        Xl = X.astype(LD)
        true_res = np.sqrt(((B[:, :r].astype(LD) - A.astype(LD) @ Xl) ** 2).sum(axis=0)).astype(np.float64)
        tol = 1e-10 * true_res + n * U64 * rf["normA2"] * np.sqrt((X * X).sum(axis=0))
        print(f"equilibrate {name}: residual norms {res}, longdouble {true_res}")
        assert np.all(np.isfinite(res)) and np.all(np.abs(res - true_res) <= tol), (res, true_res, tol)
    finally:
        for h in (p, q, w):
            h.close()


@pytest.mark.parametrize("name,n,kw,kappa,form", POLICIES, ids=IDS)
def test_operations_on_the_factors_answer_for_the_original_matrix(drv, name, n, kw, kappa, form):
    rf = reference(n, kappa)
    As, e, Rn = rf["As"], rf["e"], rf["Rn"]
    r = 5
    B, Bs = np.asfortranarray(rf["B"][:, :r]), np.asfortranarray(rf["Bs"][:, :r])
    fwd = 4 * (n + 1) * U64 / rf["rcond_true"]                                    # the first-order forward bound of the module's docstring
    p, _, _ = equilibrated(drv, rf, kw)
    q = drv.Cholinv(n, **kw)
    try:
        q.set_A(As)
        q.factor()
        Rg = np.triu(p.R())                                                        # what lies on the device: R_s
        assert Rg.tobytes() == np.triu(q.R()).tobytes()
        h1 = n >> 1 if form == "block" else None
        # apply: the four operators of A0 = R0^T R0, R0 = R_s D
        # (R^-1 takes B_s and R^-T takes B = D B_s, so that in the scaled variables both solve with the right-hand side B_s, as eta_ref does)
        Y = {op: p.apply(Bs if op == "Rinv" else B, op) for op in OPS}
        assert Y["R"].tobytes() == q.apply(ref.row_scale(B, e, 1), "R").tobytes()
        assert Y["RT"].tobytes() == ref.row_scale(q.apply(B, "RT"), e, 1).tobytes()
        assert Y["Rinv"].tobytes() == ref.row_scale(q.apply(Bs, "Rinv"), e, -1).tobytes()
        assert Y["RinvT"].tobytes() == q.apply(Bs, "RinvT").tobytes()
        check_product("R0 B = R_s (D B)", Rg, ref.row_scale(B, e, 1), Y["R"])
        check_product("R0^T B = D (R_s^T B)", Rg.T, B, ref.row_scale(Y["RT"], e, -1))
        ys = {"Rinv": (ref.row_scale(Y["Rinv"], e, 1), Bs, 0), "RinvT": (Y["RinvT"], Bs, 1)}       # (result, right-hand side, transposed) in the scaled variables
        if form == "complete":
            Ri = np.triu(p.Rinv())
            check_product("R0^-1 B = D^-1 (R_s^-1 B)", Ri, ys["Rinv"][1], ys["Rinv"][0])
            check_product("R0^-T B = R_s^-T (D^-1 B)", Ri.T, ys["RinvT"][1], ys["RinvT"][0])
        else:
            for op, (y, b, trans) in ys.items():
                eg, er = aref.eta_half(Rg, rf["normR2"], b, y, trans), eta_ref(rf, form, h1, trans)
                print(f"  {op} ({form}): eta {eg:.2e}, numpy restatement {er:.2e}")
                assert eg <= 10 * max(er, U64), (op, eg, er)
        # apply(Rinv, apply(RinvT, .)) is the unrefined solve of the original system
        assert p.apply(p.apply(B, "RinvT"), "Rinv").tobytes() == p.solve(B, refine=0, residual=False)[0].tobytes()
        # quadratic forms b^T A0^-1 b = b_s^T A_s^-1 b_s
        qf = p.quadratic_forms(B)
        assert qf.tobytes() == q.quadratic_forms(Bs).tobytes()
        qy = (Y["RinvT"].astype(LD) ** 2).sum(axis=0)
        qt = (Bs.astype(LD) * rf["xt_s"]).sum(axis=0)
        e1, e2 = float((np.abs(qf - qy) / qy).max()), float((np.abs(qf - qt) / qt).max())
        print(f"  quadratic_forms: against its own half-solve {e1:.2e} (bound {(n + 1) * U64:.2e}), against b_s^T x_true_s {e2:.2e} (bound {fwd:.2e})")
        assert e1 <= (n + 1) * U64 and e2 <= fwd
        # log det A0 = log det A_s + 2 ln 2 sum e
        ld = p.logdet()
        added = 2.0 * np.log(LD(2)) * int(e.sum())
        want = LD(np.linalg.slogdet(As)[1]) + added
        S = 2.0 * float(np.abs(np.log(np.diag(Rn))).sum())
        print(f"  logdet {ld:.6f}: |gpu - (slogdet(A_s) + 2 ln 2 sum e)| = {float(abs(LD(ld) - want)):.2e}, bound {10 * n * U64 * S + 4 * U64 * float(abs(added)):.2e}")
        assert abs(LD(ld) - want) <= 10 * n * U64 * S + 4 * U64 * float(abs(added))
        assert abs(LD(ld) - (LD(q.logdet()) + added)) <= 4 * U64 * float(abs(added)) + 2 * U64 * abs(ld)
        # diag(A0^-1)_i = 2^(-2 e_i) diag(A_s^-1)_i
        if form == "trsm":
            with pytest.raises(drv.DriverError, match="TRSM mode forms no inverse"):
                p.inverse_diagonal()
        else:
            d = p.inverse_diagonal()
            assert d.tobytes() == np.ldexp(q.inverse_diagonal(), (-2 * e).astype(np.int32)).tobytes()
            dref = np.diag(sla.cho_solve(rf["cf"], np.eye(n)))
            err = float((np.abs(np.ldexp(d, (2 * e).astype(np.int32)) - dref) / dref).max())
            print(f"  inverse_diagonal: scaled back, against diag(cho_solve(I)) on A_s {err:.2e} (bound {2 * fwd:.2e})")
            assert err <= 2 * fwd
        # update(V) then solve, against cho_solve on A0 + V V^T, in the scaled variables: A_s + V_s V_s^T, V_s = D^-1 V
        Vs = 0.25 * np.random.default_rng(n + 2).standard_normal((n, 3))
        V = np.asfortranarray(ref.row_scale(Vs, e, 1))
        p.update(V)
        q.update(np.asfortranarray(Vs))
        assert np.triu(p.A()).tobytes() == np.triu(q.A()).tobytes() and np.triu(p.R()).tobytes() == np.triu(q.R()).tobytes()
        X1 = p.solve(B)[0]
        assert X1.tobytes() == ref.row_scale(q.solve(Bs)[0], e, -1).tobytes()
        A1 = As.astype(LD) + Vs.astype(LD) @ Vs.astype(LD).T
        normA1 = np.linalg.norm(A1.astype(np.float64), 2) if n > 1 else abs(float(A1[0, 0]))

        def eta(Xs_):
            Xl = Xs_.astype(LD)
            rho = Bs.astype(LD) - A1 @ Xl
            return float((np.sqrt((rho * rho).sum(axis=0)) / (normA1 * np.sqrt((Xl * Xl).sum(axis=0)) + np.sqrt((Bs.astype(LD) ** 2).sum(axis=0)))).max())

        eg, er = eta(ref.row_scale(X1, e, 1)), eta(sla.cho_solve(sla.cho_factor(A1.astype(np.float64)), Bs))
        print(f"  update then solve: eta {eg:.2e}, scipy's cho_solve on A0 + V V^T {er:.2e}")
        assert eg <= 10 * max(er, U64)
    finally:
        p.close()
        q.close()


def test_state(drv):
    n = 1000
    rf = reference(n, 1e2)
    A = rf["A"]
    p = drv.Cholinv(n, complete_inv=1, bc_mult=-2)
    try:
        p.set_A(A)
        p.factor()
        assert p.equilibrate()[0]
        with pytest.raises(drv.DriverError, match="already equilibrated"):
            p.equilibrate()
        with pytest.raises(drv.DriverError, match="equilibrated"):
            p.factor_pivoted()
        with pytest.raises(drv.DriverError, match="factor\\(\\) has not run"):     # the factors were those of the unscaled A
            p.solve(rf["B"][:, :2])
        p.factor()
        p.solve(rf["B"][:, :2])
        p.set_A(A)                                                                 # a new matrix is not equilibrated
        assert np.all(p.scale() == 1.0)
        assert p.equilibrate()[0]
        p.unequilibrate()
        with pytest.raises(drv.DriverError, match="factor\\(\\) has not run"):
            p.solve(rf["B"][:, :2])
        rk = p.factor_pivoted(max_rank=8)[0]                                       # allowed again
        assert rk == 8
        for value, j in ((0.0, 0), (-1.0, n // 2), (np.nan, n - 1), (np.inf, 17)):
            bad = A.copy()
            bad[j, j] = value
            p.set_A(bad)
            with pytest.raises(drv.DriverError, match=f"diagonal entry {j + 1} "):
                p.equilibrate()
            assert p.A().tobytes() == bad.tobytes() and np.all(p.scale() == 1.0)
    finally:
        p.close()


WORK_CASES = [("complete", dict(complete_inv=1, bc_mult=-2)), ("block", dict(complete_inv=0, split=1, bc_mult=-3)), ("block-flush", dict(complete_inv=0, split=1, bc_mult=-3, flush_intermediates=True)),
              ("substitution", dict(bc_mult=-2, substitution=True)), ("trsm-rect", dict(bc_mult=-2, trsm_mode=True, serialize=False))]


def sequence(drv, rf, kw, poison):
    n = rf["A"].shape[0]
    B = rf["B"]
    p, _, _ = equilibrated(drv, rf, kw)
    try:
        if poison:                                                                 # NaN in every block that an equilibrated solve takes
            X, res = p.solve(np.full((n, 32), np.nan, order="F"), refine=1)
            assert np.isnan(X).all() and np.isnan(res).all()
            assert np.isnan(p.apply(np.full((n, 32), np.nan, order="F"), "R")).all()
        out = {}
        out["solve5.X"], out["solve5.res"] = p.solve(B[:, :5], refine=1)
        out["expert40.X"], out["expert40.res"], out["expert40.ferr"], out["expert40.berr"] = p.solve_expert(B, refine=1)
        for op in OPS:
            out["apply." + op] = p.apply(B[:, :33], op)
        out["quad"] = p.quadratic_forms(B[:, :5])
        return out
    finally:
        p.close()


@pytest.mark.parametrize("name,kw", WORK_CASES, ids=[c[0] for c in WORK_CASES])
def test_results_do_not_depend_on_stale_work(drv, name, kw):
    rf = reference(1000, 1e2)
    P, Q = sequence(drv, rf, kw, True), sequence(drv, rf, kw, False)
    assert P.keys() == Q.keys()
    for k in Q:
        assert np.isfinite(Q[k]).all(), k
        np.testing.assert_array_equal(P[k], Q[k], err_msg=k)
