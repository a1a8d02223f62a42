"""The factors themselves through driver.Cholinv on one GPU: apply (R, R^T, R^-1, R^-T on a thin block), quadratic_forms (b^T A^-1 b), logdet and
inverse_diagonal (diag A^-1), in every form that solve() has -- products with the complete inverse, the block form where complete_inv = 0 left
R^-1_12 unformed, capi_dtrsm in TRSM mode, substitution -- and after update().  u = 2^-53 throughout.

apply: on the device's OWN factors (p.R(), p.Rinv() fetched), a product of n terms stays componentwise within 1.01 (n + 1) u (|T| |B|) of the
  longdouble product: R and R^T always, R^-1 and R^-T where the complete inverse form runs.  The other three forms solve, and are held to the project's rule
  eta_gpu <= 10 max(eta_ref, u) on the normwise backward error eta = max_j ||op(R) y_j - b_j|| / (||R||_2 ||y_j|| + ||b_j||) in longdouble on the fetched R;
  eta_ref is the same form restated in numpy (tests/_apply_ref.py) on numpy's own factor.  ||R||_2 is taken once per matrix from numpy's factor (the
  fetched one agrees with it to rounding, and an SVD per case costs two seconds).
  apply("Rinv", apply("RinvT", B)) must equal solve(B, refine=0) bit for bit, and error_bounds after an apply must see the X of the last solve.
quadratic_forms: (n + 1) u relative against the longdouble column norms of apply("RinvT", B) (any order of n squares, test_gpu_tri_rownorm2.py), and
  1e-12 relative against b^T cho_solve(b): the parity level the project uses on generate()'s matrix.
logdet: against 2 sum log of the fetched diagonal under capi_dtri_logdiag's bound (n + 3) u sum |log r_ii|, doubled.
inverse_diagonal: the complete form against the row sums of squares of the fetched Rinv() under capi_dtri_rownorm2's bound; the block form against the
  complete form of the same matrix and both against diag(cho_solve(I)) to 1e-12 relative."""
import ctypes as C
import itertools

import numpy as np
import pytest
import scipy.linalg as sla

import _apply_ref as ref
import _conditioning as cond

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


def reference(tag, A):
    """what the checks need of the host, computed once per matrix and shared: B (n x 40), cho_solve(B), diag(A^-1), numpy's factor and its 2-norm"""
    if tag not in _REF:
        n = A.shape[0]
        rng = np.random.default_rng(n)
        B = np.asfortranarray(A @ rng.integers(-8, 9, (n, 40)).astype(np.float64))
        cf = sla.cho_factor(A)
        Rn = ref.chol_upper(A)
        _REF[tag] = {"A": A.copy(), "B": B, "X": sla.cho_solve(cf, B), "diag": np.diag(sla.cho_solve(cf, np.eye(n))).copy(), "Rn": Rn,
                     "normR2": np.linalg.norm(Rn, 2), "eta": {}, "logdet": 2.0 * np.log(np.diag(Rn)).sum()}
    assert np.array_equal(_REF[tag]["A"], A)
    return _REF[tag]


def eta_ref(rf, form, h1, trans):
    """the backward error of the form's numpy restatement on numpy's factor, once per matrix, form and direction"""
    key = (form, h1, trans)
    if key not in rf["eta"]:
        Y = ref.half(rf["Rn"], rf["B"], trans, form, h1=h1)
        rf["eta"][key] = ref.eta_half(rf["Rn"], rf["normR2"], rf["B"], Y, trans)
    return rf["eta"][key]


def check_product(what, T, B, Y):
    n = T.shape[0]
    want = T.astype(LD) @ B.astype(LD)
    bound = 1.01 * (n + 1) * U64 * (np.abs(T) @ np.abs(B))
    err = np.abs(Y.astype(LD) - want)
    print(f"  {what}: max err / bound = {float((err / bound).max()):.3f}")
    assert np.all(err <= bound), what


def check_all(p, rf, form, h1, drv):
    """every check of the module's docstring on the factors that p holds of the matrix rf describes; form: what apply_half runs"""
    B, n = rf["B"], rf["A"].shape[0]
    R = p.R()
    Ri = p.Rinv() if form != "trsm" else None
    Y = {op: p.apply(B, op) for op in OPS}                                 # 40 columns: two blocks of right-hand sides
    for r in (1, 5):
        for op in OPS:
            assert p.apply(B[:, :r], op).tobytes() == np.asfortranarray(Y[op][:, :r]).tobytes(), (op, r)      # a column does not depend on its neighbours
    check_product("R B", np.triu(R), B, Y["R"])
    check_product("R^T B", np.triu(R).T, B, Y["RT"])
    if form == "complete":
        check_product("R^-1 B", np.triu(Ri), B, Y["Rinv"])
        check_product("R^-T B", np.triu(Ri).T, B, Y["RinvT"])
    else:
        for op, trans in (("RinvT", 1), ("Rinv", 0)):
            e, er = ref.eta_half(R, rf["normR2"], B, Y[op], trans), eta_ref(rf, form, h1, trans)
            print(f"  {op} ({form}): eta {e:.2e}, numpy restatement {er:.2e}")
            assert e <= 10 * max(er, U64), (op, e, er)
    for r in (1, 5, 40):
        X = p.solve(B[:, :r], refine=0, residual=False)[0]
        assert np.array_equal(p.apply(p.apply(B[:, :r], "RinvT"), "Rinv"), X), r
    # error_bounds after an apply still sees the X of the last solve, and solve_expert returns what it returned before
    b5 = np.asfortranarray(B[:, :5])
    first = p.solve_expert(b5)
    p.apply(B, "R")
    p.quadratic_forms(B)
    ferr, berr = np.zeros(5), np.zeros(5)
    dp = C.POINTER(C.c_double)
    assert p.D.capital_cholinv_error_bounds(p.p, 5, b5.ctypes.data_as(dp), ferr.ctypes.data_as(dp), berr.ctypes.data_as(dp)) == 0
    assert ferr.tobytes() == first[2].tobytes() and berr.tobytes() == first[3].tobytes()
    for a, b in zip(first, p.solve_expert(b5)):
        assert a.tobytes() == b.tobytes()
    # quadratic forms
    for r in (1, 5, 40):
        q = p.quadratic_forms(B[:, :r])
        qy = (Y["RinvT"][:, :r].astype(LD) ** 2).sum(axis=0)
        qs = (B[:, :r] * rf["X"][:, :r]).sum(axis=0)
        e1, e2 = float((np.abs(q - qy) / qy).max()), float((np.abs(q - qs) / qs).max())
        print(f"  quadratic_forms r={r}: against ||R^-T b||^2 {e1:.2e} (bound {(n + 1) * U64:.2e}), against b^T cho_solve(b) {e2:.2e}")
        assert q.shape == (r,) and e1 <= (n + 1) * U64 and e2 <= 1e-12
    # log-determinant
    logs = np.log(np.diag(R).astype(LD))
    ld = p.logdet()
    e = abs(LD(ld) - 2 * logs.sum())
    print(f"  logdet {ld:.6f}: |gpu - 2 sum log r_ii| = {float(e):.2e}, bound {float(2 * (n + 3) * U64 * np.abs(logs).sum()):.2e}")
    assert e <= 2 * (n + 3) * U64 * np.abs(logs).sum()
    S = 2 * float(np.abs(logs).sum())
    assert abs(ld - rf["logdet"]) <= 10 * n * U64 * S                      # scipy's factor of the same matrix: the rule of the conditioning test with no truth at hand
    # diagonal of the inverse
    if form == "trsm":
        with pytest.raises(drv.DriverError, match="TRSM mode forms no inverse"):
            p.inverse_diagonal()
        return None
    d = p.inverse_diagonal()
    e = float((np.abs(d - rf["diag"]) / rf["diag"]).max())
    print(f"  inverse_diagonal: against diag(cho_solve(I)) {e:.2e}")
    assert d.shape == (n,) and e <= 1e-12
    if p.complete_form:
        Sd = (np.triu(Ri).astype(LD) ** 2).sum(axis=1)
        err, bound = np.abs(d.astype(LD) - Sd), 1.01 * (n - np.arange(n) + 1) * U64 * Sd
        assert np.all(err <= bound)
    assert p.inverse_diagonal().tobytes() == d.tobytes()
    return d


def factored(drv, n, A=None, **kw):
    """a factored problem; complete_form: inverse_diagonal reads one complete triangle"""
    p = drv.Cholinv(n, **kw)
    if A is None:
        p.generate()
    else:
        p.set_A(A)
    p.factor()
    p.complete_form = bool(kw.get("complete_inv", 0)) or p.stats()["levels"] == 0
    return p


def form_of(p, n, split):
    """what apply_half runs in inverse mode without substitution, and the order of the leading block in the block form"""
    return ("complete", None) if p.complete_form else ("block", n >> split)


_COMPLETE = {}


def against_complete_form(drv, tag, A, d, **kw):
    """the block form's diagonal d against the complete form (complete_inv = 1) of the same matrix, factored once per matrix: 1e-12 relative"""
    if tag not in _COMPLETE:
        q = factored(drv, A.shape[0], A=A, complete_inv=1, **kw)
        try:
            assert q.stats()["levels"] >= 1
            _COMPLETE[tag] = q.inverse_diagonal()
        finally:
            q.close()
    e = float((np.abs(d - _COMPLETE[tag]) / _COMPLETE[tag]).max())
    print(f"  inverse_diagonal {tag}: block form against complete form {e:.2e}")
    assert e <= 1e-12


CONFIGS = list(itertools.product((0, 1), (1, 2), (True, False), (False, True)))


@pytest.mark.parametrize("complete_inv,split,serialize,flush", CONFIGS,
                         ids=[f"ci{c}-split{s}-{'ser' if se else 'noser'}-{'flush' if f else 'save'}" for c, s, se, f in CONFIGS])
def test_over_policies(drv, complete_inv, split, serialize, flush):
    n = 2048
    p = factored(drv, n, complete_inv=complete_inv, split=split, bc_mult=-2, serialize=serialize, flush_intermediates=flush)
    try:
        assert p.stats()["levels"] >= 1
        rf = reference("gen2048", p.A())
        form, h1 = form_of(p, n, split)
        assert form == ("complete" if complete_inv else "block")
        d = check_all(p, rf, form, h1, drv)
        if form == "block":
            against_complete_form(drv, "gen2048", rf["A"], d, bc_mult=-2)
    finally:
        p.close()


@pytest.mark.parametrize("n,bc_mult,split", [(1536, -2, 2), (1000, -3, 1)])
def test_other_split_positions(drv, n, bc_mult, split):
    p = factored(drv, n, complete_inv=0, split=split, bc_mult=bc_mult)
    try:
        assert p.stats()["levels"] >= 1
        rf = reference(f"gen{n}", p.A())
        form, h1 = form_of(p, n, split)
        assert form == "block" and h1 == n >> split
        against_complete_form(drv, f"gen{n}", rf["A"], check_all(p, rf, form, h1, drv), split=split, bc_mult=bc_mult)
    finally:
        p.close()


def test_when_the_recursion_does_not_split(drv):
    p = factored(drv, 512, complete_inv=0)
    try:
        assert p.stats()["levels"] == 0
        check_all(p, reference("gen512", p.A()), "complete", None, drv)
    finally:
        p.close()


def test_trsm_mode(drv):
    n = 2048
    p = factored(drv, n, bc_mult=-2, trsm_mode=True)
    try:
        check_all(p, reference("gen2048", p.A()), "trsm", None, drv)
    finally:
        p.close()
    # with Serialize + FlushIntermediates only the packed R is resident: the inverses have no image to run on, R, R^T and logdet read it as it lies
    p = factored(drv, n, bc_mult=-2, serialize=True, flush_intermediates=True, trsm_mode=True)
    try:
        rf = reference("gen2048", p.A())
        with pytest.raises(drv.DriverError, match="FlushIntermediates"):
            p.apply(rf["B"], "Rinv")
        R = p.R()
        check_product("R B (packed R alone)", np.triu(R), rf["B"], p.apply(rf["B"], "R"))
        assert abs(p.logdet() - rf["logdet"]) <= 10 * n * U64 * 2 * np.abs(np.log(np.diag(R))).sum()
    finally:
        p.close()


def test_substitution(drv):
    n = 2048
    p = factored(drv, n, bc_mult=-2, substitution=True)
    try:
        check_all(p, reference("gen2048", p.A()), "subst", None, drv)
    finally:
        p.close()


def test_logdet_under_conditioning(drv):
    """f1_spectrum(512, 1e8) has the eigenvalues logspace(0, -8, 512): the truth is their log-sum in longdouble.  Rule: e_gpu <= 10 max(e_ref, n u S), S =
    2 sum |log r_ii| and e_ref the error of scipy's float64 factor (on the CPU: e_ref = 1.2e-8, n u S = 2.7e-10)"""
    n, kappa = 512, 1e8
    A = cond.f1_spectrum(n, kappa)
    truth = np.log(np.logspace(0, -np.log10(kappa), n).astype(LD)).sum()
    Rs = sla.cholesky(A)
    e_ref = float(abs(LD(2.0 * np.log(np.diag(Rs)).sum()) - truth))
    S = 2.0 * np.abs(np.log(np.diag(Rs))).sum()
    for complete_inv in (0, 1):
        p = factored(drv, n, A=A, complete_inv=complete_inv, bc_mult=-2)
        try:
            e = float(abs(LD(p.logdet()) - truth))
        finally:
            p.close()
        print(f"logdet kappa={kappa:.0e} complete_inv={complete_inv}: e_gpu {e:.2e}, e_ref {e_ref:.2e}, n u S {n * U64 * S:.2e}")
        assert e <= 10 * max(e_ref, n * U64 * S)


def test_inverse_diagonal_under_conditioning(drv):
    """A = Q diag(lambda) Q^T with kappa = 1e8: the truth is sum_k Q_ik^2 / lambda_k in longdouble.  Rule: e_gpu <= 10 max(e_ref, u) with e = max_i |d_i -
    truth_i| / max_i truth_i (the perturbation bound of an inverse is normwise) and e_ref from scipy's cho_solve in float64; both forms"""
    n, kappa = 512, 1e8
    Q = cond.orthogonal(n, np.random.default_rng(5))
    lam = np.logspace(0, -np.log10(kappa), n)
    A = cond.symmetrize((Q * lam[None, :]) @ Q.T)
    truth = ((Q.astype(LD) ** 2) / lam.astype(LD)[None, :]).sum(axis=1)
    err = lambda d: float(np.abs(d.astype(LD) - truth).max() / truth.max())
    e_ref = err(np.diag(sla.cho_solve(sla.cho_factor(A), np.eye(n))))
    for complete_inv in (0, 1):
        p = factored(drv, n, A=A, complete_inv=complete_inv, bc_mult=-2)
        try:
            assert p.stats()["levels"] >= 1
            e = err(p.inverse_diagonal())
        finally:
            p.close()
        print(f"inverse_diagonal kappa={kappa:.0e} complete_inv={complete_inv}: e_gpu {e:.2e}, e_ref {e_ref:.2e}")
        assert e <= 10 * max(e_ref, U64)


@pytest.mark.parametrize("complete_inv", [0, 1])
def test_after_update_and_downdate(drv, complete_inv):
    n = 1024
    p = factored(drv, n, complete_inv=complete_inv, bc_mult=-2)
    try:
        assert p.stats()["levels"] >= 1
        form, h1 = form_of(p, n, 1)
        V = np.asfortranarray(np.random.default_rng(9).standard_normal((n, 3)) * 0.5)
        p.update(V)
        A1 = cond.symmetrize(p.A())                                        # update() keeps A's upper triangle current
        d1 = check_all(p, reference(f"upd{n}", A1), form, h1, drv)
        p.update(V, downdate=True)
        A2 = cond.symmetrize(p.A())
        d2 = check_all(p, reference(f"down{n}", A2), form, h1, drv)
        if form == "block":                                                # against a fresh factorisation of the updated matrices
            against_complete_form(drv, f"upd{n}", A1, d1, bc_mult=-2)
            against_complete_form(drv, f"down{n}", A2, d2, bc_mult=-2)
    finally:
        p.close()


def test_refusals(drv):
    n = 256
    ones = np.ones((n, 2))
    every = (lambda p: p.apply(ones, "R"), lambda p: p.apply(ones, "RinvT"), lambda p: p.quadratic_forms(ones), lambda p: p.logdet(),
             lambda p: p.inverse_diagonal())
    p = drv.Cholinv(n)
    try:
        p.generate()
        for f in every:                                                    # before factor()
            with pytest.raises(drv.DriverError, match="factor\\(\\) has not run"):
                f(p)
        p.factor()
        for f in (lambda: p.apply(np.ones((n - 1, 2)), "R"), lambda: p.quadratic_forms(np.ones((n + 1, 1))), lambda: p.apply(ones, "Rt")):
            with pytest.raises(drv.DriverError, match="must be"):
                f()
        dp = C.POINTER(C.c_double)
        b = np.ones((n, 2), order="F")
        bp = b.ctypes.data_as(dp)
        assert p.D.capital_cholinv_apply(p.p, 4, 2, bp, bp) != 0 and b"op 0..3" in p.D.capital_drv_last_error()
        assert p.D.capital_cholinv_apply(p.p, 0, 0, bp, bp) != 0
        assert p.D.capital_cholinv_quadratic_forms(p.p, 2, None, bp) != 0
        assert p.D.capital_cholinv_logdet(p.p, None) != 0 and p.D.capital_cholinv_inverse_diagonal(p.p, None) != 0
        A = p.A()
        V = np.zeros((n, 1))
        V[0, 0] = 2.0 * np.sqrt(A[0, 0])                                   # A - V V^T has a negative leading entry
        with pytest.raises(drv.DriverError, match="not positive definite"):
            p.update(V, downdate=True)
        for f in every:                                                    # after a failed downdate
            with pytest.raises(drv.DriverError, match="did not succeed"):
                f(p)
        p.factor()
        assert np.isfinite(p.logdet())
        p.set_A(cond.f4_indefinite(n, [100]))
        with pytest.raises(drv.DriverError, match="not positive definite"):
            p.factor()
        for f in every:                                                    # after a factor() that threw
            with pytest.raises(drv.DriverError, match="did not succeed"):
                f(p)
    finally:
        p.close()
    p = factored(drv, n, trsm_mode=True)
    try:
        with pytest.raises(drv.DriverError, match="TRSM mode forms no inverse"):
            p.inverse_diagonal()
    finally:
        p.close()
