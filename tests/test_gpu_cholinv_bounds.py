"""cholesky::cholinv::condition and error_bounds through driver.Cholinv.rcond / solve_expert on one GPU: the reciprocal condition number, and dporfs's
backward and forward error bounds of a solve on the resident factors, over the forms of the solve (complete inverse; block-wise with R12; TRSM mode;
substitution; packed and rect factors; no split; order 1) and over kappa = 1e2 .. 1e12 (F1 spectra, seed 3).

rcond, two ways.  Against rcond_true = 1 / (||A||_1 ||inv(A)||_1) from numpy: 0.9 <= rcond / rcond_true <= 3 (in exact arithmetic the estimate of
||A^-1||_1 never exceeds the norm, so the ratio is >= 1; 0.9 allows the kappa u error of the products at kappa = 1e12; 3 is the range in which
Higham's estimator is expected to stay).  Against scipy's dpocon on dpotrf of the same A: within a factor 2 either way (the same algorithm, but its
path may differ).  On the CPU dpocon gives 1.05 .. 1.33 rcond_true on these inputs, so the reference alone meets both.
berr.  On a residual of order one (the set_A(A2) device of test_gpu_cholinv_solve.py) berr must be the formula max_i |rho_i| / (|A2| |x| + |b|)_i
evaluated in numpy.longdouble on the returned X, to 1e-10, all 40 columns (two blocks).  On a real solve (refine = 1; r = 1, 5, 40) the project's
rule: berr <= 10 max(berr_ref, u) with berr_ref from scipy's dposvx on the same A and B (1.3e-16 .. 2.9e-16 on the CPU).
ferr.  x_true from six steps of numpy.longdouble refinement on cho_solve.  ferr_j >= ||x_j - x_true,j||_inf / ||x_j||_inf with refine = 0 and with
refine = 1 (without refinement the products with an explicit inverse leave a worse X, and the bound must follow it), and with refine = 1
ferr_j <= 10 x dposvx's ferr_j (which exceeds the true error by 3e3 .. 4e4 on these inputs: there is room below)."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla
from scipy.linalg import lapack

import _conditioning as cond

pytestmark = pytest.mark.gpu
U64 = 2.0 ** -53
LD = np.longdouble
KAPPAS = [1e2, 1e6, 1e10, 1e12]


@pytest.fixture(scope="module")
def drv():
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    yield driver
    driver.finalize()


_REF, _SOLVE = {}, {}


def reference(n, kappa):
    """A, B = A X0 (integer X0, 40 columns), ||A||_1, rcond_true and dpocon's rcond: once per (n, kappa)"""
    if (n, kappa) not in _REF:
        A = cond.f1_spectrum(n, kappa, seed=3)
        anorm = np.linalg.norm(A, 1)
        rcond_true = 1.0 / (anorm * np.linalg.norm(np.linalg.inv(A), 1))
        c, info = lapack.dpotrf(A, lower=0)
        rcond_lapack, info2 = lapack.dpocon(c, anorm, uplo="U")
        assert info == 0 and info2 == 0
        X0 = np.random.default_rng(n).integers(-8, 9, (n, 40)).astype(np.float64)
        X0[X0 == 0] = 1.0
        _REF[(n, kappa)] = (A, np.asfortranarray(A @ X0), anorm, rcond_true, rcond_lapack)
    return _REF[(n, kappa)]


def solve_reference(n, kappa, r):
    """x_true (longdouble refinement on cho_solve) and dposvx's ferr, berr for the first r columns of B: once per (n, kappa, r)"""
    if (n, kappa, r) not in _SOLVE:
        A, B = reference(n, kappa)[:2]
        B = np.asfortranarray(B[:, :r])
        cf = sla.cho_factor(A)
        Al, Bl = A.astype(LD), B.astype(LD)
        xt = sla.cho_solve(cf, B).astype(LD)
        for _ in range(6):
            xt = xt + sla.cho_solve(cf, (Bl - Al @ xt).astype(np.float64))
        out = lapack.dposvx(A, B, fact="N", lower=0)
        assert out[9] in (0, n + 1)                      # (n + 1: solved, rcond below eps -- not on these inputs, but no error either)
        _SOLVE[(n, kappa, r)] = (xt, out[7], out[8])
    return _SOLVE[(n, kappa, r)]


def true_error(X, xt):
    return (np.abs(X.astype(LD) - xt).max(axis=0) / np.abs(X).max(axis=0)).astype(np.float64)


POLICIES = [
    ("complete-inverse", 1000, dict(complete_inv=1, bc_mult=-2)),
    ("blocks-R12-packed", 2048, dict(complete_inv=0, split=1, bc_mult=-2, serialize=True)),
    ("blocks-R12-rect", 1000, dict(complete_inv=0, split=1, bc_mult=-2, serialize=False)),
    ("trsm", 2048, dict(bc_mult=-2, trsm_mode=True)),
    ("trsm-rect", 1000, dict(bc_mult=-2, trsm_mode=True, serialize=False)),
    ("substitution", 1000, dict(bc_mult=-2, substitution=True)),
    ("substitution-flush", 2048, dict(bc_mult=-2, substitution=True, flush_intermediates=True)),
    ("no-split", 512, dict(complete_inv=0)),
]
CASES = [(name, n, kw, kappa) for name, n, kw in POLICIES for kappa in KAPPAS] + [("order-one", 1, dict(), 1e2)]       # (order one has one spectrum)


@pytest.mark.parametrize("name,n,kw,kappa", CASES, ids=[f"{c[0]}-kappa{c[3]:.0e}" for c in CASES])
def test_rcond_and_bounds_over_policies(drv, name, n, kw, kappa):
    A, B, anorm, rcond_true, rcond_lapack = reference(n, kappa)
    r = 5
    xt, ferr_ref, berr_ref = solve_reference(n, kappa, r)
    p = drv.Cholinv(n, **kw)
    try:
        p.set_A(A)
        p.factor()
        assert (p.stats()["levels"] >= 1) == (n > 512)
        rc, an, applies = p.rcond(details=True)
        print(f"bounds {name} n={n} kappa={kappa:.0e}: rcond {rc:.4e} = {rc / rcond_true:.3f} rcond_true = {rc / rcond_lapack:.3f} dpocon's, "
              f"||A||_1 {an:.6e}, {applies} products")
        assert abs(an - anorm) <= 4 * n * U64 * anorm
        assert 1 <= applies <= 11
        assert 0.9 <= rc / rcond_true <= 3
        assert 0.5 <= rc / rcond_lapack <= 2
        assert p.rcond() == rc
        for refine in (0, 1):
            X, res, ferr, berr = p.solve_expert(B[:, :r], refine=refine)
            Xs, ress = p.solve(B[:, :r], refine=refine)
            assert X.tobytes() == Xs.tobytes() and res.tobytes() == ress.tobytes()         # solve_expert's X is solve's, and the bounds do not write it
            err = true_error(X, xt)
            print(f"bounds {name} n={n} kappa={kappa:.0e} refine={refine}: berr {berr.max():.2e} (dposvx {berr_ref.max():.2e}), "
                  f"ferr {ferr.min():.2e} .. {ferr.max():.2e} (dposvx {ferr_ref.min():.2e} .. {ferr_ref.max():.2e}), true error {err.max():.2e}, "
                  f"min ferr / error {(ferr / np.maximum(err, 1e-300)).min():.2e}")
            assert ferr.shape == berr.shape == (r,) and np.all(np.isfinite(ferr)) and np.all(np.isfinite(berr))
            assert np.all(ferr >= err), (ferr, err)
            if refine == 1:
                assert np.all(berr <= 10 * np.maximum(berr_ref, U64)), (berr, berr_ref)
                assert np.all(ferr <= 10 * ferr_ref), (ferr, ferr_ref)
        if kappa == 1e6:
            again = p.solve_expert(B[:, :r], refine=1)
            assert p.rcond(details=True) == (rc, an, applies)
            for a, b in zip(again, (X, res, ferr, berr)):
                assert a.tobytes() == b.tobytes()
    finally:
        p.close()


@pytest.mark.parametrize("kw", [dict(complete_inv=0, bc_mult=-2), dict(bc_mult=-2, trsm_mode=True, serialize=False)], ids=["inverse", "trsm"])
def test_berr_on_a_residual_of_order_one(drv, kw):
    n, kappa = 1000, 1e2
    A, B = reference(n, kappa)[:2]
    A2 = cond.symmetrize(A + 0.01 * np.random.default_rng(n + 1).standard_normal((n, n)))
    p = drv.Cholinv(n, **kw)
    try:
        p.set_A(A)
        p.factor()
        p.set_A(A2)                                       # the factors stay those of A: X solves A X = B, the residual is that of A2
        X, res, ferr, berr = p.solve_expert(B, refine=0)
    finally:
        p.close()
    Xl, A2l = X.astype(LD), A2.astype(LD)
    rho = np.abs(B.astype(LD) - A2l @ Xl)
    w = np.abs(A2l) @ np.abs(Xl) + np.abs(B.astype(LD))
    ref = (rho / w).max(axis=0).astype(np.float64)
    rel = np.abs(berr - ref) / ref
    print(f"berr against A2, {kw}: berr {berr.min():.3e} .. {berr.max():.3e}, max |berr - longdouble| / berr = {rel.max():.2e}")
    assert berr.shape == (40,) and ref.min() > 1e-4 and rel.max() <= 1e-10
    assert np.all(ferr > 0) and np.all(np.isfinite(ferr))


@pytest.mark.parametrize("kappa", KAPPAS, ids=[f"kappa{k:.0e}" for k in KAPPAS])
def test_bounds_of_a_real_solve_over_column_counts(drv, kappa):
    n = 1000
    A, B = reference(n, kappa)[:2]
    p = drv.Cholinv(n, complete_inv=0, bc_mult=-2)
    try:
        p.set_A(A)
        p.factor()
        for r in (1, 40):                                 # (5 columns: the test over the policies); 40: two blocks of columns
            xt, ferr_ref, berr_ref = solve_reference(n, kappa, r)
            X, res, ferr, berr = p.solve_expert(B[:, :r], refine=1)
            err = true_error(X, xt)
            print(f"bounds n={n} kappa={kappa:.0e} r={r}: berr {berr.max():.2e} (dposvx {berr_ref.max():.2e}), ferr {ferr.max():.2e} "
                  f"(dposvx {ferr_ref.max():.2e}), true error {err.max():.2e}")
            assert np.all(berr <= 10 * np.maximum(berr_ref, U64)), (berr, berr_ref)
            assert np.all(ferr >= err) and np.all(ferr <= 10 * ferr_ref)
            X0, _, ferr0, _ = p.solve_expert(B[:, :r], refine=0)
            assert np.all(ferr0 >= true_error(X0, xt))
    finally:
        p.close()


def test_misuse(drv):
    n = 256
    dp = C.POINTER(C.c_double)
    p = drv.Cholinv(n)
    try:
        p.generate()
        with pytest.raises(drv.DriverError, match="factor\\(\\) has not run"):
            p.rcond()
        with pytest.raises(drv.DriverError, match="factor\\(\\) has not run"):
            p.solve_expert(np.ones((n, 2)))
        p.factor()
        with pytest.raises(drv.DriverError):
            p.solve_expert(np.ones((n - 1, 2)))
        # error_bounds on its own: before any solve there is no X; after one, B must have its number of columns
        b = np.ones((n, 3), order="F")
        f, e = np.zeros(3), np.zeros(3)
        assert p.D.capital_cholinv_error_bounds(p.p, 3, b.ctypes.data_as(dp), f.ctypes.data_as(dp), e.ctypes.data_as(dp)) != 0
        assert b"resident X" in p.D.capital_drv_last_error()
        X, _ = p.solve(np.ones((n, 2)))
        assert p.D.capital_cholinv_error_bounds(p.p, 3, b.ctypes.data_as(dp), f.ctypes.data_as(dp), e.ctypes.data_as(dp)) != 0
        assert b"resident X" in p.D.capital_drv_last_error()
        assert p.D.capital_cholinv_error_bounds(p.p, 2, b.ctypes.data_as(dp), f.ctypes.data_as(dp), e.ctypes.data_as(dp)) == 0
        assert np.all(f[:2] > 0) and np.all(e[:2] >= 0)
        assert p.D.capital_cholinv_error_bounds(p.p, 2, None, f.ctypes.data_as(dp), e.ctypes.data_as(dp)) != 0
        # the other mode's factors are refused, as solve() refuses them
        assert p.D.capital_cholinv_set_trsm_mode(p.p, 1) == 0
        with pytest.raises(drv.DriverError, match="mode"):
            p.rcond()
        with pytest.raises(drv.DriverError, match="mode"):
            p.solve_expert(np.ones((n, 2)))
    finally:
        p.close()
