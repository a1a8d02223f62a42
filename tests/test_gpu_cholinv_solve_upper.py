"""cholesky::cholinv::solve on an UPPER-STORED A, through driver.Cholinv on one GPU: factor() reads A's upper triangle alone (LAPACK's convention),
and so do the refinement and the residual norms of solve() (capi_dresid_sym).  The device copy of A holds NaN below the diagonal -- or other finite
values, which must not change a bit of X or of the norms.

Parity: X against scipy.linalg.cho_solve (on the symmetric matrix) to 1e-12 max |X_ref|; norms by the rule of test_gpu_cholinv_solve.check_parity,
|res - numpy| / (||A|| ||x|| + ||b||) <= 1e-10, and on a residual of order one (the device copy replaced by the upper triangle of a perturbed A2)
to 1e-10 relative.  Conditioning: the project's rule eta <= 10 max(eta_ref, u), eta_ref from cho_solve on the symmetric matrix."""
import numpy as np
import pytest
import scipy.linalg as sla

import _conditioning as cond

pytestmark = pytest.mark.gpu
U64 = 2.0 ** -53
LD = np.longdouble
N = 2048

CONFIGS = {
    "packed-ci0": dict(complete_inv=0, serialize=True),
    "packed-ci1": dict(complete_inv=1, serialize=True),
    "rect": dict(complete_inv=0, serialize=False),
    "trsm": dict(serialize=False, trsm_mode=True),
}


@pytest.fixture(scope="module")
def drv():
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    yield driver
    driver.finalize()


def upper_only(A, lower=np.nan):
    n = A.shape[0]
    return np.asfortranarray(np.where(np.arange(n)[:, None] > np.arange(n)[None, :], lower, A))


_REF = {}


def reference(A):
    """right-hand sides and cho_solve's solution for generate()'s matrix, computed once and shared (generate() is deterministic: checked)"""
    if "A" not in _REF:
        n = A.shape[0]
        X0 = np.asfortranarray(np.random.default_rng(n).integers(-8, 9, (n, 40)).astype(np.float64))
        B = np.asfortranarray(A @ X0)
        _REF.update(A=A.copy(), B=B, X=sla.cho_solve(sla.cho_factor(A), B), normA=np.linalg.norm(A))
    assert np.array_equal(_REF["A"], A)
    return _REF["B"], _REF["X"], _REF["normA"]


@pytest.mark.parametrize("config", list(CONFIGS))
def test_parity_from_the_upper_triangle(drv, config):
    p = drv.Cholinv(N, bc_mult=-2, **CONFIGS[config])
    try:
        p.generate()
        A = p.A()
        B, Xref, normA = reference(A)
        p.set_A(upper_only(A))
        p.factor()
        for r in (1, 5, 40):
            X, res = p.solve(B[:, :r], refine=1, residual=True)
            assert np.all(np.isfinite(X)) and np.all(np.isfinite(res))
            err = np.abs(X - Xref[:, :r]).max() / np.abs(Xref[:, :r]).max()
            ref_res = np.linalg.norm(B[:, :r] - A @ X, axis=0)
            scale = normA * np.linalg.norm(X, axis=0) + np.linalg.norm(B[:, :r], axis=0)
            rerr = np.max(np.abs(res - ref_res) / scale)
            print(f"upper-stored solve {config} r={r}: |X - cho_solve| / max|X| = {err:.2e}, |resnorm - numpy| / scale = {rerr:.2e}")
            assert err <= 1e-12
            assert res.shape == (r,) and rerr <= 1e-10
        # a residual of order one: the device copy becomes the upper triangle of a perturbed A2, the factors stay those of A
        E = np.random.default_rng(N + 1).standard_normal((N, N)) * 0.01
        A2 = cond.symmetrize(A + E)
        p.set_A(upper_only(A2))
        X, res = p.solve(B, refine=0)
        ref_res = np.linalg.norm(B - A2 @ X, axis=0)
        rel = np.max(np.abs(res - ref_res) / ref_res)
        print(f"upper-stored solve {config} r=40 against A2: resnorm {res.min():.3e} .. {res.max():.3e}, max |resnorm - numpy| / resnorm = {rel:.2e}")
        assert res.shape == (40,) and ref_res.min() > 1e-3 and rel <= 1e-10
    finally:
        p.close()


def test_the_lower_triangle_is_ignored(drv):
    p = drv.Cholinv(N, bc_mult=-2, **CONFIGS["packed-ci0"])
    try:
        p.generate()
        A = p.A()
        B = reference(A)[0]
        p.factor()
        X1, r1 = p.solve(B, refine=1, residual=True)
        p.set_A(upper_only(A, 100.0 * np.random.default_rng(5).standard_normal((N, N))))
        p.factor()
        X2, r2 = p.solve(B, refine=1, residual=True)
    finally:
        p.close()
    assert np.array_equal(X1, X2) and np.array_equal(r1, r2)


def eta(A, normA2, B, X):
    R = B.astype(LD) - A.astype(LD) @ X.astype(LD)
    num = np.sqrt((R * R).sum(axis=0))
    den = LD(normA2) * np.sqrt((X.astype(LD) ** 2).sum(axis=0)) + np.sqrt((B.astype(LD) ** 2).sum(axis=0))
    return float((num / den).max())


def test_backward_error_on_an_ill_conditioned_upper_stored_matrix(drv):
    n, kappa = 1000, 1e8
    A = cond.f1_spectrum(n, kappa)
    B = np.asfortranarray(A @ np.random.default_rng(8).standard_normal((n, 3)))
    normA2 = np.linalg.norm(A, 2)
    eta_ref = eta(A, normA2, B, sla.cho_solve(sla.cho_factor(A), B))
    p = drv.Cholinv(n, complete_inv=0, bc_mult=-2)
    try:
        p.set_A(upper_only(A))
        p.factor()
        X, res = p.solve(B, refine=1, residual=True)
    finally:
        p.close()
    assert np.all(np.isfinite(X)) and np.all(np.isfinite(res))
    e = eta(A, normA2, B, X)
    print(f"upper-stored solve kappa={kappa:.0e}: eta {e:.2e} (cho_solve {eta_ref:.2e})")
    assert e <= 10 * max(eta_ref, U64), (e, eta_ref)
