"""cholesky::cholinv::solve through driver.Cholinv.solve on one GPU: A X = B on the resident factors -- products with R^-1 (block-wise with
R^-1_11, R^-1_22 and R_12 where complete_inv = 0 left R^-1_12 unformed), or capi_dtrsm on R in TRSM mode -- with refinement and residual norms.

Parity: X against scipy.linalg.cho_solve to 1e-12 max |X_ref| on generate()'s matrix (kappa ~ 1.5).
Residual norms: to 1e-10 relative to the norm itself.  On B = A X0 the residual of a solve is at the rounding level of its own evaluation, where two
summation orders share no digit, so the norms are checked on a residual of order one: after factor() the device copy of A is replaced by a
different symmetric A2 (set_A), and solve(B, refine=0) must return ||b_j - A2 x_j||_2 for the x_j of the factored A, all 40 of them (two column
blocks).  On the solve's own residual the returned norms are only required to agree with numpy's on the scale of the summed terms.
Conditioning: the normwise backward error eta = max_j ||b_j - A x_j|| / (||A||_2 ||x_j|| + ||b_j||) in numpy.longdouble (x87 80-bit here) under the
project's rule eta_gpu <= 10 max(eta_ref, u); eta_ref from the same algorithm restated in numpy (refine = 0: products with the inverse of
numpy's Cholesky factor) or from cho_solve (refine = 1).  On the CPU the references give 2e-16..8e-16 and 1.0e-16..2.1e-16 on these inputs."""
import itertools

import numpy as np
import pytest
import scipy.linalg as sla

import _conditioning as cond

pytestmark = pytest.mark.gpu
U64 = 2.0 ** -53
LD = np.longdouble


@pytest.fixture(scope="module")
def drv():
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    yield driver
    driver.finalize()


_REF = {}


def reference(A):
    """cho_factor of generate()'s matrix, computed once per order and shared (generate() is deterministic: checked)"""
    n = A.shape[0]
    if n not in _REF:
        rng = np.random.default_rng(n)
        X0 = np.asfortranarray(rng.integers(-8, 9, (n, 40)).astype(np.float64))
        B = np.asfortranarray(A @ X0)
        cf = sla.cho_factor(A)
        _REF[n] = (A.copy(), B, sla.cho_solve(cf, B), np.linalg.norm(A))
    assert np.array_equal(_REF[n][0], A)
    return _REF[n][1:]


def check_parity(p, A, refine=1):
    B, Xref, normA = reference(A)
    for r in (1, 5, 40):                                   # 40: the loop over blocks of 32 right-hand sides runs twice
        X, res = p.solve(B[:, :r], refine=refine)
        err = np.abs(X - Xref[:, :r]).max() / np.abs(Xref[:, :r]).max()
        ref_res = np.linalg.norm(B[:, :r] - A @ X, axis=0)
        scale = normA * np.linalg.norm(X, axis=0) + np.linalg.norm(B[:, :r], axis=0)
        rerr = np.max(np.abs(res - ref_res) / scale)
        print(f"solve n={A.shape[0]} r={r}: |X - cho_solve| / max|X| = {err:.2e}, resnorm max {res.max():.2e}, |resnorm - numpy| / scale = {rerr:.2e}")
        assert err <= 1e-12
        assert res.shape == (r,) and rerr <= 1e-10
    # the norm path on a residual of order one: A2 replaces the device copy of A, the factors stay those of A
    n = A.shape[0]
    E = np.random.default_rng(n + 1).standard_normal((n, n)) * 0.01
    A2 = cond.symmetrize(A + E)
    p.set_A(A2)
    try:
        X, res = p.solve(B, refine=0)
    finally:
        p.set_A(A)
    ref_res = np.linalg.norm(B - A2 @ X, axis=0)
    rel = np.max(np.abs(res - ref_res) / ref_res)
    print(f"solve n={n} r=40 against A2: resnorm {res.min():.3e} .. {res.max():.3e}, max |resnorm - numpy| / resnorm = {rel:.2e}")
    assert res.shape == (40,) and ref_res.min() > 1e-3 and rel <= 1e-10


CONFIGS = list(itertools.product((0, 1), (1, 2), (True, False), (False, True)))


@pytest.mark.parametrize("complete_inv,split,serialize,flush", CONFIGS,
                         ids=[f"ci{c}-split{s}-{'ser' if se else 'noser'}-{'flush' if f else 'save'}" for c, s, se, f in CONFIGS])
def test_solve_parity_over_policies(drv, complete_inv, split, serialize, flush):
    p = drv.Cholinv(2048, complete_inv=complete_inv, split=split, bc_mult=-2, serialize=serialize, flush_intermediates=flush)
    try:
        p.generate()
        p.factor()
        assert p.stats()["levels"] >= 1                    # the recursion split
        check_parity(p, p.A())
    finally:
        p.close()


@pytest.mark.parametrize("n,bc_mult,split", [(2048, -1, 1), (2048, -3, 1), (1536, -2, 2), (1000, -3, 1)])
def test_solve_parity_over_base_case_sizes(drv, n, bc_mult, split):
    """other split positions and depths of the recursion (h1 = n >> split)"""
    p = drv.Cholinv(n, complete_inv=0, split=split, bc_mult=bc_mult)
    try:
        p.generate()
        p.factor()
        assert p.stats()["levels"] >= 1
        check_parity(p, p.A())
    finally:
        p.close()


def test_solve_when_the_recursion_does_not_split(drv):
    p = drv.Cholinv(512, complete_inv=0)
    try:
        p.generate()
        p.factor()
        assert p.stats()["levels"] == 0
        check_parity(p, p.A())
    finally:
        p.close()


def eta(A, normA2, B, X):
    R = B.astype(LD) - A.astype(LD) @ X.astype(LD)
    num = np.sqrt((R * R).sum(axis=0))
    den = LD(normA2) * np.sqrt((X.astype(LD) ** 2).sum(axis=0)) + np.sqrt((B.astype(LD) ** 2).sum(axis=0))
    return float((num / den).max())


@pytest.mark.parametrize("kappa", [1e2, 1e6, 1e10, 1e12])
def test_backward_error_under_conditioning(drv, kappa):
    n = 1000
    A = cond.f1_spectrum(n, kappa)
    B = np.asfortranarray(A @ np.random.default_rng(int(np.log10(kappa))).standard_normal((n, 3)))
    normA2 = np.linalg.norm(A, 2)
    Rn = np.linalg.cholesky(A).T
    Ri = sla.solve_triangular(Rn, np.eye(n))
    eta_ref0 = eta(A, normA2, B, Ri @ (Ri.T @ B))
    eta_ref1 = eta(A, normA2, B, sla.cho_solve(sla.cho_factor(A), B))
    for complete_inv in (0, 1):
        p = drv.Cholinv(n, complete_inv=complete_inv, bc_mult=-2)
        try:
            p.set_A(A)
            p.factor()
            e0 = eta(A, normA2, B, p.solve(B, refine=0, residual=False)[0])
            e1 = eta(A, normA2, B, p.solve(B, refine=1, residual=False)[0])
        finally:
            p.close()
        print(f"solve kappa={kappa:.0e} complete_inv={complete_inv}: eta refine=0 {e0:.2e} (numpy restatement {eta_ref0:.2e}), "
              f"refine=1 {e1:.2e} (cho_solve {eta_ref1:.2e})")
        assert e0 <= 10 * max(eta_ref0, U64), (e0, eta_ref0)
        assert e1 <= 10 * max(eta_ref1, U64), (e1, eta_ref1)


def test_trsm_mode(drv):
    n = 2048
    xs = []
    for serialize in (False, True):
        p = drv.Cholinv(n, bc_mult=-2, serialize=serialize, trsm_mode=True)
        try:
            p.generate()
            p.factor()
            A = p.A()
            check_parity(p, A)
            xs.append(p.solve(reference(A)[0][:, :5])[0])
        finally:
            p.close()
    np.testing.assert_array_equal(xs[0], xs[1])             # Rfull (resident) and the rect structure hold the same R
    p = drv.Cholinv(n, bc_mult=-2, serialize=True, flush_intermediates=True, trsm_mode=True)
    try:
        p.generate()
        p.factor()
        with pytest.raises(drv.DriverError, match="FlushIntermediates"):
            p.solve(np.ones((n, 1)))
    finally:
        p.close()


def test_solve_refuses_factors_of_the_other_mode(drv):
    """an inverse-mode factor() leaves Rinv filled; after a TRSM-mode factor() it is stale, and a solve in inverse mode must not use it"""
    n = 1024
    p = drv.Cholinv(n, bc_mult=-2)
    try:
        p.generate()
        p.factor()
        B = np.ones((n, 1))
        X0 = p.solve(B)[0]
        assert p.D.capital_cholinv_set_trsm_mode(p.p, 1) == 0
        with pytest.raises(drv.DriverError, match="mode"):
            p.solve(B)
        p.factor()
        np.testing.assert_allclose(p.solve(B)[0], X0, rtol=0, atol=1e-12 * np.abs(X0).max())
        assert p.D.capital_cholinv_set_trsm_mode(p.p, 0) == 0
        with pytest.raises(drv.DriverError, match="mode"):
            p.solve(B)
    finally:
        p.close()


def test_no_access_to_A_without_refinement_and_residual(drv):
    n = 1024
    p = drv.Cholinv(n, bc_mult=-2)
    try:
        p.generate()
        A = p.A()
        rng = np.random.default_rng(1)
        B = np.asfortranarray(A @ rng.integers(-8, 9, (n, 3)).astype(np.float64))
        p.set_A(np.where(np.arange(n)[:, None] > np.arange(n)[None, :], np.nan, A))      # factor() reads the upper triangle only
        p.factor()
        X, res = p.solve(B, refine=0, residual=False)
        assert res is None and np.all(np.isfinite(X))
        Xref = sla.cho_solve(sla.cho_factor(A), B)
        assert np.abs(X - Xref).max() <= 1e-12 * np.abs(Xref).max()
    finally:
        p.close()


def test_refusals(drv):
    n = 256
    p = drv.Cholinv(n)
    try:
        p.generate()
        with pytest.raises(drv.DriverError, match="factor\\(\\) has not run"):
            p.solve(np.ones((n, 2)))
        p.factor()
        with pytest.raises(drv.DriverError):
            p.solve(np.ones((n - 1, 2)))
        # below the Python check: the C entry point refuses r < 1 and null pointers itself, solve() a negative refine
        import ctypes as C
        b = np.ones((n, 2), order="F")
        bp = b.ctypes.data_as(C.POINTER(C.c_double))
        assert p.D.capital_cholinv_solve(p.p, 0, bp, bp, None, 1) != 0
        assert b"r >= 1" in p.D.capital_drv_last_error()
        assert p.D.capital_cholinv_solve(p.p, 2, None, bp, None, 1) != 0
        assert p.D.capital_cholinv_solve(p.p, 2, bp, bp, None, -1) != 0
        assert b"refine >= 0" in p.D.capital_drv_last_error()
        p.set_A(cond.f4_indefinite(n, [100]))
        with pytest.raises(drv.DriverError, match="not positive definite"):
            p.factor()
        with pytest.raises(drv.DriverError, match="factor\\(\\) has not run or did not succeed"):
            p.solve(np.ones((n, 2)))
    finally:
        p.close()


def test_repeated_solves_are_bit_identical_and_leave_the_factors(drv):
    n = 2048
    p = drv.Cholinv(n, bc_mult=-2)
    try:
        p.generate()
        p.factor()
        B = reference(p.A())[0][:, :40]
        before = (p.R(), p.Rinv())
        X1, r1 = p.solve(B)
        X2, r2 = p.solve(B)
        after = (p.R(), p.Rinv())
    finally:
        p.close()
    assert X1.tobytes() == X2.tobytes() and r1.tobytes() == r2.tobytes()
    for b, a in zip(before, after):
        np.testing.assert_array_equal(a, b)
