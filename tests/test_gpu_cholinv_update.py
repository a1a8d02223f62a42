"""cholesky::cholinv::update through driver.Cholinv.update on one GPU: A <- A +- V V^T on the resident factors without a new factorisation, over the
policies that decide which images of the factors are resident (complete_inv x Serialize x FlushIntermediates, TRSM mode, substitution).

Criteria (tests/_chud_ref.py): the factor and inverse bounds of the C-ABI tests on R() and Rinv() -- for complete_inv = 0 each diagonal block of the
inverse against its own block of R', the unformed block unchanged; then test_gpu_cholinv_solve.check_parity's criteria written out locally (X against
cho_solve on A1 to 1e-12 in max-norm, the residual norms against NumPy to 1e-10 of their scale; check_parity itself asserts the unmodified generate()
matrix); A()'s upper triangle against A0 + V V^T; the backward error of a substitution solve; rcond against the true condition number of A1; and the
state after a downdate that leaves the matrix not positive definite."""
import functools
import itertools

import numpy as np
import pytest
import scipy.linalg as sla

import _chud_ref as ref
import _conditioning as cond
from test_gpu_cholinv_solve import U64, eta

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def drv():
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    yield driver
    driver.finalize()


def vfor(A, r, seed):
    """a Gaussian V with trace(V V^T) about a quarter of trace(A)"""
    n = A.shape[0]
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((n, r)) * (0.5 * np.sqrt(np.trace(A) / n / r)))


_GEN = {}


def generated(drv, n):
    """generate()'s matrix of order n (deterministic), fetched once"""
    if n not in _GEN:
        p = drv.Cholinv(n)
        try:
            p.generate()
            _GEN[n] = p.A()
        finally:
            p.close()
        _GEN[n].setflags(write=False)
    return _GEN[n]


_CASE = {}


def case(drv, n, r, sign):
    """(A0, V, A1, B, Xref, ||A1||_F, factor bound, inverse bound): S = generate()'s matrix; update: A0 = S, downdate: A1 = S.  Once per (n, r, sign)"""
    key = (n, r, sign)
    if key not in _CASE:
        S = generated(drv, n)
        V = vfor(S, r, 100 * n + r)
        SV = np.asfortranarray(cond.symmetrize(S + V @ V.T))
        A0, A1 = (S, SV) if sign > 0 else (SV, S)
        X0 = np.random.default_rng(n).integers(-8, 9, (n, 40)).astype(np.float64)
        B = np.asfortranarray(A1 @ X0)
        _CASE[key] = (A0, V, A1, B, sla.cho_solve(sla.cho_factor(A1), B), np.linalg.norm(A1), ref.factor_bound(A0, A1), ref.inverse_bound(A0, A1))
        for a in _CASE[key][:5]:
            a.setflags(write=False)
    return _CASE[key]


def factored(drv, n, A, **kw):
    p = drv.Cholinv(n, **kw)
    try:
        p.set_A(A)
        p.factor()
    except Exception:
        p.close()
        raise
    return p


def check_solves(p, A1, B, Xref, normA, rs=(1, 5, 40)):
    """test_gpu_cholinv_solve.check_parity's two criteria, against the updated matrix"""
    for r in rs:                                           # 40: the loop over blocks of 32 right-hand sides runs twice
        X, res = p.solve(B[:, :r], refine=1)
        err = np.abs(X - Xref[:, :r]).max() / np.abs(Xref[:, :r]).max()
        ref_res = np.linalg.norm(B[:, :r] - A1 @ X, axis=0)
        scale = normA * np.linalg.norm(X, axis=0) + np.linalg.norm(B[:, :r], axis=0)
        rerr = np.max(np.abs(res - ref_res) / scale)
        print(f"solve after update n={A1.shape[0]} r={r}: |X - cho_solve| / max|X| = {err:.2e}, |resnorm - numpy| / scale = {rerr:.2e}")
        assert err <= 1e-12
        assert res.shape == (r,) and rerr <= 1e-10


def check_factors(p, A0, A1, rho_max, eps_max, h1=0, inverse=True, before=None):
    n = A1.shape[0]
    R1 = p.R()
    assert (np.tril(R1, -1) == 0).all() and (np.diag(R1) > 0).all()
    rho = ref.factor_error(R1, A0, A1)
    print(f"update n={n}: rho {rho / U64:.1f} u (bound {rho_max / U64:.1f} u, {rho / (rho_max / 32):.2f} x ref)")
    assert rho <= rho_max
    if not inverse:
        return
    Ri1 = p.Rinv()
    assert (np.tril(Ri1, -1) == 0).all()
    spans = [(0, n)] if h1 == 0 else [(0, h1), (h1, n)]
    for a, b in spans:
        eps = ref.inverse_error(Ri1[a:b, a:b], R1[a:b, a:b])
        print(f"update n={n}: ||Rinv' R' - I|| over [{a}, {b}) {eps:.2e} (bound {eps_max:.2e}, {eps / (eps_max / 16):.2f} x ref)")
        assert eps <= eps_max
    if h1:
        assert Ri1[:h1, h1:].tobytes() == before[:h1, h1:].tobytes()          # the unformed block


def check_A(p, A1):
    got = p.A()
    iu = np.triu_indices(A1.shape[0])
    assert np.abs(got[iu] - A1[iu]).max() <= 4 * U64 * np.linalg.norm(A1)


INVERSE = list(itertools.product((0, 1), (True, False), (True, False)))


@pytest.mark.parametrize("complete_inv,serialize,flush", INVERSE,
                         ids=[f"ci{c}-{'ser' if se else 'noser'}-{'flush' if f else 'save'}" for c, se, f in INVERSE])
def test_inverse_mode_over_policies(drv, complete_inv, serialize, flush):
    n, r = 2048, 5
    A0, V, A1, B, Xref, normA, rho_max, eps_max = case(drv, n, r, 1)
    p = factored(drv, n, A0, complete_inv=complete_inv, bc_mult=-2, serialize=serialize, flush_intermediates=flush)
    try:
        assert p.stats()["levels"] >= 1
        before = p.Rinv()
        p.update(V)
        check_factors(p, A0, A1, rho_max, eps_max, h1=0 if complete_inv else n // 2, before=before)
        check_A(p, A1)
        check_solves(p, A1, B, Xref, normA)
    finally:
        p.close()


@pytest.mark.parametrize("serialize,flush,subst", [(False, False, False), (True, False, False), (True, True, True)], ids=["noser", "ser-save", "ser-flush-subst"])
def test_trsm_mode(drv, serialize, flush, subst):
    """no inverse exists; ser-save solves by capi_dtrsm on the full-storage image, which must have followed; ser-flush has the packed R alone"""
    n, r = 2048, 5
    A0, V, A1, B, Xref, normA, rho_max, eps_max = case(drv, n, r, 1)
    p = factored(drv, n, A0, bc_mult=-2, serialize=serialize, flush_intermediates=flush, trsm_mode=True, substitution=subst)
    try:
        p.update(V)
        check_factors(p, A0, A1, rho_max, eps_max, inverse=False)
        check_A(p, A1)
        check_solves(p, A1, B, Xref, normA)
        if not flush:                                                       # the other form of the solve reads the other image where there are two
            p.set_solve_substitution(True)
            check_solves(p, A1, B, Xref, normA, rs=(5,))
    finally:
        p.close()


@pytest.mark.parametrize("sign", [1, -1], ids=["update", "downdate"])
@pytest.mark.parametrize("n,bc_mult", [(1000, -3), (512, 0)])
def test_other_orders_both_signs(drv, n, bc_mult, sign):
    """n = 1000: ragged panels, a top split at 500; n = 512: factor() does not split, so complete_inv = 0 has a complete inverse all the same"""
    r = 5
    A0, V, A1, B, Xref, normA, rho_max, eps_max = case(drv, n, r, sign)
    p = factored(drv, n, A0, bc_mult=bc_mult)
    try:
        assert (p.stats()["levels"] == 0) == (n == 512)
        before = p.Rinv()
        p.update(V, downdate=sign < 0)
        check_factors(p, A0, A1, rho_max, eps_max, h1=0 if n == 512 else n // 2, before=before)
        check_A(p, A1)
        check_solves(p, A1, B, Xref, normA)
    finally:
        p.close()


@pytest.mark.parametrize("complete_inv", [0, 1])
def test_forty_columns_take_two_blocks(drv, complete_inv):
    n, r = 1000, 40
    A0, V, A1, B, Xref, normA, rho_max, eps_max = case(drv, n, r, 1)
    p = factored(drv, n, A0, complete_inv=complete_inv, bc_mult=-3)
    try:
        before = p.Rinv()
        p.update(V)
        check_factors(p, A0, A1, rho_max, eps_max, h1=0 if complete_inv else n // 2, before=before)
        check_A(p, A1)
        check_solves(p, A1, B, Xref, normA, rs=(5,))
    finally:
        p.close()


def test_update_then_downdate_returns_to_the_matrix(drv):
    n, r = 2048, 5
    A0, V, A1, _, _, _, _, _ = case(drv, n, r, 1)
    B = np.asfortranarray(A0 @ np.random.default_rng(7).integers(-8, 9, (n, 5)).astype(np.float64))
    Xref = sla.cho_solve(sla.cho_factor(A0), B)
    p = factored(drv, n, A0, bc_mult=-2)
    try:
        p.update(V)
        p.update(V, downdate=True)
        X = p.solve(B)[0]
        check_A(p, A0)
    finally:
        p.close()
    assert np.abs(X - Xref).max() <= 1e-12 * np.abs(Xref).max()


@pytest.mark.parametrize("kappa", [1e2, 1e6])
def test_backward_error_by_substitution_without_refinement(drv, kappa):
    """test_gpu_cholinv_solve_subst's criterion on the updated factors"""
    n, r = 1000, 3
    A0 = cond.f1_spectrum(n, kappa)
    V = vfor(A0, r, int(np.log10(kappa)))
    A1 = cond.symmetrize(A0 + V @ V.T)
    B = np.asfortranarray(A1 @ np.random.default_rng(int(np.log10(kappa))).standard_normal((n, 3)))
    normA2 = np.linalg.norm(A1, 2)
    eta_ref = eta(A1, normA2, B, sla.cho_solve(sla.cho_factor(A1), B))
    p = factored(drv, n, A0, bc_mult=-2, substitution=True)
    try:
        p.update(V)
        e = eta(A1, normA2, B, p.solve(B, refine=0, residual=False)[0])
    finally:
        p.close()
    print(f"update kappa={kappa:.0e}: eta by substitution, refine=0, {e:.2e} (cho_solve {eta_ref:.2e})")
    assert e <= 10 * max(eta_ref, U64), (e, eta_ref)


def test_rcond_after_an_update(drv):
    """test_gpu_cholinv_bounds' criterion against the true condition number of A1"""
    n, r = 1000, 5
    A0, V, A1, _, _, _, _, _ = case(drv, n, r, 1)
    rcond_true = 1.0 / (np.linalg.norm(A1, 1) * np.linalg.norm(np.linalg.inv(A1), 1))
    p = factored(drv, n, A0, bc_mult=-3)
    try:
        rc0 = p.rcond()
        p.update(V)
        rc, an, applies = p.rcond(details=True)
    finally:
        p.close()
    print(f"rcond after update: {rc:.4e} = {rc / rcond_true:.3f} rcond_true (before the update {rc0:.4e})")
    assert abs(an - np.linalg.norm(A1, 1)) <= 4 * n * U64 * an
    assert 0.9 <= rc / rcond_true <= 3


@pytest.mark.parametrize("kw", [dict(), dict(serialize=False), dict(trsm_mode=True, substitution=True, flush_intermediates=True)], ids=["ser", "noser", "trsm-flush"])
def test_failed_downdate(drv, kw):
    n = 1000
    A0 = generated(drv, n)
    V = ref.failing_v(A0)
    B = np.asfortranarray(A0 @ np.ones((n, 2)))
    p = factored(drv, n, A0, bc_mult=-3, **kw)
    try:
        with pytest.raises(drv.DriverError, match="not positive definite \\(step"):
            p.update(V, downdate=True)
        assert p.A().tobytes() == np.asfortranarray(A0).tobytes()
        with pytest.raises(drv.DriverError, match="factor\\(\\) has not run or did not succeed"):
            p.solve(B)
        with pytest.raises(drv.DriverError, match="factor\\(\\) has not run or did not succeed"):
            p.update(V)
        p.factor()
        X = p.solve(B)[0]
        assert np.abs(X - 1.0).max() <= 1e-10
        p.update(V)                                                         # the same V as an update is fine
    finally:
        p.close()


def test_arguments(drv):
    n = 512
    p = factored(drv, n, generated(drv, n))
    try:
        with pytest.raises(drv.DriverError, match="V must be"):
            p.update(np.ones((n + 1, 2)))
        q = drv.Cholinv(n)
        try:
            q.generate()
            with pytest.raises(drv.DriverError, match="factor\\(\\) has not run"):
                q.update(np.ones((n, 1)))
        finally:
            q.close()
    finally:
        p.close()
