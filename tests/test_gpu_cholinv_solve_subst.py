"""cholesky::cholinv::solve by SUBSTITUTION (info::solve_by_substitution, Cholinv(..., substitution=True)): a copy and two capi_dtrsm_thin calls on the
resident R, packed or rect, in both factor modes.  No inverse takes part: Rinv is not touched in inverse mode, and in TRSM mode no full-storage
image of R is needed, so Serialize + FlushIntermediates solves.

Parity: test_gpu_cholinv_solve.check_parity's criteria (X against cho_solve to 1e-12, the residual norms, r = 1, 5, 40) on its shared reference.
Conditioning, the numerical claim: with refine = 0 the normwise backward error (test_gpu_cholinv_solve.eta, numpy.longdouble) obeys
eta <= 10 max(eta(cho_solve), u) up to kappa = 1e12, in both modes -- substitution is backward stable where products with an explicit inverse
are only conditionally so (their refine = 0 value is printed beside it)."""
import itertools

import numpy as np
import pytest
import scipy.linalg as sla

import _conditioning as cond
from test_gpu_cholinv_solve import U64, check_parity, eta, reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def drv():
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    yield driver
    driver.finalize()


def factored(drv, n, A=None, **kw):
    p = drv.Cholinv(n, **kw)
    try:
        if A is None:
            p.generate()
        else:
            p.set_A(A)
        p.factor()
    except Exception:
        p.close()
        raise
    return p


INVERSE = list(itertools.product((0, 1), (True, False), (True, False)))


@pytest.mark.parametrize("complete_inv,serialize,flush", INVERSE,
                         ids=[f"ci{c}-{'ser' if se else 'noser'}-{'flush' if f else 'save'}" for c, se, f in INVERSE])
def test_inverse_mode_parity(drv, complete_inv, serialize, flush):
    p = factored(drv, 2048, complete_inv=complete_inv, bc_mult=-2, serialize=serialize, flush_intermediates=flush, substitution=True)
    try:
        assert p.stats()["levels"] >= 1
        before = p.Rinv()
        check_parity(p, p.A())
        np.testing.assert_array_equal(p.Rinv(), before)                   # Rinv is not touched
    finally:
        p.close()


@pytest.mark.parametrize("serialize,flush", [(False, False), (True, False), (True, True)], ids=["noser", "ser-save", "ser-flush"])
def test_trsm_mode_parity(drv, serialize, flush):
    """ser-flush: only the packed R is left after factor(); without the flag solve() throws there, with it it solves"""
    p = factored(drv, 2048, bc_mult=-2, serialize=serialize, flush_intermediates=flush, trsm_mode=True, substitution=True)
    try:
        check_parity(p, p.A())
    finally:
        p.close()


@pytest.mark.parametrize("n,bc_mult,trsm", [(1000, -3, False), (1000, -3, True), (512, 0, False), (512, 0, True)])
def test_other_orders(drv, n, bc_mult, trsm):
    """n = 1000: ragged 32-row blocks and a ragged last leaf; n = 512: one leaf at most 512, no product (and factor() does not split either)"""
    p = factored(drv, n, bc_mult=bc_mult, trsm_mode=trsm, substitution=True)
    try:
        assert (p.stats()["levels"] == 0) == (n == 512)
        check_parity(p, p.A())
    finally:
        p.close()


@pytest.mark.parametrize("kappa", [1e2, 1e6, 1e10, 1e12])
def test_backward_error_without_refinement(drv, kappa):
    n = 1000
    A = cond.f1_spectrum(n, kappa)
    B = np.asfortranarray(A @ np.random.default_rng(int(np.log10(kappa))).standard_normal((n, 3)))
    normA2 = np.linalg.norm(A, 2)
    eta_ref = eta(A, normA2, B, sla.cho_solve(sla.cho_factor(A), B))
    for trsm in (False, True):
        p = factored(drv, n, A=A, bc_mult=-2, trsm_mode=trsm, substitution=True)
        try:
            e_sub = eta(A, normA2, B, p.solve(B, refine=0, residual=False)[0])
            e_inv = None
            if not trsm:
                p.set_solve_substitution(False)
                e_inv = eta(A, normA2, B, p.solve(B, refine=0, residual=False)[0])
        finally:
            p.close()
        print(f"solve kappa={kappa:.0e} {'TRSM' if trsm else 'inverse'} mode, refine=0: eta by substitution {e_sub:.2e} (cho_solve {eta_ref:.2e})"
              + (f", by products with R^-1 {e_inv:.2e}" if e_inv is not None else ""))
        assert e_sub <= 10 * max(eta_ref, U64), (e_sub, eta_ref)


def test_flag_off_still_refuses_packed_trsm_mode(drv):
    n = 1024
    p = factored(drv, n, bc_mult=-2, serialize=True, flush_intermediates=True, trsm_mode=True)
    try:
        B = reference_rhs(p, n)
        with pytest.raises(drv.DriverError, match="FlushIntermediates"):
            p.solve(B)
        p.set_solve_substitution(True)                                    # the same factors, no new factor()
        X = p.solve(B)[0]
        Xref = sla.cho_solve(sla.cho_factor(p.A()), B)
        assert np.abs(X - Xref).max() <= 1e-12 * np.abs(Xref).max()
        p.set_solve_substitution(False)
        with pytest.raises(drv.DriverError, match="FlushIntermediates"):
            p.solve(B)
    finally:
        p.close()


def reference_rhs(p, n):
    A = p.A()
    return np.asfortranarray(A @ np.random.default_rng(n).integers(-8, 9, (n, 5)).astype(np.float64))


@pytest.mark.parametrize("trsm", [False, True], ids=["inverse", "trsm"])
def test_switching_between_solves_needs_no_new_factor(drv, trsm):
    n = 2048
    p = factored(drv, n, bc_mult=-2, trsm_mode=trsm)
    try:
        B = reference(p.A())[0][:, :40]
        X_off = p.solve(B)[0]
        p.set_solve_substitution(True)
        X_on = p.solve(B)[0]
        p.set_solve_substitution(False)
        X_off2 = p.solve(B)[0]
    finally:
        p.close()
    assert np.abs(X_on - X_off).max() <= 1e-12 * np.abs(X_off).max()
    assert X_off2.tobytes() == X_off.tobytes()                            # with the flag off nothing has changed
