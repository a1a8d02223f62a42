"""CPU: the mathematics of capi_dormqr before any kernel runs.  tests/_ormqr_ref.py's one-reflector-at-a-time dorm2r, and its restatement of the
blocked scheme the kernels follow (panels of 32, T by dlarft's recurrence from G = P^T P), against scipy's LAPACK dormqr on the same image: 1e-13 of
max |C| at (700, 48, r = 5), both trans."""
import numpy as np
import pytest
import scipy.linalg.lapack as lapack

import _ormqr_ref as ref

TOL = 1e-13


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(70048)
    A = np.asfortranarray(rng.random((700, 48)) - 0.5)
    C = np.asfortranarray(rng.standard_normal((700, 5)))
    fac, tau, _, info = lapack.dgeqrf(A)
    assert info == 0
    out = {}
    for trans in ("T", "N"):
        lwork = int(lapack.dormqr("L", trans, fac, tau, C, -1)[1][0])
        cq, _, info = lapack.dormqr("L", trans, fac, tau, C, lwork)
        assert info == 0
        out[trans] = cq
    for a in (fac, tau, C, out["T"], out["N"]):
        a.setflags(write=False)
    return fac, tau, C, out


def _check(what, err, tol):
    print(f"{what}: err/tol {err:.3e}/{tol:.1e} = {err / tol:.3f}")
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize("trans", ["T", "N"])
def test_reflector_by_reflector_is_dormqr(case, trans):
    fac, tau, C, out = case
    got = ref.ormqr(fac, tau, C, trans == "T")
    _check(f"dorm2r {trans}", np.abs(got - out[trans]).max() / np.abs(C).max(), TOL)


@pytest.mark.parametrize("trans", ["T", "N"])
def test_blocked_scheme_is_dormqr(case, trans):
    fac, tau, C, out = case
    got = ref.ormqr_blocked(fac, tau, C, trans == "T")
    _check(f"blocked {trans}", np.abs(got - out[trans]).max() / np.abs(C).max(), TOL)


def test_fewer_reflectors_and_nan_above_the_diagonal(case):
    """k = 20 of 48 against scipy on the first 20 columns; R's place filled with NaN changes no bit of either restatement"""
    fac, tau, C, _ = case
    lwork = int(lapack.dormqr("L", "T", fac[:, :20], tau[:20], C, -1)[1][0])
    want = lapack.dormqr("L", "T", fac[:, :20], tau[:20], C, lwork)[0]
    poisoned = fac.copy(order="F")
    poisoned[np.triu_indices(48, 0, 48)[0], np.triu_indices(48, 0, 48)[1]] = np.nan
    for f in (ref.ormqr, ref.ormqr_blocked):
        got = f(fac, tau, C, True, k=20)
        _check(f"{f.__name__} k=20", np.abs(got - want).max() / np.abs(C).max(), TOL)
        assert np.array_equal(f(poisoned, tau, C, True, k=20), got)
