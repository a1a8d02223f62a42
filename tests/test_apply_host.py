"""CPU: the numpy restatements of tests/_apply_ref.py against scipy on _conditioning.f1_spectrum matrices (kappa(A) = 1.5, 1e4, 1e8, so
kappa_2(R) = sqrt(kappa(A))), before the GPU tests take their references from them.

The two solve forms ("subst", "trsm") are backward stable: their eta is held to the project's rule eta <= 10 max(eta_scipy, u), eta_scipy from
scipy.linalg.solve_triangular.  The two forms that multiply by an explicit inverse are not backward stable in general; they are held to the forward
bound instead.  With kappa = kappa_2(R): solve_triangular's y and the product's y each lie within about n u kappa ||y|| of the exact solution
(Higham, Accuracy and Stability, Thm 8.5 for the solve; the computed inverse carries a relative error of n u kappa and the product adds n u |R^-1||b|), so
they differ by at most 2 n u kappa ||y||; the tests allow 4 n u kappa.  diag(A^-1): each route squares entries of an inverse that is within n u kappa of
R^-1 normwise, so two routes differ by at most 2 (2 n u kappa) max_i d_i; the tests allow 4 n u kappa relative to max d."""
import numpy as np
import pytest
import scipy.linalg as sla

import _apply_ref as ref
import _conditioning as cond

U64 = 2.0 ** -53
N, H1 = 512, 256
KAPPAS = [1.5, 1e4, 1e8]
_CACHE = {}


def problem(kappa):
    if kappa not in _CACHE:
        A = cond.f1_spectrum(N, kappa)
        R = ref.chol_upper(A)
        B = np.asfortranarray(np.random.default_rng(7).standard_normal((N, 5)))
        _CACHE[kappa] = (A, R, B, np.linalg.norm(R, 2), np.linalg.cond(R, 2))
    return _CACHE[kappa]


@pytest.mark.parametrize("kappa", KAPPAS)
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("form", ref.FORMS)
def test_half_solves_against_solve_triangular(form, trans, kappa):
    A, R, B, normR, kR = problem(kappa)
    Ys = sla.solve_triangular(R, B, trans="T" if trans else "N")
    Y = ref.half(R, B, trans, form, h1=H1)
    if form in ("subst", "trsm"):
        e, es = ref.eta_half(R, normR, B, Y, trans), ref.eta_half(R, normR, B, Ys, trans)
        print(f"{form} trans={trans} kappa={kappa:.0e}: eta {e:.2e} (solve_triangular {es:.2e})")
        assert e <= 10 * max(es, U64)
    else:
        d = np.linalg.norm(Y - Ys, axis=0) / np.linalg.norm(Ys, axis=0)
        print(f"{form} trans={trans} kappa={kappa:.0e}: |y - solve_triangular| / |y| = {d.max():.2e}, bound {4 * N * U64 * kR:.2e}")
        assert d.max() <= 4 * N * U64 * kR


@pytest.mark.parametrize("kappa", KAPPAS)
@pytest.mark.parametrize("form", ref.FORMS)
def test_two_halves_make_cho_solve(form, kappa):
    """R^-1 (R^-T B) against cho_solve: both within n u kappa(A) of A^-1 B, kappa(A) = kappa_2(R)^2"""
    A, R, B, normR, kR = problem(kappa)
    X = ref.half(R, ref.half(R, B, 1, form, h1=H1), 0, form, h1=H1)
    Xs = sla.cho_solve(sla.cho_factor(A), B)
    d = np.linalg.norm(X - Xs, axis=0) / np.linalg.norm(Xs, axis=0)
    assert d.max() <= 4 * N * U64 * kR * kR


@pytest.mark.parametrize("kappa", KAPPAS)
def test_block_form_of_the_inverse_diagonal(kappa):
    A, R, B, normR, kR = problem(kappa)
    dc, db = ref.inverse_diagonal(R), ref.inverse_diagonal(R, H1)
    ds = np.diag(sla.cho_solve(sla.cho_factor(A), np.eye(N)))
    tol = 4 * N * U64 * kR * ds.max()
    print(f"diag(A^-1) kappa={kappa:.0e}: block - complete {np.abs(db - dc).max() / ds.max():.2e}, complete - cho_solve {np.abs(dc - ds).max() / ds.max():.2e}")
    assert np.abs(db - dc).max() <= tol and np.abs(dc - ds).max() <= tol and np.abs(db - ds).max() <= tol
    assert np.all(db > 0)


def test_block_form_equals_complete_form_in_exact_arithmetic():
    """integer-valued unit-diagonal R: every inverse and product is an integer below 2^53, so the two routes must agree exactly"""
    rng = np.random.default_rng(3)
    n, h1 = 12, 5
    R = np.triu(rng.integers(-1, 2, (n, n)).astype(np.float64), 1) + np.eye(n)
    np.testing.assert_array_equal(ref.inverse_diagonal(R, h1), ref.inverse_diagonal(R))
    B = rng.integers(-4, 5, (n, 3)).astype(np.float64)
    for trans in (0, 1):
        want = ref.half(R, B, trans, "complete")
        for form in ("subst", "trsm", "block"):
            np.testing.assert_array_equal(ref.half(R, B, trans, form, h1=h1), want)
