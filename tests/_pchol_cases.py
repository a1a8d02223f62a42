"""The seeded inputs of the pivoted partial Cholesky tests (tests/_pchol_ref.py is the restatement), each built once and read-only:
  (a) exact rank: A = B B^T, B n x k standard normal with columns scaled by logspace(0, -s, k); tol = 1e-12
  (b) an RBF kernel matrix of 700 random points of the unit square, length scale 0.3: every diagonal entry is 1, so the first pivot is a tie
  (c) SPD of order 2500 (beyond capi_dpstrf's 2048): a graded B B^T + 1e-3 I, capped at 130 columns
  (d) n = 1, n = 33 with padded leading dimensions, and the zero matrix"""
import functools

import numpy as np

import _pchol_ref as pref

EXACT = ((300, 40, 3), (1100, 70, 2))
EXACT_TOL = 1e-12


def _frozen(A):
    A = np.asfortranarray(A)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def exact_rank(n, k, s):
    rng = np.random.default_rng(1000 + n + k)
    B = rng.standard_normal((n, k)) * np.logspace(0, -s, k)
    return _frozen(B @ B.T)


@functools.lru_cache(maxsize=None)
def rbf(n=700, scale=0.3):
    X = np.random.default_rng(77).random((n, 2))
    D2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    return _frozen(np.exp(-D2 / (2.0 * scale * scale)))


@functools.lru_cache(maxsize=None)
def spd(n=2500, k=200):
    rng = np.random.default_rng(2500)
    B = rng.standard_normal((n, k)) * np.logspace(0, -2, k)
    return _frozen(B @ B.T + 1e-3 * np.eye(n))


@functools.lru_cache(maxsize=None)
def zero(n=17):
    return _frozen(np.zeros((n, n)))


@functools.lru_cache(maxsize=None)
def one():
    return _frozen(np.array([[4.0]]))


# name -> (matrix, tol (< 0: LAPACK's default), max_rank (None: n), lda, ldl (None: n))
CASES = {
    "exact300": (lambda: exact_rank(*EXACT[0]), EXACT_TOL, None, None, None),
    "exact1100": (lambda: exact_rank(*EXACT[1]), EXACT_TOL, None, None, None),
    "rbf700": (rbf, -1.0, None, None, None),
    "rbf700cap33": (rbf, -1.0, 33, None, None),
    "spd2500cap130": (spd, -1.0, 130, None, None),
    "one": (one, -1.0, None, None, None),
    "pad33": (lambda: exact_rank(33, 9, 1), EXACT_TOL, None, 36, 40),
    "zero": (zero, -1.0, None, None, None),
}
EXACT_CASES = {"exact300": 40, "exact1100": 70}
CAPPED_CASES = {"rbf700cap33": 33, "spd2500cap130": 130}


def case(name):
    """(A, tol, max_rank, lda, ldl) with the defaults filled in"""
    make, tol, kmax, lda, ldl = CASES[name]
    A = make()
    n = A.shape[0]
    return A, tol, kmax or n, lda or n, ldl or n


@functools.lru_cache(maxsize=None)
def restatement(name):
    """dict(L, piv, d, rank, resid_trace, thresh, res): the restatement on the case, and its two residuals, computed once"""
    A, tol, kmax, _, _ = case(name)
    L, piv, d, rank, tr, thresh = pref.pchol(A, tol, kmax)
    for a in (L, piv, d):
        a.setflags(write=False)
    return {"L": L, "piv": piv, "d": d, "rank": rank, "resid_trace": tr, "thresh": thresh, "res": pref.residuals(A, L, piv, rank, d)}
