"""The seeded rank-deficient tall panels of the column-pivoted CholeskyQR tests (tests/test_pcqr_host.py, test_gpu_pstrf.py,
test_gpu_cacqr_pivoted.py) and the references every one of them shares, computed once.

A = panel(m, k, 1e2, seed) @ W: an m x n panel of exact rank k whose nonzero singular values span about 1e2 times the spread of W,
W = standard_normal((k, n)) with its columns scaled by powers of two in 2^-2 .. 2^2; with k == n the panel itself.  The (m, n, k) triples
cover n = one panel of capi_dpstrf (32 columns), the panel edge +- 1, the odd rest, a stop inside the first, a middle and the last
panel, and rank 1."""
import functools

import numpy as np

import _pcqr_ref as pref
import _scqr_ref as ref

CASES = [(2048, 2, 1), (2048, 32, 1), (2048, 32, 32), (2048, 31, 31), (2112, 33, 20), (4160, 65, 40), (4160, 65, 64), (8320, 130, 97), (16448, 257, 200)]
IDS = [f"{m}x{n}-rank{k}" for m, n, k in CASES]
NRHS = 3


def seed_of(m, n, k):
    return n + k


@functools.lru_cache(maxsize=None)
def matrix(m, n, k):
    """the read-only m x n panel of rank k (Fortran order)"""
    seed = seed_of(m, n, k)
    if k == n:
        A = ref.panel(m, n, 1e2, seed)
    else:
        rng = np.random.default_rng(seed)
        W = rng.standard_normal((k, n))
        W = W * (2.0 ** rng.integers(-2, 3, n))[None, :]
        A = np.asfortranarray(ref.panel(m, k, 1e2, seed) @ W)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def gram(m, n, k):
    """G = A^T A as numpy forms it: the bits that both the restatement and the device kernel are given"""
    A = matrix(m, n, k)
    G = np.asfortranarray(A.T @ A)
    G.setflags(write=False)
    return G


@functools.lru_cache(maxsize=None)
def rhs(m, n, k):
    B = np.asfortranarray(np.random.default_rng(seed_of(m, n, k) + 7).standard_normal((m, NRHS)))
    B.setflags(write=False)
    return B


@functools.lru_cache(maxsize=None)
def restatement(m, n, k, rtol=0.0):
    """the numpy restatement of qr::cacqr::factor_pivoted on the case: a dict (see _pcqr_ref.pcqr) with its metrics"""
    A = matrix(m, n, k)
    out = pref.pcqr(A, rtol=rtol)
    out["residual"], out["orthogonality"] = pref.metrics(A, out["Q"], out["R"], out["piv"])
    return out


@functools.lru_cache(maxsize=None)
def qrcp(m, n, k):
    """scipy.linalg.qr(pivoting=True) of the case: (Q, R, P), economic, untruncated"""
    import scipy.linalg as sla
    return sla.qr(matrix(m, n, k), mode="economic", pivoting=True)


def qrcp_metrics(m, n, k, rank):
    """(residual, orthogonality) of scipy's QRCP truncated at `rank`"""
    Q, R, P = qrcp(m, n, k)
    return pref.metrics(matrix(m, n, k), Q[:, :rank], R[:rank], P)


@functools.lru_cache(maxsize=None)
def lstsq_reference(m, n, k):
    """||A x - b||_2 per right-hand side of numpy.linalg.lstsq(A, b, rcond=sqrt(tol))"""
    A, B = matrix(m, n, k), rhs(m, n, k)
    X = np.linalg.lstsq(A, B, rcond=np.sqrt(pref.floor_tol(m, n)))[0]
    return np.linalg.norm(A @ X - B, axis=0)
