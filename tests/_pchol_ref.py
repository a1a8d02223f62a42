"""Diagonally pivoted, partial Cholesky in numpy fp64: the restatement that the tests compare capi_dpchol (capital_amd/csrc/pchol_f64.hip) and
cholesky::cholinv::factor_pivoted with.  Swap-free: L stays in A's row ordering; only A's upper triangle is read.  thresh = tol trace(A), or for
tol < 0 LAPACK dpstrf's default n u max a_ii; at step j the FIRST index p of the largest remaining d_i (a NaN counts as -inf); stop unless d_p > thresh."""
import numpy as np

U64 = 2.0 ** -53


def sym(A):
    """the symmetric matrix that A's upper triangle stands for"""
    return np.triu(A) + np.triu(A, 1).T


def pchol(A, tol, max_rank=None):
    """(L n x rank, piv, d, rank, resid_trace, thresh)"""
    n = A.shape[0]
    kmax = n if max_rank is None else max_rank
    S = sym(A)
    d = np.diag(S).copy()
    thresh = n * U64 * float(np.max(np.where(np.isnan(d), -np.inf, d))) if tol < 0 else tol * float(np.sum(d))
    L = np.zeros((n, kmax), order="F")
    chosen = np.zeros(n, dtype=bool)
    piv = []
    for j in range(kmax):
        w = np.where(chosen | np.isnan(d), -np.inf, d)
        p = int(np.argmax(w))                              # numpy's argmax returns the first maximum
        if not (w[p] > thresh):
            break
        r = np.sqrt(w[p])
        c = (S[:, p] - L[:, :j] @ L[p, :j]) / r
        c[chosen] = 0.0
        c[p] = r
        L[:, j] = c
        chosen[p] = True
        piv.append(p)
        d = d - c * c
        d[p] = 0.0
    rank = len(piv)
    rest = np.flatnonzero(~chosen)
    return L[:, :rank], np.array(piv + rest.tolist(), dtype=np.int64), d, rank, float(np.sum(d[rest])), thresh


def residuals(A, L, piv, rank, d):
    """the two measures the device tests bound: (||(A - L L^T)[chosen, :]||_F / ||A||_F, max over the rows not chosen of |diag(A - L L^T)_i - d_i| / trace)"""
    S = sym(A)
    E = S - L[:, :rank] @ L[:, :rank].T
    rest = piv[rank:]
    r1 = float(np.linalg.norm(E[piv[:rank]]) / np.linalg.norm(S)) if rank else 0.0
    r2 = float(np.max(np.abs(np.diag(E)[rest] - d[rest])) / np.trace(S)) if len(rest) and rank else 0.0
    return r1, r2


def running_diagonal(A, L, rank):
    """d before every step, recomputed from L as the device carries it: d <- fl(d - fl(L(:, l)^2)), l ascending.  (rank + 1) x n"""
    out = np.empty((rank + 1, A.shape[0]))
    out[0] = np.diag(A)
    for l in range(rank):
        out[l + 1] = out[l] - L[:, l] * L[:, l]
    return out
