"""Column-pivoted CholeskyQR in numpy / scipy fp64: the restatement that the tests compare capi_dpstrf (capital_amd/csrc/pstrf_f64.hip) and
qr::cacqr::factor_pivoted (capital_amd/src/alg/qr/cacqr/cacqr.h) with.

pstrf: LAPACK dpstrf's blocked, lazy scheme on the upper triangle, panels of 32 columns, with the stopping rule of capi_dpstrf -- thresh = tol *
trace(G); at step j the FIRST index p of the largest remaining updated diagonal entry; stop unless d_p > thresh (a NaN compares false and stops).
pcqr: G = A^T A; the pivoted factorization with tol = tol_scale max(rtol^2, 11 (m n + n (n + 1)) u); M = P(:, 0:k) R11^-1; Q1 = A M; one plain
CholeskyQR sweep on Q1; R = R2 [R11 R12]."""
import numpy as np
import scipy.linalg as sla

U64 = 2.0 ** -53
NB = 32


def floor_tol(m_global, n):
    """the factor of the shift a shifted sweep would add (tests/_scqr_ref.py): what a dropped column's squared norm is compared with"""
    return 11.0 * (float(m_global) * n + float(n) * (n + 1)) * U64


def pivot_tol(m_global, n, rtol=0.0, tol_scale=1.0):
    return tol_scale * max(rtol * rtol, floor_tol(m_global, n))


def pstrf(G, tol, absolute=False):
    """(R, piv, rank, thresh): rows < rank of R hold the rank x n upper trapezoid, P^T G P = R^T R + diag-block(0, S); piv 0-based, column j of the
    permuted matrix is column piv[j] of G.  Only G's upper triangle is read.  absolute: thresh = tol itself (LAPACK's convention)"""
    n = G.shape[0]
    A = np.triu(np.array(G, dtype=np.float64))
    piv = np.arange(n)
    thresh = tol if absolute else tol * float(np.sum(np.diag(A)))
    for k0 in range(0, n, NB):
        kend = min(k0 + NB, n)
        dg = np.diag(A).copy()
        dots = np.zeros(n)
        for j in range(k0, kend):
            w = dg[j:] - dots[j:]
            w = np.where(np.isnan(w), -np.inf, w)
            p = j + int(np.argmax(w))                      # numpy's argmax returns the first maximum
            if not (w[p - j] > thresh):
                return A, piv, j, thresh
            if p != j:
                A[:j, [j, p]] = A[:j, [p, j]]                                  # the column parts above
                A[j, p + 1:], A[p, p + 1:] = A[p, p + 1:].copy(), A[j, p + 1:].copy()   # the row parts to the right
                A[j, j + 1:p], A[j + 1:p, p] = A[j + 1:p, p].copy(), A[j, j + 1:p].copy()   # the transposed middle piece
                piv[[j, p]] = piv[[p, j]]
                dg[p], dots[p] = dg[j], dots[j]
                A[p, p] = dg[p]
            ajj = np.sqrt(w[p - j])
            A[j, j] = ajj
            if j + 1 < n:
                A[j, j + 1:] = (A[j, j + 1:] - A[k0:j, j] @ A[k0:j, j + 1:]) / ajj
                dots[j + 1:] += A[j, j + 1:] ** 2
        if kend < n:
            S = A[k0:kend, kend:]
            A[kend:, kend:] -= np.triu(S.T @ S)
    return A, piv, n, thresh


def pcqr(A, rtol=0.0, tol_scale=1.0, m_global=None):
    """dict(Q m x k, R k x n, piv, rank, tol, thresh, trace) of the schedule of qr::cacqr::factor_pivoted"""
    m, n = A.shape
    G = A.T @ A
    tol = pivot_tol(m if m_global is None else m_global, n, rtol, tol_scale)
    Rf, piv, k, thresh = pstrf(G, tol)
    out = {"piv": piv, "rank": k, "tol": tol, "thresh": thresh, "trace": float(np.trace(G))}
    if k == 0:
        return out
    R1 = np.triu(Rf[:k])                                                       # [R11 R12]
    X11 = sla.solve_triangular(R1[:, :k], np.eye(k), lower=False)
    M = np.zeros((n, k))
    M[piv[:k]] = np.triu(X11)
    Q1 = A @ M
    R2 = sla.cholesky(np.triu(Q1.T @ Q1), lower=False)
    Q = sla.solve_triangular(R2, Q1.T, trans="T", lower=False).T
    out["Q"], out["R"] = np.asfortranarray(Q), np.asfortranarray(R2 @ R1)
    return out


def metrics(A, Q, R, piv):
    """(||A P - Q R||_F / ||A||_F, ||Q^T Q - I||_F)"""
    return (float(np.linalg.norm(A[:, piv] - Q @ R) / np.linalg.norm(A)), float(np.linalg.norm(Q.T @ Q - np.eye(Q.shape[1]))))


def basic_solution(Q, R, piv, B):
    """X = P [R11^-1 (Q^T B); 0]"""
    k, n = R.shape
    X = np.zeros((n, B.shape[1]))
    X[piv[:k]] = sla.solve_triangular(R[:, :k], Q.T @ B, lower=False)
    return X


def pstrf_checks(G, R, piv, rank):
    """the quantities the device test bounds, from the upper triangle of G and the rank x n trapezoid R:
    (relative residual of rows < rank of triu(P^T G P - R^T R) against ||G||_max, the largest Schur diagonal entry implied by R)"""
    Gs = np.triu(G) + np.triu(G, 1).T
    Gp = Gs[np.ix_(piv, piv)]
    Rk = np.triu(R[:rank])
    E = np.triu(Gp - Rk.T @ Rk)
    res = float(np.abs(E[:rank]).max() / np.abs(np.triu(G)).max()) if rank else 0.0
    schur = np.diag(Gp)[rank:] - np.sum(Rk[:, rank:] ** 2, axis=0)
    return res, (float(schur.max()) if rank < G.shape[0] else -np.inf)
