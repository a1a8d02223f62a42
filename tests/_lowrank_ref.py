"""M = L L^T + D in numpy: the restatement that the tests compare cholesky::cholinv::lowrank_prepare / lowrank_solve / lowrank_quadratic_forms with, in the
formulas of the host layer (Woodbury's identity on the k x k capacitance matrix C = I + L^T D^-1 L = R_c^T R_c), and the reference they are all measured
against: a Cholesky solve of the dense M in 80-bit longdouble, with its own factorization and substitutions.

  d             = (shift + diag) + schur, in that order
  C             = I + L_s^T L_s, L_s = L * (1 / sqrt(d))        a general d
                = I + (L^T L) / sigma^2                         a uniform d = sigma^2
  M^-1 B        = (B - L T) / d,  T = R_c^-1 R_c^-T (L^T (B / d))
  log det M     = sum log d_i + 2 sum log (R_c)_ii;  S = sum |log d_i| + 2 sum |log (R_c)_ii| is the scale its error is measured in
  b^T M^-1 b    = sum (b / sqrt(d))^2 - ||R_c^-T L^T (b / d)||^2
  ||b - M x||   with M x = L (L^T x) + d x
The form is not backward stable: every error scales with ||C||_1 u (u = 2^-53), which is why prepare() returns it."""
import numpy as np
import scipy.linalg as sl

U64 = 2.0 ** -53


def diag_vector(n, shift, diag=None, schur=None):
    d = np.full(n, float(shift))
    if diag is not None:
        d = d + diag
    if schur is not None:
        d = d + schur
    return d


def prepare(L, d, uniform=False):
    """dict(Rc, C, cnorm1, logdet, S); uniform: d is constant and C is formed from G = L^T L"""
    k = L.shape[1]
    if uniform:
        C = np.eye(k) + (L.T @ L) / d[0]
    else:
        Ls = L * (1.0 / np.sqrt(d))[:, None]
        C = np.eye(k) + Ls.T @ Ls
    Rc = sl.cholesky(C)
    lr = np.log(np.diag(Rc))
    return {"Rc": Rc, "C": C, "cnorm1": float(np.linalg.norm(C, 1)), "logdet": float(np.sum(np.log(d)) + 2.0 * np.sum(lr)),
            "S": float(np.sum(np.abs(np.log(d))) + 2.0 * np.sum(np.abs(lr)))}


def solve(L, d, Rc, B):
    T = L.T @ (B / d[:, None])
    T = sl.solve_triangular(Rc, sl.solve_triangular(Rc, T, trans=1))
    return (B - L @ T) / d[:, None]


def quadratic_forms(L, d, Rc, B):
    """(q, sum b^2 / d)"""
    b2 = np.sum((B * (1.0 / np.sqrt(d))[:, None]) ** 2, axis=0)
    Y = sl.solve_triangular(Rc, L.T @ (B / d[:, None]), trans=1)
    return b2 - np.sum(Y * Y, axis=0), b2


def residual_norms(L, d, B, X):
    return np.linalg.norm(B - (L @ (L.T @ X) + d[:, None] * X), axis=0)


def residual_scale(L, d, B, X):
    """|| |L| (|L|^T |x|) + d |x| + |b| ||_2 per column: what the rounding errors of a residual evaluated in fp64 are proportional to"""
    aL, aX = np.abs(L), np.abs(X)
    return np.linalg.norm(aL @ (aL.T @ aX) + d[:, None] * aX + np.abs(B), axis=0)


# ---- the longdouble reference (n <= 700: seconds) ----
def _chol_ld(M):
    M = M.copy()
    n = M.shape[0]
    R = np.zeros_like(M)
    for j in range(n):
        R[j, j:] = M[j, j:] / np.sqrt(M[j, j])
        M[j + 1:, j + 1:] -= np.outer(R[j, j + 1:], R[j, j + 1:])
    return R


def reference(L, d, B):
    """(X, logdet, q) of M = L L^T + diag(d) by an upper Cholesky factorization and two substitutions in longdouble, rounded to fp64 at the end"""
    Ll = L.astype(np.longdouble)
    M = Ll @ Ll.T + np.diag(d.astype(np.longdouble))
    n = M.shape[0]
    assert n <= 700, "the longdouble reference is O(n^3) in interpreted loops"
    R = _chol_ld(M)
    Y = B.astype(np.longdouble).copy()
    for i in range(n):
        Y[i] = (Y[i] - R[:i, i] @ Y[:i]) / R[i, i]
    q = np.sum(Y * Y, axis=0)
    for i in range(n - 1, -1, -1):
        Y[i] = (Y[i] - R[i, i + 1:] @ Y[i + 1:]) / R[i, i]
    return Y.astype(np.float64), float(2 * np.sum(np.log(np.diag(R)))), q.astype(np.float64)


def column_errors(X, Xref):
    return np.linalg.norm(X - Xref, axis=0) / np.linalg.norm(Xref, axis=0)
