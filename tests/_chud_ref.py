"""NumPy restatement of the step formulas of capi_dchud / capi_dchud_inv (capital_amd/csrc/chud_f64.hip), and what the tests of the update share:
inputs, the two error figures and their bounds.

Step k (sg = +1 update, -1 downdate) has alpha = T_kk and x = the current row k of V:
    beta = sqrt(alpha^2 + sg ||x||^2), not positive definite unless alpha^2 + sg ||x||^2 > 0 (a NaN compares false)
    for every column j >= k:  t = (alpha T_kj + sg x^T v_j) / beta,  v_j <- v_j - x (T_kj + t) / (alpha + beta),  T_kj <- t
The inverse takes the same step on the pairs (Tinv_ck, e_c), c <= k, with e_c an r-vector that starts at zero."""
import numpy as np
import scipy.linalg as sla

import _conditioning as cond

U64 = cond.U64


def chud(T, V, sign):
    """(T', log, info): T upper triangular n x n, V n x r.  log[k] = (x_k (r), alpha_k, beta_k).  info = 0, or the 1-based step that failed
    (T' is then unspecified from that row down).  Nothing below T's diagonal is read or written."""
    T = np.array(T, dtype=np.float64, order="F")
    V = np.array(V, dtype=np.float64, order="C")
    n, r = V.shape
    sg = float(sign)
    log = np.zeros((n, r + 2))
    for k in range(n):
        alpha, x = T[k, k], V[k].copy()
        d = alpha * alpha + sg * (x @ x)
        if not d > 0.0:
            return T, log, k + 1
        beta = np.sqrt(d)
        log[k, :r], log[k, r], log[k, r + 1] = x, alpha, beta
        row = T[k, k:].copy()
        t = (alpha * row + sg * (V[k:] @ x)) / beta
        V[k:] -= np.outer((row + t) / (alpha + beta), x)
        T[k, k:] = t
    return T, log, 0


def chud_inv(Tinv, log, sign, k0=0, k1=None):
    """the logged steps [k0, k1) on the rows of Tinv that belong to the diagonal sub-triangle [k0, k1); nothing else is read or written"""
    Tinv = np.array(Tinv, dtype=np.float64, order="F")
    n, r = log.shape[0], log.shape[1] - 2
    k1 = n if k1 is None else k1
    sg = float(sign)
    E = np.zeros((n, r))
    for k in range(k0, k1):
        x, alpha, beta = log[k, :r], log[k, r], log[k, r + 1]
        col = Tinv[k0:k + 1, k].copy()
        t = (alpha * col + sg * (E[k0:k + 1] @ x)) / beta
        E[k0:k + 1] -= np.outer((col + t) / (alpha + beta), x)
        Tinv[k0:k + 1, k] = t
    return Tinv


# ---- inputs and criteria shared by test_chud_host.py and the GPU tests ----
def problem(n, r, sign, kappa=1e4, seed=0):
    """(A0, V, A1): S = f1_spectrum(n, kappa) and a Gaussian V with trace(V V^T) about a quarter of trace(S) -- a change of the order of the matrix
    itself, spread over r directions.  Update: A0 = S, A1 = S + V V^T.  Downdate: A0 = S + V V^T, A1 = S, so that the result is positive definite by
    construction and as ill-conditioned as S."""
    rng = np.random.default_rng(1000 * n + 10 * r + (sign > 0) + seed)
    S = cond.f1_spectrum(n, kappa, seed=seed + 1)
    V = rng.standard_normal((n, r)) * (0.5 * np.sqrt(np.trace(S) / n / r))
    if sign > 0:
        A0 = S
        A1 = cond.symmetrize(S + V @ V.T)
    else:
        A1 = S
        A0 = cond.symmetrize(S + V @ V.T)
    return np.asfortranarray(A0), np.asfortranarray(V), np.asfortranarray(A1)


def chol_upper(A):
    return np.triu(sla.cholesky(A, lower=False))


def tri_inv(R):
    return sla.solve_triangular(R, np.eye(R.shape[0]), lower=False)


def factor_error(R1, A0, A1):
    """rho = ||R'^T R' - A1||_F / ||A_big||_F, A_big the one of A0, A1 with the larger norm"""
    big = max(np.linalg.norm(A0), np.linalg.norm(A1))
    return np.linalg.norm(R1.T @ R1 - A1) / big


def factor_bound(A0, A1):
    """32 max(rho_ref, u), rho_ref the same figure for scipy.linalg.cholesky(A1)"""
    return 32 * max(factor_error(chol_upper(A1), A0, A1), U64)


def inverse_error(Ri, R):
    return np.linalg.norm(Ri @ R - np.eye(R.shape[0]))


def inverse_bound(A0, A1):
    """16 max(eps0, eps1, n u), eps_i = ||inv(R_i) R_i - I||_F for SciPy's Cholesky factor and solve_triangular inverse of A_i"""
    n = A0.shape[0]
    eps = [inverse_error(tri_inv(R), R) for R in (chol_upper(A0), chol_upper(A1))]
    return 16 * max(eps[0], eps[1], n * U64)


def failing_v(A, scale=1.001):
    """V (n x 1) = scale sqrt(lambda_max) q_max: A - V V^T has the eigenvalue (1 - scale^2) lambda_max < 0"""
    w, Q = np.linalg.eigh(A)
    return np.asfortranarray(scale * np.sqrt(w[-1]) * Q[:, -1:])
