"""Least-squares problems with a planted solution for qr::cacqr::least_squares (tests/test_gpu_lstsq.py, tests/test_lstsq_host.py and the
rank programs): the seeded ill-conditioned panels of tests/_scqr_ref.py, a right-hand side B = A x_true + w with w orthogonal to range(A)
and ||w_j|| = rho, and the two fp64 references the GPU is measured against.

w is projected off the panel's OWN left basis Uq (the first draw of _scqr_ref.panel, re-derived from the same stream), NOT off numpy's
Householder Q of A: that would hand Householder a right-hand side whose Q^T w is zero to the last bit and make it look orders of magnitude
better than any other backward-stable solver.  A problem with residual rho is conditioned like kappa + kappa^2 rho / (||A|| ||x||) (Wedin),
so rho = 1 is only meaningful at small kappa.

The rule: eta_gpu <= 10 max(eta_householder, eta_scqr, u), eta(X) = max_j ||x_j - x_true_j|| / ||x_true_j||."""
import numpy as np
import scipy.linalg as sla

import _scqr_ref as ref
from _scqr_ref import U64

LD = np.longdouble
CB = 10.0

# (m, n, r, kappa, sweeps, shifted, rho)
CASES = [(1 << 14, 256, 4, 1e1, 2, 0, 0.0), (1 << 14, 256, 4, 1e4, 2, 0, 1.0), (1 << 14, 256, 32, 1e7, 2, 0, 1e-3), (1 << 14, 256, 32, 1e7, 2, 0, 0.0),
         (1 << 16, 256, 1, 1e4, 2, 0, 1.0), (8192, 130, 5, 1e4, 2, 0, 1.0), (1 << 14, 1024, 3, 1e4, 2, 0, 1.0), (1 << 14, 256, 4, 1e10, 3, 1, 0.0),
         (1 << 14, 256, 4, 1e10, 3, 1, 1e-8), (1 << 14, 256, 4, 1e12, 4, 2, 0.0), (1 << 14, 256, 40, 1e4, 2, 0, 1.0)]
IDS = [f"{m}x{n}-r{r}-k{k:.0e}-{it}_{sh}-rho{rho:g}" for m, n, r, k, it, sh, rho in CASES]
SEED = 1


def problem(m, n, r, kappa, rho, seed=SEED):
    """(A, B, x_true): A = _scqr_ref.panel(m, n, kappa, seed), B = fl(A x_true + w), the product in long double"""
    A = ref.panel(m, n, kappa, seed)
    Uq, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((m, n)))      # the panel's left basis: the first draw of panel()
    rng = np.random.default_rng(seed + 100)
    x_true = rng.standard_normal((n, r))
    w = rng.standard_normal((m, r))
    for _ in range(2):
        w -= Uq @ (Uq.T @ w)
    w *= rho / np.linalg.norm(w, axis=0)
    B = (A.astype(LD) @ x_true.astype(LD) + w.astype(LD)).astype(np.float64)
    return A, np.asfortranarray(B), x_true


def eta(X, x_true):
    return float(np.max(np.linalg.norm(X - x_true, axis=0) / np.linalg.norm(x_true, axis=0)))


def solve_householder(A, B):
    Q, R = np.linalg.qr(A)
    return sla.solve_triangular(R, Q.T @ B, lower=False)


def solve_scqr(A, B, sweeps, shifted):
    Q, R, _ = ref.scqr(A, sweeps, shifted)
    return sla.solve_triangular(R, Q.T @ B, lower=False)


def reference_etas(A, B, x_true, sweeps, shifted):
    """(eta of Householder QR + triangular solve, eta of the numpy restatement of the sweeps + triangular solve)"""
    return eta(solve_householder(A, B), x_true), eta(solve_scqr(A, B, sweeps, shifted), x_true)


def gamma(k):
    return k * U64 / (1.0 - k * U64)


def residual_check(A, B, X, resnorms):
    """resnorms[j] against the long-double ||b_j - A x_j||_2 within gamma_(n+2) || |b_j| + |A| |x_j| ||_2; returns (errors, bounds)"""
    true = np.linalg.norm(B.astype(LD) - A.astype(LD) @ X.astype(LD), axis=0).astype(np.float64)
    bound = gamma(A.shape[1] + 2) * np.linalg.norm(np.abs(B) + np.abs(A) @ np.abs(X), axis=0)
    return np.abs(resnorms - true), bound
