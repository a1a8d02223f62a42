"""Seeded input families for the conditioning tests (tests/test_gpu_conditioning.py, tests/test_oracle_ld_validators.py).

Every matrix is numpy float64 in Fortran (column-major) order unless the name says `device`.
  F1  spectrum:      A = Q diag(lambda) Q^T, lambda log-spaced 1 .. 1/kappa (numpy up to order 2048; on the device above that)
  F2  graded:        D B D with D = diag(2^e): exact scaling, R(DBD) = R(B) D and X(DBD) = D^-1 X(B)
  F3  exact factor:  R* upper, small-integer entries, graded power-of-two diagonal, A = R*^T R* exact in fp64
  F4  indefinite:    A = R*^T diag(1, .., -1, .., 1) R*: the first failing pivot is exactly k + 1 (1-based)
  F5  Kahan-type:    T = I - (strictly upper ones), column-scaled by powers of two; T^-1 known in closed form
"""
import numpy as np

U64 = 2.0 ** -53          # unit roundoff of fp64


def orthogonal(n, rng):
    """Haar-distributed orthogonal matrix (QR of a Gaussian, signs fixed)."""
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))[None, :]


def symmetrize(A):
    """exactly symmetric: the upper triangle mirrored"""
    U = np.triu(A)
    return np.asfortranarray(U + np.triu(U, 1).T)


def f1_spectrum(n, kappa, seed=0):
    """F1: SPD of order n <= 2048 with eigenvalues log-spaced from 1 to 1/kappa."""
    rng = np.random.default_rng(seed)
    Q = orthogonal(n, rng)
    lam = np.logspace(0, -np.log10(kappa), n) if n > 1 else np.ones(1)
    return symmetrize((Q * lam[None, :]) @ Q.T)


def f1_device(n, kappa, seed=0):
    """F1 above order 2048, built on the device in torch fp64: A = R0^T R0 with R0 = D (I + N), D log-spaced from 1 to
    kappa^-1/2 and N strictly upper, small Gaussian.  Returns (A as a column-major numpy array, the kappa reached)."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    d = torch.logspace(0, -0.5 * np.log10(kappa), n, dtype=torch.float64, device="cuda")
    N = torch.triu(torch.randn(n, n, dtype=torch.float64, device="cuda", generator=g), 1) * (0.1 / np.sqrt(n))
    R0 = d[:, None] * (torch.eye(n, dtype=torch.float64, device="cuda") + N)
    A = R0.T @ R0
    A = torch.triu(A) + torch.triu(A, 1).T
    ev = torch.linalg.eigvalsh(A)
    reached = (ev[-1] / ev[0]).item()
    # torch is row-major: A is symmetric, so its storage read column-major is the same matrix
    return np.asfortranarray(A.cpu().numpy()), reached


def f2_graded(B, e):
    """F2: D B D with D = diag(2^e) (exact)."""
    e = np.asarray(e, dtype=np.int64)
    return np.asfortranarray(np.ldexp(np.ldexp(B, e[:, None]), e[None, :]))


def f2_exponents(n, seed=0, ramp=False, lo=-200, hi=200):
    """random power-of-two exponents in [lo, hi], or a monotone ramp over that range"""
    if ramp:
        return np.round(np.linspace(lo, hi, n)).astype(np.int64)
    return np.random.default_rng(seed).integers(lo, hi + 1, n)


def f3_exact(n, seed=0, emin=8, emax=20):
    """F3: (A, R*) with R* upper triangular, diagonal 2^e_i (e_i in [emin, emax]), off-diagonal integers of row i in
    [-2^(e_i - 8), 2^(e_i - 8)].  Every entry of A = R*^T R* is an integer below 2^53 and so is exact in fp64
    (kappa(R*) is about 2^(emax - emin))."""
    rng = np.random.default_rng(seed)
    e = rng.integers(emin, emax + 1, n)
    lim = 2 ** np.maximum(e - 8, 0)
    R = np.triu(np.floor(rng.random((n, n)) * (2 * lim[:, None] + 1)) - lim[:, None], 1)
    R += np.diag(np.ldexp(1.0, e))
    R = np.asfortranarray(R)
    A = R.T @ R                                     # integer partial sums below 2^53: exact in any summation order
    assert np.abs(A).max() < 2.0 ** 53
    return symmetrize(A), R


def f4_factor(n, ks, seed=0):
    """(R*, s) of F4: an F3 factor whose column k (each k in ks) has R*_kk = 1, an entry 2 above it and row k off-diagonal entries
    in {-1, 0, 1}; s = diag(S) with -1 at each k."""
    _, R = f3_exact(n, seed, emin=8, emax=14)
    R = R.copy(order="F")
    rng = np.random.default_rng(seed + 1)
    s = np.ones(n)
    for k in ks:
        R[k, k + 1:] = rng.integers(-1, 2, n - k - 1)
        R[k, k] = 1.0
        if k > 0:
            R[k - 1, k] = 2.0
        s[k] = -1.0
    return R, s


def f4_indefinite(n, ks, seed=0):
    """F4: A = R*^T S R* (f4_factor).  The leading minors are positive up to the first k; pivot k + 1 (1-based) is exactly -1 in
    exact arithmetic, while every diagonal entry of A but A_00 (k = 0) is positive.  Every entry is an integer below 2^53."""
    R, s = f4_factor(n, ks, seed)
    A = R.T @ (s[:, None] * R)
    assert np.abs(A).max() < 2.0 ** 53
    A = symmetrize(A)
    if min(ks) > 0:
        assert (np.diag(A) > 0).all()
    return A


def f5_kahan(n, uplo=1, scale_seed=None):
    """F5: T = I - (strictly upper ones) (uplo = 1) or its transpose, optionally with power-of-two column scalings C
    (T C, exponents in [-8, 8]).  Returns (T, X*) with X* = T^-1 exact: (I - N)^-1 has entries 2^(j - i - 1) above the
    diagonal, and (T C)^-1 = C^-1 T^-1."""
    i, j = np.indices((n, n))
    T = np.eye(n) - (j > i)
    X = np.where(j > i, np.ldexp(1.0, np.maximum(j - i - 1, 0)), 0.0) + np.eye(n)
    if scale_seed is not None:
        c = np.random.default_rng(scale_seed).integers(-8, 9, n)
        T = np.ldexp(T, c[None, :])
        X = np.ldexp(X, -c[:, None])
    if uplo == 0:
        T, X = T.T, X.T
    return np.asfortranarray(T), np.asfortranarray(X)


def kappa_tri(R, X=None):
    """Frobenius-norm condition number ||R||_F ||R^-1||_F of a triangle (an upper bound on the 2-norm one)"""
    if X is None:
        X = np.linalg.inv(R)
    return np.linalg.norm(R) * np.linalg.norm(X)

