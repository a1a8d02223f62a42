"""Shifted CholeskyQR in numpy / scipy fp64: the reference that tests/test_gpu_shifted_cqr.py and tests/test_shifted_cqr_host.py
compare qr::cacqr's shifted sweeps with (capital_amd/src/alg/qr/cacqr/cacqr.h), and the seeded ill-conditioned panels both use.

One sweep: G = A^T A; a shifted sweep equilibrates it by powers of two taken from the exponents of its diagonal (frexp),
G' = D^-1 G D^-1, adds s = shift_scale * 11 (m n + n (n + 1)) u trace(G') to the diagonal, factors G' + s I = R'^T R' and takes
R = R' D; a plain sweep factors G itself.  Q = A R^-1, and R = R_k .. R_2 R_1 over the sweeps."""
import numpy as np
import scipy.linalg as sla

U64 = 2.0 ** -53


def equilibrate_shift(G, m_global, shift_scale=1.0):
    """(G' + s I, d, s, trace(G'), info) from the upper triangle of G; info = j + 1 of the first diagonal entry that is zero, negative
    or not finite (0: none) -- such a column stays unscaled and outside the trace."""
    n = G.shape[0]
    g = np.diag(G).copy()
    bad = ~(g > 0.0) | np.isinf(g)
    info = int(np.argmax(bad)) + 1 if bad.any() else 0
    _, ex = np.frexp(np.where(bad, 1.0, g))                     # g = f 2^ex, f in [0.5, 1)
    e = np.floor_divide(ex.astype(np.int64), 2)
    e[bad] = 0
    d = np.ldexp(1.0, e)
    Gp = np.ldexp(np.triu(G), -(e[:, None] + e[None, :]))
    tr = float(np.sum(np.diag(Gp)[~bad]))
    s = (shift_scale * (11.0 * (float(m_global) * n + float(n) * (n + 1)) * U64)) * tr
    Gp[np.diag_indices(n)] += s
    return Gp, d, s, tr, info


def tri_rescale(Rp, Xp, d):
    """(R' D, D^-1 R'^-1, ||R'||_1 ||R'||_inf, ||R'^-1||_1 ||R'^-1||_inf)"""
    e = np.frexp(d)[1] - 1
    a, b = np.abs(np.triu(Rp)), np.abs(np.triu(Xp))
    return (np.ldexp(Rp, e[None, :]), np.ldexp(Xp, -e[:, None]), float(a.sum(axis=0).max() * a.sum(axis=1).max()),
            float(b.sum(axis=0).max() * b.sum(axis=1).max()))


def sweep(A, shifted, m_global=None, shift_scale=1.0):
    """one sweep: (Q, R, stats); numpy.linalg.LinAlgError when the (shifted) Gram matrix does not factor"""
    m, n = A.shape
    G = A.T @ A
    d, s, tr = np.ones(n), 0.0, 0.0
    if shifted:
        G, d, s, tr, info = equilibrate_shift(G, m if m_global is None else m_global, shift_scale)
        if info:
            raise np.linalg.LinAlgError(f"diagonal entry {info} of the Gram matrix is not a positive finite number")
    Rp = sla.cholesky(np.triu(G), lower=False)
    Xp = sla.solve_triangular(Rp, np.eye(n), lower=False)
    R, X, nr, nx = tri_rescale(Rp, Xp, d)
    Q = sla.solve_triangular(R, A.T, trans="T", lower=False).T   # Q = A R^-1
    return np.asfortranarray(Q), R, {"shift": s, "trace": tr, "cond_bound": nr * nx}


def scqr(A, num_iter, num_shifted, shift_scale=1.0):
    """(Q, R, [stats per sweep]): num_iter sweeps of which the first num_shifted are shifted"""
    Q, R, stats = np.asarray(A, dtype=np.float64), None, []
    for k in range(num_iter):
        Q, Rk, st = sweep(Q, k < num_shifted, A.shape[0], shift_scale)
        R = Rk if R is None else np.triu(Rk @ R)
        stats.append(st)
    return Q, np.asfortranarray(R), stats


def grading_exponents(n, seed, lo=-40, hi=40):
    return np.random.default_rng(seed).integers(lo, hi + 1, n)


def panel(m, n, kappa, seed=0, graded=False):
    """A = U diag(sigma) V^T (m x n, Fortran order), sigma log-spaced 1 .. 1/kappa, U and V orthonormal from QR of seeded Gaussians;
    graded: its columns times seeded powers of two in 2^-40 .. 2^40"""
    rng = np.random.default_rng(seed)
    Uq, _ = np.linalg.qr(rng.standard_normal((m, n)))
    Vq, _ = np.linalg.qr(rng.standard_normal((n, n)))
    sig = np.logspace(0, -np.log10(kappa), n) if n > 1 else np.ones(1)
    A = (Uq * sig[None, :]) @ Vq.T
    if graded:
        A = np.ldexp(A, grading_exponents(n, seed + 1)[None, :])
    return np.asfortranarray(A)
