"""One-sided (Hestenes) Jacobi SVD of an upper triangular R in numpy fp64: the restatement of the steps capi_dgesvj takes
(capital_amd/csrc/svd_f64.hip), vectorised per step, that tests/test_gpu_gesvj.py and tests/test_gpu_cacqr_svd.py compare the GPU with.

The columns of M = R^T are rotated, M J = V Sigma: cyclic sweeps in the round-robin order of capital_amd/csrc/jacobi_plan.h (N = n rounded up
to even, N - 1 steps of up to N / 2 disjoint pairs), a pair rotated when |x^T y| > sqrt(n) 2^-53 ||x|| ||y||, until a sweep rotates nothing
(30 sweeps at the most).  The normalised columns are V, their norms sigma, the accumulated rotations U, polished by one Newton-Schulz step
U <- U (1.5 I - 0.5 U^T U); then a stable descending sort.  R = U diag(sigma) V^T."""
import numpy as np

MAX_SWEEPS = 30


def step_pairs(n, step):
    """the pairs (p < q) of one step, slot by slot; an odd n rests one column (the partner of the phantom column n)"""
    N = n + (n & 1)
    k = np.arange(1, N // 2)
    a = np.concatenate(([N - 1], (step + k) % (N - 1)))
    b = np.concatenate(([step], (step - k) % (N - 1)))
    p, q = np.minimum(a, b), np.maximum(a, b)
    keep = q < n
    return p[keep], q[keep]


def jacobi_svd(R, want_u=True, polish=True):
    """(U or None, sigma, V, sweeps) from the upper triangle of R; sweeps = -30 when the cap was hit"""
    n = R.shape[0]
    W = np.asfortranarray(np.triu(R).T)
    J = np.asfortranarray(np.eye(n)) if want_u else None
    tol = np.sqrt(float(n)) * 2.0 ** -53
    N = n + (n & 1)
    sweeps = 0
    while sweeps < MAX_SWEEPS:
        sweeps += 1
        rotated = 0
        for step in range(N - 1):
            p, q = step_pairs(n, step)
            x, y = W[:, p], W[:, q]
            a, b, c = np.sum(x * x, axis=0), np.sum(y * y, axis=0), np.sum(x * y, axis=0)
            with np.errstate(all="ignore"):
                rot = (np.abs(c) > tol * np.sqrt(a) * np.sqrt(b)) & (a != 0.0) & (b != 0.0)
                zeta = (b - a) / (2.0 * np.where(rot, c, 1.0))
                t = np.where(zeta >= 0.0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
            cs = 1.0 / np.sqrt(1.0 + t * t)
            cs, sn = np.where(rot, cs, 1.0), np.where(rot, cs * t, 0.0)
            W[:, p], W[:, q] = cs * x - sn * y, sn * x + cs * y
            if want_u:
                x, y = J[:, p], J[:, q]
                J[:, p], J[:, q] = cs * x - sn * y, sn * x + cs * y
            rotated += int(rot.sum())
        if rotated == 0:
            break
    else:
        sweeps = -MAX_SWEEPS
    s = np.sqrt(np.sum(W * W, axis=0))
    V = W / np.where(s == 0.0, 1.0, s)[None, :]
    order = np.argsort(-s, kind="stable")
    U = None
    if want_u:
        U = J[:, order]
        if polish:
            U = U @ (1.5 * np.eye(n) - 0.5 * (U.T @ U))
    return U, s[order], np.asfortranarray(V[:, order]), sweeps


def metrics(R, U, s, V, s_ref):
    """(residual, orthogonality of U, orthogonality of V, sigma error / sigma_1) of R = U diag(s) V^T; R may be tall (A itself)"""
    n = V.shape[0]
    Rt = np.triu(R) if R.shape[0] == R.shape[1] else R
    return (np.linalg.norm(Rt - (U * s[None, :]) @ V.T) / np.linalg.norm(Rt), np.linalg.norm(U.T @ U - np.eye(n)),
            np.linalg.norm(V.T @ V - np.eye(n)), float(np.max(np.abs(s - s_ref)) / s_ref[0]))
