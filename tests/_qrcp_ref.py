"""numpy restatement of capi_dgeqp3's step rule (include/capital_hip.h) and of the whole capi_dgelsy path, with the case builders the CPU and GPU tests
share (tests/test_qrcp_ref.py, tests/test_gpu_geqp3.py, tests/test_gpu_gelsy.py, tests/test_gpu_gelsy_engine.py).

geqp3 is swap-free as the kernel is: a column stays where it is, sel marks the chosen ones.  Pivot: the FIRST index of the largest running norm among
the columns not chosen (a NaN entered as -inf); nu recomputed from the column; stop unless nu > rtol nu_0 and nu > 0; dlarfg's reflector without
rescaling (tau = 0, beta = alpha when nothing lies below alpha); dlaqp2's two-vector downdate with tol3z = sqrt(2^-53).  Sums are numpy's, not the
kernel's fixed orders: the two agree to rounding, so a comparison needs inputs whose pivot choice and stop do not hang on the last bits -- `gaps`
(runner-up / pivot running norm per step) is what the case builders assert on."""
import functools

import numpy as np
import scipy.linalg as sla

U64 = 2.0 ** -53
TOL3Z = np.sqrt(2.0 ** -53)
GAP = 1.0 - 1e-6


def geqp3(W, rtol):
    """(image, tau, jpvt, k, gaps): the LAPACK image of W P = Q R (mr x n), tau (min(mr, n)), jpvt (n, 0-based, a permutation), the rank"""
    W = np.array(W, dtype=np.float64, order="F")
    mr, n = W.shape
    kmin = min(mr, n)
    if rtol < 0:
        rtol = max(mr, n) * 2.0 ** -52
    out = np.zeros((mr, n), order="F")
    tau = np.zeros(kmin)
    sel = np.full(n, -1)
    vn1 = np.sqrt((W * W).sum(axis=0))
    vn2 = vn1.copy()
    chosen, gaps = [], []
    k, nu0 = kmin, 0.0
    for j in range(kmin):
        free = np.flatnonzero(sel < 0)
        key = np.where(np.isnan(vn1[free]), -np.inf, vn1[free])
        p = int(free[np.argmax(key)])                                    # argmax: the first of the largest
        top = np.sort(key)[::-1]
        gaps.append(float(top[1] / top[0]) if len(top) > 1 and top[0] > 0 else 0.0)
        x = W[j:, p].copy()
        alpha = x[0]
        s2 = float(x[1:] @ x[1:])
        nu = np.sqrt(alpha * alpha + s2)
        if j == 0:
            nu0 = nu
        if not (nu > rtol * nu0 and nu > 0.0):
            k = j
            gaps.pop()
            break
        v = np.zeros(mr - j)
        v[0] = 1.0
        if s2 != 0.0:
            beta = -np.copysign(nu, alpha)
            tau[j] = (beta - alpha) / beta
            v[1:] = x[1:] / (alpha - beta)
        else:
            beta = alpha
        out[:j, j] = W[:j, p]
        out[j, j] = beta
        out[j + 1:, j] = v[1:]
        sel[p] = j
        chosen.append(p)
        rest = np.flatnonzero(sel < 0)
        if len(rest):
            blk = W[j:, rest]
            blk -= np.outer(v, tau[j] * (v @ blk))
            W[j:, rest] = blk
            for c in rest:
                if vn1[c] != 0.0:
                    q = abs(W[j, c]) / vn1[c]
                    temp = max(1.0 - q * q, 0.0)
                    temp2 = temp * (vn1[c] / vn2[c]) ** 2
                    if not temp2 > TOL3Z:
                        vn1[c] = vn2[c] = np.sqrt(W[j + 1:, c] @ W[j + 1:, c])
                    else:
                        vn1[c] *= np.sqrt(temp)
    rest = np.flatnonzero(sel < 0)
    out[:, k:] = W[:, rest]
    jpvt = np.array(chosen + list(rest), dtype=np.int64)
    return out, tau, jpvt, k, gaps


def q_of(image, tau, k):
    """the mr x mr orthogonal factor H_0 .. H_{k-1} of an image"""
    mr = image.shape[0]
    Q = np.eye(mr)
    for j in range(k - 1, -1, -1):
        v = np.zeros(mr)
        v[j] = 1.0
        v[j + 1:] = image[j + 1:, j]
        Q -= tau[j] * np.outer(v, v @ Q)
    return Q


def r_of(image, k):
    """R with the remainder after a stop: rows < k of the upper trapezoid, and rows >= k of the columns >= k"""
    R = np.triu(image)
    R[k:, k:] = image[k:, k:]
    return R


def factor_errors(W, image, tau, jpvt, k):
    """(||W P - Q R||_F / ||W||_F, ||Q^T Q - I||_F)"""
    Q = q_of(image, tau, k)
    nrm = np.linalg.norm(W)
    return float(np.linalg.norm(W[:, jpvt] - Q @ r_of(image, k)) / (nrm if nrm > 0 else 1.0)), float(np.linalg.norm(Q.T @ Q - np.eye(Q.shape[0])))


def gelsy(A, B, rcond, min_norm=True):
    """the capi_dgelsy path: (X, k, jpvt, F image, tauf).  A = Q1 R1 (Householder), R1 P = Q2 R, basic or minimum-norm Y, X = P Y"""
    m, n = A.shape
    Q1, R1 = np.linalg.qr(A)
    if rcond < 0:
        rcond = m * 2.0 ** -52
    F, tauf, jpvt, k, _ = geqp3(np.triu(R1), rcond)
    C = q_of(F, tauf, k).T @ (Q1.T @ B)
    Y = np.zeros((n, B.shape[1]))
    if k > 0:
        R = np.triu(F)[:k]
        if min_norm and k < n:
            Zq, T = np.linalg.qr(R.T)
            Y = Zq @ sla.solve_triangular(T, C[:k], trans="T", lower=False)
        else:
            Y[:k] = sla.solve_triangular(R[:, :k], C[:k], lower=False)
    X = np.zeros_like(Y)
    X[jpvt] = Y
    return X, k, jpvt, F, tauf


# ---- cases ----
def planted(m, n, k, smin, seed):
    """(A, U, s, V): A = U diag(s) V^T of rank k, s from 1 down to smin (logarithmically spaced)"""
    rng = np.random.default_rng(seed)
    Uo, _ = np.linalg.qr(rng.standard_normal((m, k)))
    Vo, _ = np.linalg.qr(rng.standard_normal((n, k)))
    s = np.logspace(0.0, np.log10(smin), k) if k > 1 else np.ones(1)
    return np.asfortranarray((Uo * s) @ Vo.T), Uo, s, Vo


def check_case(W, rtol, k_planted=None):
    """the restatement's result on W, after asserting that the references agree among themselves on it: at every step the runner-up's running norm is at
    most (1 - 1e-6) of the pivot's, and with a planted rank sigma_{k+1} / sigma_1 <= 1e-15 (far below the rtol in use)"""
    res = geqp3(W, rtol)
    gaps = res[4]
    assert all(g <= GAP for g in gaps), ("pivot gap", max(gaps))
    if k_planted is not None and k_planted < min(W.shape):
        sv = np.linalg.svd(W, compute_uv=False)
        assert sv[k_planted] / sv[0] <= 1e-15, ("sigma_{k+1} / sigma_1", sv[k_planted] / sv[0])
        assert res[3] == k_planted, (res[3], k_planted)
    return res


# orders and shapes of the factorization tests: (mr, n, ldw - mr, seed).  515 = 64 x 8 + 3: 65 workgroups of 8 columns, the last with three columns
# and two idle waves; 17 = two workgroups and one column.  Kept at kappa 10: the reflector entries of a late column are x / (alpha - beta) with x a
# remainder that carries an absolute error of u ||W||, so an elementwise bar of 1e-12 holds only while ||W|| / ||remainder|| stays modest
GEQP3_SHAPES = [(1, 1, 0, 1), (2, 2, 0, 1), (31, 31, 0, 1), (33, 33, 0, 1), (64, 64, 0, 1), (130, 130, 0, 1), (257, 257, 0, 1), (40, 64, 0, 1),
                (100, 33, 0, 1), (17, 17, 0, 1), (515, 515, 0, 2), (130, 130, 3, 2)]
GEQP3_IDS = [f"{mr}x{n}" + (f"-ld+{pad}" if pad else "") for mr, n, pad, _ in GEQP3_SHAPES]


@functools.lru_cache(maxsize=None)
def geqp3_case(mr, n, seed, smin=0.1):
    """(W, restatement's (image, tau, jpvt, k, gaps)) at rtol = 0, full rank.  Square: triu of the R factor of a planted tall panel, as capi_dgelsy feeds
    the routine; otherwise the planted block itself"""
    kk = min(mr, n)
    if mr == n:
        W = np.asfortranarray(np.triu(np.linalg.qr(planted(4 * n, n, kk, smin, seed)[0])[1]))
    else:
        W = planted(mr, n, kk, smin, seed)[0]
    res = check_case(W, 0.0)
    assert res[3] == kk
    W.setflags(write=False)
    return W, res


# (m, n, planted rank, sigma_k / sigma_1, seed) of the least-squares tests; rcond = RCOND throughout
RCOND = 1e-13
GELSY_SHAPES = [(2048, 64, 40, 1e-3, 1), (2048, 64, 40, 1e-9, 1), (4096, 130, 97, 1e-10, 1), (2048, 33, 33, 1e-12, 1), (2048, 64, 1, 1.0, 1),
                (16384, 256, 200, 1e-8, 1)]
GELSY_IDS = [f"{m}x{n}-rank{k}-s{s:.0e}" for m, n, k, s, _ in GELSY_SHAPES]


@functools.lru_cache(maxsize=None)
def gelsy_case(m, n, k, smin, seed, r=3):
    """(A, B, x_true, k, V): A = U diag(s) V^T planted of rank k; B = A x_true + w with x_true the planted MINIMUM-NORM solution (in range(V)) and w orthogonal to range(A),
    ||w_j|| = rho = min(1e-3, sigma_k / sigma_1) -- a problem with residual rho is conditioned like kappa + kappa^2 rho / (||A|| ||x||) (Wedin), so a larger
    one leaves nothing to measure at kappa 1e10 -- in tests/_lstsq_cases's style (projected off the planted left basis, not off a computed Q).  Asserted: the restatement on triu(R1)
    finds k with gaps at every step, and sigma_{k+1} / sigma_1 <= 1e-15"""
    A, Uo, s, Vo = planted(m, n, k, smin, seed)
    rho = min(1e-3, smin)
    rng = np.random.default_rng(seed + 100)
    x_true = Vo @ rng.standard_normal((k, r))
    w = rng.standard_normal((m, r))
    for _ in range(2):
        w -= Uo @ (Uo.T @ w)
    w *= rho / np.linalg.norm(w, axis=0)
    LD = np.longdouble
    B = np.asfortranarray(((Uo.astype(LD) * s.astype(LD)) @ (Vo.T.astype(LD) @ x_true.astype(LD)) + w.astype(LD)).astype(np.float64))
    R1 = np.triu(np.linalg.qr(A, mode="r"))
    check_case(R1, RCOND, k)
    sv = np.linalg.svd(A, compute_uv=False)
    assert k == n or sv[k] / sv[0] <= 1e-15
    for a in (A, B, x_true):
        a.setflags(write=False)
    return A, B, x_true, k, Vo


def eta(X, x_true):
    return float(np.max(np.linalg.norm(X - x_true, axis=0) / np.linalg.norm(x_true, axis=0)))
