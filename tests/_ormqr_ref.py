"""References for capi_dormqr (tests/test_ormqr_ref.py, tests/test_gpu_ormqr.py, tests/test_gpu_gels.py, tests/test_gpu_ormqr_engine.py).

ormqr     LAPACK's dorm2r in numpy: the reflectors H_j = I - tau_j v_j v_j^T of a dgeqrf image applied one at a time, H_1 first for Q^T and H_k first
          for Q.  v_j has an implied 1 on the diagonal and is read strictly below it: nothing on or above A's diagonal is touched.
ormqr_blocked   a restatement of the kernel's scheme: panels of 32, G = P^T P, T by dlarft's recurrence from G and tau, Z = T^T (P^T C) or T (P^T C),
          C -= P Z; ascending panels for Q^T, descending for Q.
image     the ORACLE's dgeqrf image and tau of A (oracle.dgeqrf, column by column): parity tests on it do not depend on capi_dgeqrf."""
import numpy as np

NB = 32


def image(A):
    import oracle
    fac = np.array(A, dtype=np.float64, order="F")
    tau = oracle.dgeqrf(fac)
    return fac, np.asarray(tau, dtype=np.float64)


def ormqr(fac, tau, C, trans, k=None):
    """Q^T C (trans) or Q C, Q = H_1 .. H_k"""
    m = fac.shape[0]
    k = len(tau) if k is None else k
    out = np.array(C, dtype=np.float64, order="F")
    for j in (range(k) if trans else range(k - 1, -1, -1)):
        v = np.zeros(m)
        v[j] = 1.0
        v[j + 1:] = fac[j + 1:, j]
        out -= tau[j] * np.outer(v, v @ out)
    return out


def larft(G, tau):
    """T (upper triangular) of the block reflector I - V T V^T from G = V^T V: T(0:i, i) = -tau_i T(0:i, 0:i) G(0:i, i)"""
    nb = len(tau)
    T = np.zeros((nb, nb))
    for i in range(nb):
        T[:i, i] = -tau[i] * (T[:i, :i] @ G[:i, i])
        T[i, i] = tau[i]
    return T


def ormqr_blocked(fac, tau, C, trans, k=None):
    m = fac.shape[0]
    k = len(tau) if k is None else k
    out = np.array(C, dtype=np.float64, order="F")
    starts = list(range(0, k, NB))
    for j0 in (starts if trans else starts[::-1]):
        nb = min(NB, k - j0)
        P = np.tril(fac[j0:, j0:j0 + nb], -1)
        P[np.arange(nb), np.arange(nb)] = 1.0
        T = larft(P.T @ P, tau[j0:j0 + nb])
        W = P.T @ out[j0:]
        out[j0:] -= P @ ((T.T if trans else T) @ W)
    return out
