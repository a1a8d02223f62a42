"""numpy restatements of what cholesky::cholinv::apply and inverse_diagonal compute on the factors of A = R^T R, form by form, in float64 -- the
references that the GPU tests take their eta_ref and e_ref from (tests/test_gpu_cholinv_apply.py), checked themselves against scipy in
tests/test_apply_host.py.

    half(R, B, trans, form, h1)      R^-T B (trans) or R^-1 B in one of the four forms of cholinv's apply_half:
        "subst"     substitution on R, one row at a time (capi_dtrsm_thin)
        "trsm"      the block solve of TRSM mode: diagonal blocks of order 256 inverted, the rest by products (capi_dtrsm)
        "complete"  one product with the explicit inverse
        "block"     the inverse kept as R11^-1, R22^-1 and R12 (complete_inv = 0, top split at h1):
                    R^-T: y1 = R11^-T b1, y2 = R22^-T (b2 - R12^T y1);  R^-1: x2 = R22^-1 y2, x1 = R11^-1 (y1 - R12 x2)
    inverse_diagonal(R, h1)          diag(A^-1) as row sums of squares of R^-1; with h1 the block form: the two diagonal blocks and
                                     R^-1_12 = -R11^-1 R12 R22^-1 added into the leading h1 entries
    eta_half(R, normR2, B, Y, trans) the normwise backward error max_j ||op(R) y_j - b_j|| / (||R||_2 ||y_j|| + ||b_j||) in longdouble"""
import numpy as np
import scipy.linalg as sla

LD = np.longdouble
FORMS = ("subst", "trsm", "complete", "block")


def chol_upper(A):
    return np.asfortranarray(np.linalg.cholesky(A).T)


def tri_inverse(R):
    return sla.solve_triangular(R, np.eye(R.shape[0]))


def _subst(R, B, trans):
    n = R.shape[0]
    Y = np.array(B, dtype=np.float64, order="F")
    if trans:                                   # R^T y = b: forward
        for i in range(n):
            Y[i] = (Y[i] - R[:i, i] @ Y[:i]) / R[i, i]
    else:                                       # R x = y: backward
        for i in range(n - 1, -1, -1):
            Y[i] = (Y[i] - R[i, i + 1:] @ Y[i + 1:]) / R[i, i]
    return Y


def _trsm(R, B, trans, nb=256):
    n = R.shape[0]
    Y = np.array(B, dtype=np.float64, order="F")
    starts = list(range(0, n, nb))
    for k in (starts if trans else starts[::-1]):
        e = min(n, k + nb)
        Dk = tri_inverse(R[k:e, k:e])
        if trans:
            Y[k:e] = Dk.T @ (Y[k:e] - R[:k, k:e].T @ Y[:k])
        else:
            Y[k:e] = Dk @ (Y[k:e] - R[k:e, e:] @ Y[e:])
    return Y


def half(R, B, trans, form, h1=None, Ri=None):
    """Ri: tri_inverse(R) where the caller has it already ("complete")"""
    B = np.asarray(B, dtype=np.float64)
    if form == "subst":
        return _subst(R, B, trans)
    if form == "trsm":
        return _trsm(R, B, trans)
    if form == "complete":
        Ri = tri_inverse(R) if Ri is None else Ri
        return (Ri.T if trans else Ri) @ B
    assert form == "block" and h1 is not None and 0 < h1 < R.shape[0]
    I11, I22, R12 = tri_inverse(R[:h1, :h1]), tri_inverse(R[h1:, h1:]), R[:h1, h1:]
    Y = np.empty(B.shape, order="F")
    if trans:
        Y[:h1] = I11.T @ B[:h1]
        Y[h1:] = I22.T @ (B[h1:] - R12.T @ Y[:h1])
    else:
        Y[h1:] = I22 @ B[h1:]
        Y[:h1] = I11 @ (B[:h1] - R12 @ Y[h1:])
    return Y


def inverse_diagonal(R, h1=None):
    if h1 is None:
        Ri = tri_inverse(R)
        return (Ri * Ri).sum(axis=1)
    I11, I22, R12 = tri_inverse(R[:h1, :h1]), tri_inverse(R[h1:, h1:]), R[:h1, h1:]
    I12 = -(I11 @ R12) @ I22
    d = np.concatenate([(I11 * I11).sum(axis=1), (I22 * I22).sum(axis=1)])
    d[:h1] += (I12 * I12).sum(axis=1)
    return d


def eta_half(R, normR2, B, Y, trans):
    """R: the factor the result is measured on (upper triangular); normR2 its 2-norm"""
    Rl, Yl, Bl = np.triu(R).astype(LD), np.asarray(Y).astype(LD), np.asarray(B).astype(LD)
    D = (Rl.T if trans else Rl) @ Yl - Bl
    num = np.sqrt((D * D).sum(axis=0))
    den = LD(normR2) * np.sqrt((Yl * Yl).sum(axis=0)) + np.sqrt((Bl * Bl).sum(axis=0))
    return float((num / den).max())
