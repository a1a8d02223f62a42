"""numpy restatement of the exponent rule of capi_dpoequ2 / capi_dsym_scale2 / capi_drow_scale2 (capital_amd/csrc/equil_f64.hip): for a diagonal entry
a_jj = f 2^ex_j with f in [0.5, 1) (np.frexp's convention, subnormals included) e_j = floor(ex_j / 2) and dscale[j] = 2^e_j.  Everything here is exact:
frexp, floor_divide and ldexp neither round nor depend on an order."""
import numpy as np

DBL_MIN = np.finfo(np.float64).tiny
SMALL = DBL_MIN / np.finfo(np.float64).eps              # dlaqsy's SMALL = safe minimum / precision (DBL_MIN / DBL_EPSILON), LARGE = 1 / SMALL
LARGE = 1.0 / SMALL


def first_bad(d):
    """0, or j + 1 for the first diagonal entry that is zero, negative, NaN or Inf"""
    d = np.asarray(d, dtype=np.float64)
    bad = ~((d > 0) & np.isfinite(d))
    return int(np.argmax(bad)) + 1 if bad.any() else 0


def exponents(d):
    """e_j = floor(ex_j / 2) for positive finite d_j = f 2^ex_j, f in [0.5, 1)"""
    d = np.asarray(d, dtype=np.float64)
    assert first_bad(d) == 0
    _, ex = np.frexp(d)
    return np.floor_divide(ex.astype(np.int64), 2)


def poequ2(d):
    """(dscale, rec) as capi_dpoequ2 writes them for the diagonal d: rec = [scond, amax, amin, 0], or with a bad entry dscale all ones and
    rec = [1, 0, 0, j + 1]"""
    d = np.asarray(d, dtype=np.float64)
    bad = first_bad(d)
    if bad:
        return np.ones(len(d)), np.array([1.0, 0.0, 0.0, float(bad)])
    dscale = np.ldexp(1.0, exponents(d).astype(np.int32))
    return dscale, np.array([dscale.min() / dscale.max(), d.max(), d.min(), 0.0])


def scales_by_rule(scond, amax, thresh=0.1):
    """dlaqsy's rule as cholinv::equilibrate applies it"""
    return bool(scond < thresh or amax < SMALL or amax > LARGE or thresh > 1.0)


def sym_scale(A, e, sign=1):
    """ldexp(a_ij, -sign (e_i + e_j)) on every element of A"""
    e = np.asarray(e, dtype=np.int64)
    return np.ldexp(A, (-sign * (e[:, None] + e[None, :])).astype(np.int32))


def row_scale(X, e, sign=1):
    """ldexp(x_ij, sign e_i)"""
    e = np.asarray(e, dtype=np.int64)
    return np.ldexp(X, (sign * e).astype(np.int32)[:, None])


def graded(n, kappa, seed=3):
    """the graded input of the equilibration tests: (A, C, D0) with A = triu-symmetrized D0 C D0, C = f1_spectrum(n, kappa, seed) and
    D0 = 10^uniform(-8, 8) from default_rng(n)"""
    import _conditioning as cond
    C = cond.f1_spectrum(n, kappa, seed=seed)
    D0 = 10.0 ** np.random.default_rng(n).uniform(-8, 8, n)
    return cond.symmetrize(D0[:, None] * C * D0[None, :]), C, D0
