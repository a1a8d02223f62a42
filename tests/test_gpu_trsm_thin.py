"""capi_dtrsm_thin (B <- op(T)^-1 B by substitution, T upper triangular in column-major or packed storage, r <= 32 columns; the kernel of
capital_amd/csrc/tri_solve_f64.hip and the step list of trsm_thin_plan.h) on the GPU.

EXACT cases: T has integer entries in -8..8 above the diagonal and diagonal entries from {+-1, +-2, +-0.5}; X0 has integer entries in -8..8 and
B = op(T) X0 is formed in numpy.  Substitution then meets only multiples of 1/2 far below 2^53 whatever its order (the reciprocals 1, 1/2 and 2 are
exact), so the comparison is for equality.  A kernel that drops or doubles a block, reads below the diagonal, takes a packed column from a wrong
offset, mixes up the order of leaves and products or writes outside the n x r window fails outright.
REAL values: T = chol(A)^T for A of a prescribed spectrum (a random triangle would be exponentially ill-conditioned); the normwise backward error
eta = max_j ||op(T) x_j - b_j|| / (||T||_2 ||x_j|| + ||b_j||) in numpy.longdouble under the project's rule eta_gpu <= 10 max(eta_ref, u), eta_ref from
scipy.linalg.solve_triangular on the same T and B."""
import numpy as np
import pytest
import scipy.linalg as sla

import _conditioning as cond
from test_gpu_tri_thin import EINVAL, NOTRANS, TRANS, Out, dev, ints, pack_upper, pstart

pytestmark = pytest.mark.gpu
U64 = 2.0 ** -53
LD = np.longdouble

NS = [1, 2, 31, 32, 33, 255, 256, 257, 511, 513, 1023, 1025, 2100]
RS = [1, 3, 16, 17, 32]
STORES = ["packed", "view77", "view78", "ld", "ld+3"]
CASES = [(n, RS[(i + t + 2 * k) % 5], t, st) for i, n in enumerate(NS) for t in (NOTRANS, TRANS) for k, st in enumerate(STORES)]


def exact_triangle(rng, n):
    U = np.triu(ints(rng, (n, n)), 1)
    U[np.arange(n), np.arange(n)] = rng.choice([1.0, -1.0, 2.0, -2.0, 0.5, -0.5], n)
    return np.asfortranarray(U)


def place(U, store):
    """the triangle on the device as `store` says, NaN wherever the call must not look: (tensor kept alive, pointer, ldt, col0)"""
    n = U.shape[0]
    if store in ("packed", "view77", "view78"):
        col0 = {"packed": 0, "view77": 77, "view78": 78}[store]
        N = col0 + n + (5 if col0 else 0)                                 # the view lies inside a larger triangle
        host = np.full(1 + pstart(N) + 1, np.nan)                         # a NaN word in front of and behind the triangle
        for j in range(n):
            s = 1 + pstart(col0 + j) + col0
            host[s:s + j + 1] = U[:j + 1, j]
        dT = dev(host)
        return dT, dT.data_ptr() + 8 * (1 + pstart(col0) + col0), 0, col0
    ld = n + (3 if store == "ld+3" else 0)
    full = np.full((ld, n), np.nan)                                       # NaN below the diagonal and in the padding rows
    full[:n, :] = np.where(np.arange(n)[:, None] <= np.arange(n)[None, :], U, np.nan)
    dT = dev(full.T.reshape(-1))
    return dT, dT.data_ptr(), ld, 0


def solve(hip, trans, n, r, Tptr, ldt, col0, out, raw=False):
    args = (trans, n, r, Tptr, ldt, col0, out.ptr, out.ld)
    if raw:
        rc = hip.L.capi_dtrsm_thin(hip.h, *args)
        hip.sync()
        return rc
    hip.call("capi_dtrsm_thin", *args)
    hip.sync()


@pytest.mark.parametrize("n,r,trans,store", CASES, ids=[f"n{n}-r{r}-t{t}-{st}" for n, r, t, st in CASES])
def test_exact_solves(hip, n, r, trans, store):
    rng = np.random.default_rng(1000 * n + 10 * r + trans)
    U = exact_triangle(rng, n)
    X0 = ints(rng, (n, r))
    B = (U.T if trans else U) @ X0
    keep, Tptr, ldt, col0 = place(U, store)
    out = Out(B)                                                          # ldb = n + 5, three doubles into a sentinel-filled buffer
    solve(hip, trans, n, r, Tptr, ldt, col0, out)
    np.testing.assert_array_equal(out.get(), X0)                          # (get() checks that nothing outside the window was written)


@pytest.mark.parametrize("trans", [NOTRANS, TRANS])
def test_nan_below_the_diagonal_changes_no_bit_and_runs_repeat(hip, trans):
    n, r = 1100, 17
    rng = np.random.default_rng(40 + trans)
    A = cond.f1_spectrum(n, 1e4)
    U = np.asfortranarray(np.linalg.cholesky(A).T)
    B = np.asfortranarray(rng.standard_normal((n, r)))
    got = []
    for fill in (0.0, np.nan, np.nan):
        full = np.asfortranarray(np.where(np.arange(n)[:, None] <= np.arange(n)[None, :], U, fill))
        dT = dev(full.T.reshape(-1))
        out = Out(B)
        solve(hip, trans, n, r, dT.data_ptr(), n, 0, out)
        got.append(out.get())
    assert np.all(np.isfinite(got[0]))
    assert got[0].tobytes() == got[1].tobytes()                           # NaN below the diagonal: the same bits as zeros there
    assert got[1].tobytes() == got[2].tobytes()                           # two runs: the same bits


def test_argument_errors_touch_nothing(hip):
    rng = np.random.default_rng(3)
    n = 40
    U = exact_triangle(rng, n)
    dT = dev(U.T.reshape(-1))
    B = ints(rng, (n, 33))
    out = Out(B)
    assert solve(hip, NOTRANS, n, 33, dT.data_ptr(), n, 0, out, raw=True) == EINVAL
    np.testing.assert_array_equal(out.get(), B)
    out = Out(B[:, :3])
    assert solve(hip, TRANS, n, 0, dT.data_ptr(), n, 0, out, raw=True) == EINVAL
    assert solve(hip, 2, n, 3, dT.data_ptr(), n, 0, out, raw=True) == EINVAL
    assert solve(hip, NOTRANS, n, 3, dT.data_ptr(), n - 1, 0, out, raw=True) == EINVAL
    np.testing.assert_array_equal(out.get(), B[:, :3])
    for trans in (NOTRANS, TRANS):                                        # n == 0 is OK and touches nothing
        assert solve(hip, trans, 0, 3, dT.data_ptr(), 1, 0, out, raw=True) == 0
        assert solve(hip, trans, 0, 3, None, 0, 0, out, raw=True) == 0
    np.testing.assert_array_equal(out.get(), B[:, :3])


def eta(T, normT2, B, X):
    R = T.astype(LD) @ X.astype(LD) - B.astype(LD)
    num = np.sqrt((R * R).sum(axis=0))
    den = LD(normT2) * np.sqrt((X.astype(LD) ** 2).sum(axis=0)) + np.sqrt((B.astype(LD) ** 2).sum(axis=0))
    return float((num / den).max())


_CHOL = {}


def chol_factor(kappa):
    if kappa not in _CHOL:
        U = np.asfortranarray(np.linalg.cholesky(cond.f1_spectrum(1000, kappa)).T)
        _CHOL[kappa] = (U, np.linalg.norm(U, 2))
    return _CHOL[kappa]


@pytest.mark.parametrize("trans", [NOTRANS, TRANS])
@pytest.mark.parametrize("kappa", [1e2, 1e8, 1e12])
def test_backward_error_on_cholesky_factors(hip, kappa, trans):
    n, r = 1000, 3
    U, normT2 = chol_factor(kappa)
    op = np.asfortranarray(U.T) if trans else U
    B = np.asfortranarray(np.random.default_rng(int(np.log10(kappa)) + trans).standard_normal((n, r)))
    eta_ref = eta(op, normT2, B, sla.solve_triangular(U, B, trans=1 if trans else 0, lower=False))
    etas = {}
    for store in ("packed", "ld"):
        keep, Tptr, ldt, col0 = place(U, store)
        out = Out(B)
        solve(hip, trans, n, r, Tptr, ldt, col0, out)
        etas[store] = eta(op, normT2, B, out.get())
    print(f"dtrsm_thin kappa={kappa:.0e} trans={trans}: eta packed {etas['packed']:.2e}, full {etas['ld']:.2e}; solve_triangular {eta_ref:.2e}")
    for e in etas.values():
        assert e <= 10 * max(eta_ref, U64), (e, eta_ref)
