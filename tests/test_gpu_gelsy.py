"""capi_dgelsy (csrc/qr_apply_f64.hip) and capital_amd.hqr.Hqr.lstsq_pivoted: least squares for A of any rank by Householder QR and capi_dgeqp3 on
the n x n triangle.

Problems are tests/_qrcp_ref.gelsy_case's: A planted of rank k with sigma_k / sigma_1 down to 1e-10 (the builder asserts a pivot gap at every step of the
restatement and sigma_{k+1} / sigma_1 <= 1e-15), rcond = 1e-13, B = A x_true + w with x_true the planted minimum-norm solution and w orthogonal to
range(A).  The rule for X is the project's: eta_gpu <= 10 max(eta_ref, u), eta_ref the larger of scipy's dgelsy and the
restatement for the minimum-norm X, scipy's lstsq on A[:, jpvt[:k]] for the basic one.  Residual norms: tests/_lstsq_cases.residual_check's bound.
16384 x 256 crosses capi_dgeqrf's tall gate (m >= 64 n) and its fallback.  Every comparison prints err/tol before it asserts."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.linalg as sla

import _lstsq_cases as lc
import _qrcp_ref as ref
from _qrcp_ref import U64

pytestmark = pytest.mark.gpu

CB = 10.0
FILL = 7.25
RCOND = ref.RCOND
# the shapes of the issue, each with r = 1, 3 or 40 right-hand sides
CASES = [c + (r,) for c, r in zip(ref.GELSY_SHAPES, (3, 1, 40, 3, 3, 3))]
IDS = [i + f"-r{c[-1]}" for i, c in zip(ref.GELSY_IDS, CASES)]

_bits = lambda a: np.ascontiguousarray(a).view(np.int64)


def _gelsy(hip, A, B, min_norm, rcond=RCOND, norms=True):
    """capi_dgelsy on device copies: dict of rc, k, A, tau, F, tauf, jpvt, B, colnorm2 on exit"""
    import torch
    from capital_amd import capi
    m, n = A.shape
    r = B.shape[1]
    dA, dB = capi.to_device(A), capi.to_device(B)
    full = lambda *s: torch.full(s, FILL, dtype=torch.float64, device="cuda")     # noqa: E731
    dtau, dF, dtauf, dZ, dtauz = full(n), full(n, n), full(n), full(n, n), full(n)
    dj = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    dn = full(r) if norms else None
    k = ctypes.c_int(-99)
    torch.cuda.synchronize()
    rc = hip.L.capi_dgelsy(hip.h, m, n, r, capi.ptr(dA), A.shape[0], capi.ptr(dtau), capi.ptr(dF), n, capi.ptr(dtauf), capi.ptr(dj),
                           capi.ptr(dZ) if min_norm else None, n, capi.ptr(dtauz) if min_norm else None, capi.ptr(dB), B.shape[0], rcond,
                           1 if min_norm else 0, capi.ptr(dn), ctypes.byref(k))
    hip.sync()
    return dict(rc=rc, k=k.value, A=capi.to_host(dA), tau=dtau.cpu().numpy(), F=capi.to_host(dF), tauf=dtauf.cpu().numpy(),
                jpvt=dj.cpu().numpy().astype(np.int64), B=capi.to_host(dB), cn2=(dn.cpu().numpy() if norms else None), Z=capi.to_host(dZ))


def _geqrf(hip, A):
    import torch
    from capital_amd import capi
    m, n = A.shape
    dA = capi.to_device(A)
    dtau = torch.full((n,), FILL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    hip.call("capi_dgeqrf", m, n, capi.ptr(dA), m, capi.ptr(dtau))
    hip.sync()
    return capi.to_host(dA), dtau.cpu().numpy()


def _rule(what, X, x_true, eta_ref):
    e = lc.eta(X, x_true)
    bound = CB * max(eta_ref, U64)
    print(f"{what}: eta {e:.3e} (reference {eta_ref:.3e}, ratio {e / max(eta_ref, U64):.2f}) bound {bound:.3e}")
    assert e <= bound, (what, e, eta_ref)


def _residuals(what, A, B, X, cn2):
    err, bound = lc.residual_check(A, B, X, np.sqrt(cn2))
    print(f"{what}: residual norms err/bound {float(np.max(err / bound)):.3e}")
    assert np.all(err <= bound), (what, err, bound)


@pytest.mark.parametrize("m,n,k,smin,seed,r", CASES, ids=IDS)
def test_gelsy(hip, m, n, k, smin, seed, r):
    from capital_amd.hqr import Hqr
    A, B, x_true, _, Vo = ref.gelsy_case(m, n, k, smin, seed, r)
    what = f"{m}x{n} rank {k} sigma_k {smin:.0e} r={r}"
    # minimum norm
    g = _gelsy(hip, A, B, True)
    assert g["rc"] == 0 and g["k"] == k, (g["rc"], g["k"], hip.L.capi_last_error(hip.h).decode())
    assert sorted(g["jpvt"]) == list(range(n))
    Xr, kr, jr, _, _ = ref.gelsy(A, B, RCOND, True)
    assert kr == k and np.array_equal(g["jpvt"][:k], jr[:k])
    Xs, _, ks, _ = sla.lstsq(A, B, cond=RCOND, lapack_driver="gelsy")
    assert ks == k
    X = g["B"][:n]
    _rule(f"{what} minimum norm", X, x_true, max(lc.eta(Xs, x_true), lc.eta(Xr, x_true)))
    _residuals(f"{what} minimum norm", A, B, X, g["cn2"])
    # the image and tau: bit for bit a separate capi_dgeqrf's
    fac, tau = _geqrf(hip, A)
    assert np.array_equal(_bits(g["A"]), _bits(fac)) and np.array_equal(_bits(g["tau"]), _bits(tau))
    # basic
    b = _gelsy(hip, A, B, False)
    assert b["rc"] == 0 and b["k"] == k and np.array_equal(b["jpvt"], g["jpvt"])
    assert np.array_equal(_bits(b["F"]), _bits(g["F"])) and np.array_equal(_bits(b["cn2"]), _bits(g["cn2"]))
    Xb = b["B"][:n]
    jp = b["jpvt"]
    assert np.all(Xb[jp[k:]] == 0.0)
    # the truth of the basic solution: A = U S V^T and A[:, jpvt[:k]] y = A x_true give V[jpvt[:k]]^T y = V^T x_true, a k x k system
    Asub = A[:, jp[:k]]
    xb_true = np.linalg.solve(Vo[jp[:k]].T, Vo.T @ x_true)
    Xl = sla.lstsq(Asub, B, lapack_driver="gelsy")[0]
    _rule(f"{what} basic, on A[:, jpvt[:k]]", Xb[jp[:k]], xb_true, lc.eta(Xl, xb_true))
    _residuals(f"{what} basic", A, B, Xb, b["cn2"])
    # a second set of right-hand sides on the factors: Hqr.lstsq_pivoted's second route is bit for bit its first
    q = Hqr(hip, A)
    X1, res1, k1 = q.lstsq_pivoted(B, rcond=RCOND)
    assert k1 == k and np.array_equal(_bits(X1), _bits(X)) and np.array_equal(_bits(res1), _bits(np.sqrt(g["cn2"])))
    X2, res2, k2 = q.lstsq_pivoted(B, rcond=RCOND)
    assert k2 == k and np.array_equal(_bits(X2), _bits(X1)) and np.array_equal(_bits(res2), _bits(res1))
    X3, _, _ = q.lstsq_pivoted(B, rcond=RCOND, min_norm=False)
    assert np.array_equal(_bits(X3), _bits(Xb))
    assert np.array_equal(q.jpvt, g["jpvt"]) and q.rank == k
    # another rcond: only the triangle is pivoted again
    k4 = q.factor_pivoted(rcond=0.5)
    assert 1 <= k4 <= k and q.factor_pivoted(rcond=RCOND) == k
    X5, _, _ = q.lstsq_pivoted(B, rcond=RCOND)
    assert np.array_equal(_bits(X5), _bits(X))
    q.close()


def test_rank_zero(hip):
    """A zero: rank 0, X = 0, colnorm2 the squared column norms of B"""
    A = np.zeros((300, 20), order="F")
    B = np.asfortranarray(np.random.default_rng(4).standard_normal((300, 3)))
    for mn in (True, False):
        g = _gelsy(hip, A, B, mn)
        assert g["rc"] == 0 and g["k"] == 0 and np.all(g["B"][:20] == 0.0) and np.array_equal(g["jpvt"], np.arange(20))
        err = np.abs(g["cn2"] - (B * B).sum(axis=0)).max() / (B * B).sum(axis=0).max()
        print(f"rank 0 colnorm2: err/tol {err:.3e}/1.0e-13")
        assert err <= 1e-13


def test_refuses_wide_and_bad_arguments(hip):
    import torch
    from capital_amd import capi
    A = np.asfortranarray(np.random.default_rng(5).random((40, 50)))
    B = np.asfortranarray(np.random.default_rng(6).random((50, 2)))
    dA, dB = capi.to_device(A), capi.to_device(B)
    full = lambda *s: torch.full(s, FILL, dtype=torch.float64, device="cuda")     # noqa: E731
    dtau, dF, dtauf, dZ, dtauz, dn = full(50), full(50, 50), full(50), full(50, 50), full(50), full(2)
    dj = torch.full((50,), -7, dtype=torch.int32, device="cuda")
    p = capi.ptr
    torch.cuda.synchronize()
    good = [40, 50, 2, p(dA), 40, p(dtau), p(dF), 50, p(dtauf), p(dj), p(dZ), 50, p(dtauz), p(dB), 50, RCOND, 1, p(dn)]
    calls = [good]                                                   # m < n
    tall = list(good)
    tall[0], tall[1], tall[4], tall[7], tall[11], tall[14] = 50, 40, 50, 40, 40, 50     # a well-formed 50 x 40 problem, spoilt one argument at a time:
    for idx, val in ((3, None), (6, None), (9, None), (10, None), (12, None), (13, None), (4, 49), (7, 39), (11, 39), (14, 49), (15, float("nan")),
                     (13, p(dB) + 4), (2, 0)):
        c = list(tall)
        c[idx] = val
        calls.append(c)
    for c in calls:
        k = ctypes.c_int(-99)
        rc = hip.L.capi_dgelsy(hip.h, *c, ctypes.byref(k))
        assert rc == -1 and k.value == -99, c
    hip.sync()
    print(hip.L.capi_last_error(hip.h).decode())
    assert np.array_equal(_bits(capi.to_host(dA)), _bits(A)) and np.array_equal(_bits(capi.to_host(dB)), _bits(B))
    for t in (dtau, dF, dtauf, dZ, dtauz, dn):
        assert torch.all(t == FILL)
    assert torch.all(dj == -7)


@functools.lru_cache(maxsize=None)
def _collinear(kind):
    """kappa 1e10 on 62 independent columns plus two collinear ones; B in range(A).
    "axis": the pair is 2 e_1 and 3 e_1 in front.  H_1 is then the identity reflector, the second column keeps exact zeros below its first row and
    R(2, 2) is an exact zero: capi_dgels returns info = 2.
    "copies": the pair is copies of columns 3 and 17 behind the others.  Measured on an MI355X: capi_dgels returns info 0 there -- the copies' pivots
    come out as rounding noise, |r_jj| = 1.2e-16 and 1.3e-16 beside |r_11| = 0.15, not as exact zeros -- and divides by them."""
    m, n = 2048, 64
    A0 = ref.planted(m, 62, 62, 1e-10, 7)[0]
    A = np.zeros((m, n), order="F")
    if kind == "axis":
        A[0, 0], A[0, 1] = 2.0, 3.0
        A[:, 2:] = A0
        N = np.zeros((n, 1))
        N[0, 0], N[1, 0] = 3.0, -2.0                         # 3 (2 e_1) - 2 (3 e_1) = 0
    else:
        A[:, :62] = A0
        A[:, 62] = A0[:, 3]
        A[:, 63] = A0[:, 17]
        N = np.zeros((n, 2))
        N[3, 0], N[62, 0], N[17, 1], N[63, 1] = 1.0, -1.0, 1.0, -1.0
    y = np.random.default_rng(8).standard_normal((n, 3))
    B = np.asfortranarray((A.astype(np.longdouble) @ y.astype(np.longdouble)).astype(np.float64))
    N /= np.linalg.norm(N, axis=0)
    for a in (A, B):
        a.setflags(write=False)
    return A, B, y, N


@pytest.mark.parametrize("kind", ["axis", "copies"])
def test_collinear_columns_at_kappa_1e10(hip, kind):
    """a panel neither earlier route takes: the Gram route cannot see a gap at 1e-10 (its resolution is sqrt(u)), capi_dgels refuses ("axis") or
    divides by noise ("copies"); capi_dgelsy finds the rank and the minimum-norm solution, measured against the planted one (the null space of A is known exactly)"""
    import torch
    from capital_amd import capi
    from capital_amd.hqr import Hqr
    A, B, y, N = _collinear(kind)
    m, n = A.shape
    dA, dB = capi.to_device(A), capi.to_device(B)
    dtau = torch.zeros(n, dtype=torch.float64, device="cuda")
    info = ctypes.c_int(-99)
    torch.cuda.synchronize()
    assert hip.L.capi_dgels(hip.h, m, n, 3, capi.ptr(dA), m, capi.ptr(dtau), capi.ptr(dB), m, None, ctypes.byref(info)) == 0
    hip.sync()
    d = np.abs(np.diag(capi.to_host(dA)[:n]))
    print(f"collinear {kind}: capi_dgels info {info.value}; min |r_jj| {d.min():.3e}, |r_11| {d[0]:.3e}")
    if kind == "axis":
        assert info.value > 0
    k_true = 63 if kind == "axis" else 62
    g = _gelsy(hip, A, B, True)
    assert g["rc"] == 0 and g["k"] == k_true, g["k"]
    X = g["B"][:n]
    Xs, _, ks, _ = sla.lstsq(A, B, cond=RCOND, lapack_driver="gelsy")
    assert ks == k_true
    res = np.linalg.norm(B - A @ X, axis=0) / np.linalg.norm(B, axis=0)
    res_s = np.linalg.norm(B - A @ Xs, axis=0) / np.linalg.norm(B, axis=0)
    print(f"collinear {kind}: relative residuals {res.max():.3e} (scipy dgelsy {res_s.max():.3e}); ||X|| {np.linalg.norm(X):.3e} (scipy {np.linalg.norm(Xs):.3e})")
    assert res.max() <= CB * max(res_s.max(), U64)
    # the planted minimum-norm solution: B = A y, and the null space of A is known exactly -- y minus its part in it
    x_true = y - N @ (N.T @ y)
    _rule(f"collinear {kind} minimum norm", X, x_true, lc.eta(Xs, x_true))
    q = Hqr(hip, A)
    Xq, _, kq = q.lstsq_pivoted(B, rcond=RCOND)
    assert kq == k_true and np.array_equal(_bits(Xq), _bits(X))
    q.close()


def test_hqr_lstsq_still_raises_on_the_singular_case(hip):
    """the unpivoted route is unchanged: an exactly zero column raises, and the pivoted route solves the same problem"""
    from capital_amd import capi
    from capital_amd.hqr import Hqr
    A, B, _ = lc.problem(2048, 64, 3, 1e1, 0.0)
    A = np.asfortranarray(A).copy(order="F")
    A[:, 40] = 0.0
    q = Hqr(hip, A)
    with pytest.raises(capi.CapiError, match="column 41"):
        q.lstsq(B)
    q.close()
    dA, dB = capi.to_device(A), capi.to_device(B)
    import torch
    dtau = torch.zeros(64, dtype=torch.float64, device="cuda")
    info = ctypes.c_int(-99)
    torch.cuda.synchronize()
    assert hip.L.capi_dgels(hip.h, 2048, 64, 3, capi.ptr(dA), 2048, capi.ptr(dtau), capi.ptr(dB), 2048, None, ctypes.byref(info)) == 0
    assert info.value == 41
    q = Hqr(hip, A)
    X, res, k = q.lstsq_pivoted(B)
    assert k == 63 and np.all(X[40] == 0.0)
    Xs = sla.lstsq(A, B, lapack_driver="gelsy")[0]
    e = np.abs(X - Xs).max() / np.abs(Xs).max()
    print(f"zero column: X against scipy dgelsy err/tol {e:.3e}/1.0e-12")
    assert e <= 1e-12
    q.close()
