"""capi_dgels (csrc/qr_apply_f64.hip) and capital_amd.hqr.Hqr: least squares by Householder QR up to kappa(A) ~ 1 / u.

Problems are tests/_lstsq_cases.problem's (planted solution, residual rho orthogonal to range(A)).  The rule for X is the project's (DESIGN.md
section 2a): eta_gpu <= CB max(eta_householder, u), CB = 10, eta_householder numpy's Householder QR + triangular solve; on the CPU the blocked scheme
in numpy gives eta / eta_householder between 0.36 and 1.40 on these families.  Residual norms: tests/_lstsq_cases.residual_check's bound.

The tail of B (rows n ..) and the Q^T B of a singular problem are compared with tests/_ormqr_ref.py's dorm2r applied with the reflectors the call
left in A and tau -- the image that another test pins to capi_dgeqrf's bit for bit.  Against the reflectors of a DIFFERENT factorisation of the same A
the tail is not comparable entry by entry: the basis of range(A)'s complement moves with the reflectors, by kappa u (the figure against the oracle's
image is printed for the well-conditioned cases, not asserted).  Every comparison prints err/tol before it asserts."""
import ctypes
import functools

import numpy as np
import pytest

import _lstsq_cases as lc
import _ormqr_ref as ref
from _conditioning import U64

pytestmark = pytest.mark.gpu

TOL = 1e-12
CB = 10.0
FILL = 7.25
CASES = [(2048, 64, 3, 1e1, 0.0), (2048, 64, 3, 1e4, 1.0), (4096, 64, 32, 1e7, 1e-3), (2048, 32, 1, 1e10, 0.0), (2048, 64, 3, 1e12, 0.0),
         (2048, 64, 3, 1e14, 0.0), (8192, 130, 5, 1e4, 1.0), (4096, 64, 40, 1e4, 1.0), (16384, 256, 4, 1e4, 1.0), (16384, 256, 4, 1e14, 0.0)]
IDS = [f"{m}x{n}-r{r}-k{k:.0e}-rho{rho:g}" for m, n, r, k, rho in CASES]

_bits = lambda a: np.ascontiguousarray(a).view(np.int64)


def _check(what, err, tol=TOL):
    print(f"{what}: err/tol {err:.3e}/{tol:.1e} = {err / tol:.3f}")
    assert err <= tol, (what, err, tol)


@functools.lru_cache(maxsize=None)
def _problem(m, n, r, kappa, rho):
    A, B, x_true = lc.problem(m, n, r, kappa, rho)
    A = np.asfortranarray(A)
    eta_h = lc.eta(lc.solve_householder(A, B), x_true)
    for a in (A, B, x_true):
        a.setflags(write=False)
    return A, B, x_true, eta_h


def _gels(hip, A, B, norms=True):
    """capi_dgels on device copies: (rc, info, A on exit, tau, B on exit, colnorm2 or None)"""
    import torch
    from capital_amd import capi
    m, n = A.shape
    r = B.shape[1]
    dA, dB = capi.to_device(A), capi.to_device(B)
    dtau = torch.full((n,), FILL, dtype=torch.float64, device="cuda")
    dn = torch.full((r,), FILL, dtype=torch.float64, device="cuda") if norms else None
    info = ctypes.c_int(-99)
    torch.cuda.synchronize()
    rc = hip.L.capi_dgels(hip.h, m, n, r, capi.ptr(dA), m, capi.ptr(dtau), capi.ptr(dB), m, capi.ptr(dn), ctypes.byref(info))
    hip.sync()
    return rc, info.value, capi.to_host(dA), dtau.cpu().numpy(), capi.to_host(dB), (dn.cpu().numpy() if norms else None)


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


def _assert_rule(what, X, x_true, eta_h):
    e = lc.eta(X, x_true)
    bound = CB * max(eta_h, U64)
    print(f"{what}: eta {e:.3e} (householder {eta_h:.3e}, ratio {e / max(eta_h, U64):.2f}) bound {bound:.3e}")
    assert e <= bound, (what, e, eta_h)


@pytest.mark.parametrize("m,n,r,kappa,rho", CASES, ids=IDS)
def test_gels(hip, oracle, m, n, r, kappa, rho):
    """X by the rule, the residual norms, the tail of Q^T B, the image and tau against a separate capi_dgeqrf bit for bit, and a second set of
    right-hand sides through capi_dormqr + capi_dtrsm_thin on the factors the call left"""
    import torch
    from capital_amd import capi
    A, B, x_true, eta_h = _problem(m, n, r, kappa, rho)
    what = f"{m}x{n} r={r} kappa={kappa:.0e} rho={rho:g}"
    rc, info, fac, tau, out, cn2 = _gels(hip, A, B)
    assert rc == 0 and info == 0, (rc, info, hip.L.capi_last_error(hip.h).decode())
    X = out[:n]
    _assert_rule(what, X, x_true, eta_h)
    # residual norms
    err, bound = lc.residual_check(A, B, X, np.sqrt(cn2))
    worst = float(np.max(err / bound))
    print(f"{what}: residual norms err/bound {worst:.3e}")
    assert np.all(err <= bound), (what, err, bound)
    # the tail of Q^T B, with the reflectors the call left behind
    qtb = ref.ormqr(fac, tau, B, True)
    _check(f"{what} tail of Q^T B", np.abs(out[n:] - qtb[n:]).max() / np.abs(B).max())
    if kappa <= 1e4:
        ofac, otau = ref.image(A)
        print(f"{what} tail against the oracle's reflectors (not asserted): {np.abs(out[n:] - ref.ormqr(ofac, otau, B, True)[n:]).max() / np.abs(B).max():.3e}")
    # the image
    fac2, tau2 = _geqrf(hip, A)
    assert np.array_equal(_bits(fac), _bits(fac2)) and np.array_equal(_bits(tau), _bits(tau2))
    # more right-hand sides on those factors
    r2 = 3
    x2 = np.random.default_rng(m + n + r).standard_normal((n, r2))
    B2 = np.asfortranarray((A.astype(np.longdouble) @ x2.astype(np.longdouble)).astype(np.float64))
    eta2 = lc.eta(lc.solve_householder(A, B2), x2)
    dA, dtau, dB2 = capi.to_device(fac), torch.from_numpy(tau).cuda(), capi.to_device(B2)
    torch.cuda.synchronize()
    hip.call("capi_dormqr", capi.LEFT, capi.TRANS, m, r2, n, capi.ptr(dA), m, capi.ptr(dtau), capi.ptr(dB2), m)
    hip.call("capi_dtrsm_thin", capi.NOTRANS, n, r2, capi.ptr(dA), m, 0, capi.ptr(dB2), m)
    hip.sync()
    _assert_rule(f"{what} second set", capi.to_host(dB2)[:n], x2, eta2)


def test_without_norms_and_square(hip, oracle):
    """colnorm2 == NULL: the same X bit for bit.  m == n: zeros in colnorm2"""
    A, B, x_true, eta_h = _problem(2048, 64, 3, 1e4, 1.0)
    a = _gels(hip, A, B)
    b = _gels(hip, A, B, norms=False)
    assert b[0] == 0 and b[1] == 0 and np.array_equal(_bits(a[4]), _bits(b[4]))
    rng = np.random.default_rng(64)
    S = np.asfortranarray(rng.standard_normal((64, 64)) + 8.0 * np.eye(64))
    xs = rng.standard_normal((64, 2))
    rc, info, _, _, out, cn2 = _gels(hip, S, np.asfortranarray(S @ xs))
    assert rc == 0 and info == 0 and np.array_equal(cn2, np.zeros(2))
    _check("square 64", np.abs(out - xs).max() / np.abs(xs).max(), 1e-11)


@functools.lru_cache(maxsize=None)
def _singular():
    A, B, _, _ = _problem(2048, 64, 3, 1e1, 0.0)
    A = A.copy(order="F")
    A[:, 40] = 0.0
    A.setflags(write=False)
    return A, B


def test_exactly_singular(hip, oracle):
    """column 40 zero: it stays zero under H_1 .. H_40, R(41, 41) == 0 exactly: info 41, B left as Q^T B, colnorm2 untouched"""
    A, B = _singular()
    rc, info, fac, tau, out, cn2 = _gels(hip, A, B)
    assert rc == 0 and info == 41
    assert np.array_equal(cn2, np.full(3, FILL))
    _check("singular: B = Q^T B", np.abs(out - ref.ormqr(fac, tau, B, True)).max() / np.abs(B).max())


def test_refuses_wide(hip, oracle):
    import torch
    from capital_amd import capi
    A = np.asfortranarray(np.random.default_rng(5).random((40, 50)))
    B = np.asfortranarray(np.random.default_rng(6).random((50, 2)))
    dA, dB = capi.to_device(A), capi.to_device(B)
    dtau = torch.full((50,), FILL, dtype=torch.float64, device="cuda")
    dn = torch.full((2,), FILL, dtype=torch.float64, device="cuda")
    info = ctypes.c_int(-99)
    torch.cuda.synchronize()
    rc = hip.L.capi_dgels(hip.h, 40, 50, 2, capi.ptr(dA), 40, capi.ptr(dtau), capi.ptr(dB), 50, capi.ptr(dn), ctypes.byref(info))
    hip.sync()
    print(rc, hip.L.capi_last_error(hip.h).decode())
    assert rc == -1 and info.value == -99
    assert np.array_equal(_bits(capi.to_host(dA)), _bits(A)) and np.array_equal(_bits(capi.to_host(dB)), _bits(B))
    assert np.all(dtau.cpu().numpy() == FILL) and np.all(dn.cpu().numpy() == FILL)


def test_hqr(hip, oracle):
    from capital_amd import capi
    from capital_amd.hqr import Hqr
    A, B, x_true, eta_h = _problem(2048, 64, 3, 1e4, 1.0)
    _, _, fac, _, out, cn2 = _gels(hip, A, B)
    q = Hqr(hip, A)
    X, res = q.lstsq(B)
    assert np.array_equal(_bits(X), _bits(out[:64])) and np.array_equal(_bits(res), _bits(np.sqrt(cn2)))
    X2, res2 = q.lstsq(B)                                  # on the factors: capi_dormqr + capi_dtrsm_thin, the same kernels in the same order
    assert np.array_equal(_bits(X2), _bits(X)) and np.array_equal(_bits(res2), _bits(res))
    assert np.array_equal(_bits(q.R()), _bits(np.triu(fac[:64])))
    back = q.apply_q(q.apply_qt(B))
    _check("Hqr: Q (Q^T B)", np.abs(back - B).max() / np.abs(B).max())
    q.close()
    As, Bs = _singular()
    q = Hqr(hip, As)
    with pytest.raises(capi.CapiError, match="column 41"):
        q.lstsq(Bs)
    with pytest.raises(capi.CapiError, match="column 41"):
        q.lstsq(Bs)
    q.close()
