"""capi_dgeqp3 (csrc/qrcp_f64.hip): QR with column pivoting of a block of order <= 2048, against tests/_qrcp_ref.py, the numpy restatement of its step rule.

Parity cases (tests/_qrcp_ref.GEQP3_SHAPES, rtol = 0, full rank, kappa 10; the builder asserts a pivot gap at every step): jpvt and k equal; R, the
reflectors and tau elementwise to 1e-12 of max|R|, the project's parity bar; ||W P - Q R|| / ||W|| and ||Q^T Q - I|| by the project's rule
eta_gpu <= 10 max(eta_ref, u).  515 = 64 workgroups of 8 columns and 3 more; 17 = two workgroups and one column; one case with ldw = mr + 3.
Then the stop at a planted rank, a duplicated column, a zero matrix, a NaN, run-to-run identity and the refusals.  Every comparison prints err/tol
before it asserts."""
import ctypes

import numpy as np
import pytest

import _qrcp_ref as ref
from _qrcp_ref import U64

pytestmark = pytest.mark.gpu

TOL = 1e-12
CB = 10.0
FILL = 7.25

_bits = lambda a: np.ascontiguousarray(a).view(np.int64)


def _check(what, err, tol=TOL):
    print(f"{what}: err/tol {err:.3e}/{tol:.1e} = {err / tol:.3f}")
    assert err <= tol, (what, err, tol)


def _geqp3(hip, W, rtol, pad=0):
    """capi_dgeqp3 on a device copy with ldw = mr + pad: (rc, k, image, tau, jpvt, the padding rows on exit)"""
    import torch
    from capital_amd import capi
    mr, n = W.shape
    ld = mr + pad
    Wp = np.full((ld, n), FILL, order="F")
    Wp[:mr] = W
    dW = capi.to_device(Wp)
    dtau = torch.full((min(mr, n),), FILL, dtype=torch.float64, device="cuda")
    dj = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    k = ctypes.c_int(-99)
    torch.cuda.synchronize()
    rc = hip.L.capi_dgeqp3(hip.h, mr, n, capi.ptr(dW), ld, capi.ptr(dj), capi.ptr(dtau), rtol, ctypes.byref(k))
    hip.sync()
    out = capi.to_host(dW)
    return rc, k.value, np.asfortranarray(out[:mr]), dtau.cpu().numpy(), dj.cpu().numpy().astype(np.int64), out[mr:]


@pytest.mark.parametrize("mr,n,pad,seed", ref.GEQP3_SHAPES, ids=ref.GEQP3_IDS)
def test_parity_with_the_restatement(hip, mr, n, pad, seed):
    W, (image, tau, jpvt, k, _) = ref.geqp3_case(mr, n, seed)
    rc, kg, img, taug, jg, padrows = _geqp3(hip, W, 0.0, pad)
    assert rc == 0, hip.L.capi_last_error(hip.h).decode()
    assert kg == k and np.array_equal(jg, jpvt), (kg, k)
    assert np.all(padrows == FILL)
    scale = np.abs(np.triu(image)).max()
    _check(f"{mr}x{n} image (R and the reflectors)", np.abs(img - image).max() / scale)
    _check(f"{mr}x{n} tau", np.abs(taug - tau).max() / scale)
    e_fac, e_orth = ref.factor_errors(W, img, taug, jg, kg)
    r_fac, r_orth = ref.factor_errors(W, image, tau, jpvt, k)
    _check(f"{mr}x{n} ||W P - Q R|| / ||W|| (restatement {r_fac:.3e})", e_fac, CB * max(r_fac, U64))
    _check(f"{mr}x{n} ||Q^T Q - I|| (restatement {r_orth:.3e})", e_orth, CB * max(r_orth, U64))


@pytest.mark.parametrize("n,k,smin", [(64, 40, 1e-9), (130, 97, 1e-10)], ids=["64-rank40-1e-9", "130-rank97-1e-10"])
def test_planted_rank_stops_at_k(hip, n, k, smin):
    """triu of the R factor of a planted tall panel, rtol = 1e-13: rank k, the restatement's pivots, tau = 0 behind them, a remainder below rtol nu_0"""
    A = ref.planted(16 * n, n, k, smin, 1)[0]
    W = np.asfortranarray(np.triu(np.linalg.qr(A, mode="r")))
    image, tau, jpvt, kr, _ = ref.check_case(W, 1e-13, k)
    rc, kg, img, taug, jg, _ = _geqp3(hip, W, 1e-13)
    assert rc == 0 and kg == k == kr
    assert np.array_equal(jg[:k], jpvt[:k]) and sorted(jg) == list(range(n)) and np.array_equal(jg[k:], np.sort(jg[k:]))
    assert np.all(taug[k:] == 0.0)
    rem = np.sqrt((img[k:, k:] ** 2).sum(axis=0)).max()
    _check(f"{n} rank {k}: remainder / (rtol nu_0)", rem / abs(img[0, 0]), 1e-13 * (1.0 + 1e-6))
    e_fac, e_orth = ref.factor_errors(W, img, taug, jg, kg)
    r_fac, r_orth = ref.factor_errors(W, image, tau, jpvt, kr)
    _check(f"{n} rank {k} ||W P - Q R|| / ||W|| (restatement {r_fac:.3e})", e_fac, CB * max(r_fac, U64))
    _check(f"{n} rank {k} ||Q^T Q - I|| (restatement {r_orth:.3e})", e_orth, CB * max(r_orth, U64))
    d, dr = np.abs(np.diag(img))[:k], np.abs(np.diag(image))[:k]
    _check(f"{n} rank {k} |diag R| against the restatement, relative to r_00", np.abs(d - dr).max() / dr[0])


def test_duplicated_column_zero_matrix_and_nan(hip):
    rng = np.random.default_rng(3)
    W = np.asfortranarray(rng.standard_normal((40, 24)))
    W[:, 17] = W[:, 5]
    image, tau, jpvt, k, _ = ref.geqp3(W, 1e-13)
    rc, kg, img, taug, jg, _ = _geqp3(hip, W, 1e-13)
    assert rc == 0 and kg == k == 23
    assert np.array_equal(jg, jpvt) and list(jg).index(5) < 23 and jg[23] == 17          # the tie goes to the first index
    Z = np.zeros((33, 20), order="F")
    rc, kg, img, taug, jg, _ = _geqp3(hip, Z, -1.0)
    assert rc == 0 and kg == 0 and np.array_equal(jg, np.arange(20)) and np.all(taug == 0.0) and np.all(img == 0.0)
    W = np.asfortranarray(rng.standard_normal((70, 70)))
    W[11, 30] = np.nan
    rc, kg, img, taug, jg, _ = _geqp3(hip, W, 0.0)
    assert rc == 0 and 0 <= kg <= 70 and sorted(jg) == list(range(70))


def test_two_runs_give_identical_bytes(hip):
    W, _ = ref.geqp3_case(257, 257, 1)
    a = _geqp3(hip, W, 0.0)
    b = _geqp3(hip, W, 0.0)
    assert a[1] == b[1] and np.array_equal(a[4], b[4])
    assert np.array_equal(_bits(a[2]), _bits(b[2])) and np.array_equal(_bits(a[3]), _bits(b[3]))


def test_refusals_touch_nothing(hip):
    import torch
    from capital_amd import capi
    mr = n = 16
    dW = torch.full((n, mr), FILL, dtype=torch.float64, device="cuda")
    dtau = torch.full((n,), FILL, dtype=torch.float64, device="cuda")
    dj = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    W, t, j = capi.ptr(dW), capi.ptr(dtau), capi.ptr(dj)
    torch.cuda.synchronize()
    bad = [(mr, n, None, mr, j, t, 0.0), (mr, n, W, mr, None, t, 0.0), (mr, n, W, mr, j, None, 0.0), (mr, n, W, mr - 1, j, t, 0.0),
           (2049, n, W, 2049, j, t, 0.0), (mr, 2049, W, mr, j, t, 0.0), (-1, n, W, mr, j, t, 0.0), (mr, n, W, mr, j, t, float("nan")),
           (mr, n, W + 4, mr, j, t, 0.0)]
    for args in bad:
        k = ctypes.c_int(-99)
        rc = hip.L.capi_dgeqp3(hip.h, *args, ctypes.byref(k))
        assert rc == -1 and k.value == -99, args
    assert hip.L.capi_dgeqp3(hip.h, mr, n, W, mr, j, t, 0.0, None) == -1
    hip.sync()
    assert torch.all(dW == FILL) and torch.all(dtau == FILL) and torch.all(dj == -7)
    k = ctypes.c_int(-99)                                                                 # an empty problem: rank 0, nothing launched
    assert hip.L.capi_dgeqp3(hip.h, 0, n, W, 1, j, t, 0.0, ctypes.byref(k)) == 0 and k.value == 0
    hip.sync()
    assert torch.all(dW == FILL) and torch.all(dj == -7)
