"""capi_dormqr (csrc/qr_apply_f64.hip): Q^T C and Q C from a dgeqrf image without forming Q.

The reference is tests/_ormqr_ref.py's dorm2r in numpy on the ORACLE's dgeqrf image, so parity here does not depend on capi_dgeqrf.  Parity is 1e-12 of
max |C|, the tolerance of tests/test_gpu_householder_qr.py (the blocked scheme in numpy is within 3e-14 of LAPACK's dormqr).  Every comparison prints
err/tol before it asserts."""
import functools

import numpy as np
import pytest

import _ormqr_ref as ref

pytestmark = pytest.mark.gpu

TOL = 1e-12
FILL = 7.25
EINVAL = -1
SHAPES = [(1, 1), (33, 1), (64, 32), (97, 33), (64, 64), (700, 48), (2053, 70), (4096, 256)]
RS = [1, 5, 16, 17, 32]

_bits = lambda a: np.ascontiguousarray(a).view(np.int64)


def _check(what, err, tol=TOL):
    print(f"{what}: err/tol {err:.3e}/{tol:.1e} = {err / tol:.3f}")
    assert err <= tol, (what, err, tol)


def _padded(A, ld, fill=FILL):
    out = np.full((ld, A.shape[1]), fill, order="F")
    out[:A.shape[0]] = A
    return out


def _frozen(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs


@functools.lru_cache(maxsize=None)
def _case(m, n, kind="random"):
    """(the oracle's dgeqrf image of a seeded m x n matrix, its tau), read-only"""
    A = np.asfortranarray(np.random.default_rng(m * 1000 + n).random((m, n)) - 0.5)
    if kind == "zero_col":                                     # column 40 zero: tau[40] = 0
        A[:, 40] = 0.0
    elif kind == "e1":                                         # first column a multiple of e_1: H_0 = I
        A[:, 0] = 0.0
        A[0, 0] = -0.7
    else:
        assert kind == "random"
    return _frozen(*ref.image(A))


@functools.lru_cache(maxsize=None)
def _block(m, r):
    return _frozen(np.asfortranarray(np.random.default_rng(7 * m + r).standard_normal((m, r))))[0]


@functools.lru_cache(maxsize=None)
def _expected(m, n, r, trans, k=None, kind="random"):
    fac, tau = _case(m, n, kind)
    return _frozen(ref.ormqr(fac, tau, _block(m, r), trans, k))[0]


def _ormqr(hip, fac, tau, C, trans, k=None, lda=None, ldc=None, shift=0, side=0, null_c=False, null_tau=False, rc_only=False):
    """capi_dormqr on device copies: (return code, host image of A with its padding, host image of C with its padding).  shift: C starts that many
    doubles into its allocation (8-byte alignment only)."""
    import torch
    from capital_amd import capi
    m, r = C.shape
    k = fac.shape[1] if k is None else k
    lda = fac.shape[0] if lda is None else lda
    ldc = m if ldc is None else ldc
    dA = capi.to_device(_padded(fac, lda))
    dC = torch.full((shift + ldc * r,), FILL, dtype=torch.float64, device="cuda")
    dC[shift:] = torch.from_numpy(np.ascontiguousarray(_padded(C, ldc).T).ravel()).cuda()
    dtau = None if (null_tau or tau is None) else torch.from_numpy(np.array(tau, dtype=np.float64)).cuda()
    torch.cuda.synchronize()
    rc = hip.L.capi_dormqr(hip.h, side, 1 if trans else 0, m, r, k, capi.ptr(dA), lda, capi.ptr(dtau),
                           None if null_c else capi.ptr(dC) + 8 * shift, ldc)
    hip.sync()
    return rc, capi.to_host(dA), np.asfortranarray(dC[shift:].cpu().numpy().reshape(r, ldc).T), dC[:shift].cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. parity
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [True, False], ids=["QT", "Q"])
@pytest.mark.parametrize("m,k", SHAPES)
def test_parity(hip, oracle, m, k, trans):
    fac, tau = _case(m, k)
    for r in RS:
        C = _block(m, r)
        rc, _, out, _ = _ormqr(hip, fac, tau, C, trans)
        assert rc == 0
        _check(f"{m}x{k} r={r} {'Q^T' if trans else 'Q'}", np.abs(out - _expected(m, k, r, trans)).max() / np.abs(C).max())


@pytest.mark.parametrize("trans", [True, False], ids=["QT", "Q"])
def test_many_row_slices_ragged_last_tile(hip, oracle, trans):
    m, k, r = 40000, 32, 3
    fac, tau = _case(m, k)
    C = _block(m, r)
    rc, _, out, _ = _ormqr(hip, fac, tau, C, trans)
    assert rc == 0
    _check(f"{m}x{k} r={r}", np.abs(out - _expected(m, k, r, trans)).max() / np.abs(C).max())


# ---------------------------------------------------------------------------------------------------------------------------
# 2. padded and unaligned layouts
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [True, False], ids=["QT", "Q"])
@pytest.mark.parametrize("m,k,r", [(700, 48, 5), (2053, 70, 17), (700, 48, 40)])
def test_padded_and_unaligned(hip, oracle, m, k, r, trans):
    """lda = m + 3, ldc = m + 5 (odd: the 8-byte path), C one double into its allocation: parity, the padding rows and the double in front keep
    their fill bit for bit, A comes back bit for bit"""
    fac, tau = _case(m, k)
    C = _block(m, r)
    rc, outA, out, front = _ormqr(hip, fac, tau, C, trans, lda=m + 3, ldc=m + 5, shift=1)
    assert rc == 0
    _check(f"padded {m}x{k} r={r}", np.abs(out[:m] - _expected(m, k, r, trans)).max() / np.abs(C).max())
    assert np.array_equal(_bits(out[m:]), _bits(np.full((5, r), FILL)))
    assert np.array_equal(_bits(front), _bits(np.full(1, FILL)))
    assert np.array_equal(_bits(outA), _bits(_padded(fac, m + 3)))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. nothing on or above A's diagonal takes part
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [True, False], ids=["QT", "Q"])
@pytest.mark.parametrize("m,k,r", [(700, 48, 5), (97, 33, 32), (700, 48, 40)])
def test_nan_in_place_of_r_changes_no_bit(hip, oracle, m, k, r, trans):
    fac, tau = _case(m, k)
    poisoned = fac.copy(order="F")
    iu = np.triu_indices(k, 0, k)
    poisoned[iu] = np.nan
    C = _block(m, r)
    rc1, _, clean, _ = _ormqr(hip, fac, tau, C, trans)
    rc2, _, masked, _ = _ormqr(hip, poisoned, tau, C, trans)
    assert rc1 == 0 and rc2 == 0
    assert np.isfinite(masked).all()
    assert np.array_equal(_bits(masked), _bits(clean))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. fewer reflectors than columns; tau = 0
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [True, False], ids=["QT", "Q"])
def test_fewer_reflectors(hip, oracle, trans):
    m, n, k, r = 700, 48, 20, 5
    fac, tau = _case(m, n)
    C = _block(m, r)
    rc, _, out, _ = _ormqr(hip, fac, tau, C, trans, k=k)
    assert rc == 0
    _check(f"k={k} of {n}", np.abs(out - _expected(m, n, r, trans, k)).max() / np.abs(C).max())


@pytest.mark.parametrize("trans", [True, False], ids=["QT", "Q"])
@pytest.mark.parametrize("kind", ["zero_col", "e1"])
def test_identity_reflectors(hip, oracle, kind, trans):
    m, n, r = 300, 96, 5
    fac, tau = _case(m, n, kind)
    assert tau[40 if kind == "zero_col" else 0] == 0.0
    C = _block(m, r)
    rc, _, out, _ = _ormqr(hip, fac, tau, C, trans)
    assert rc == 0
    _check(f"{kind}", np.abs(out - _expected(m, n, r, trans, None, kind)).max() / np.abs(C).max())


# ---------------------------------------------------------------------------------------------------------------------------
# 5. round trip
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,k,r", [(2053, 70, 17), (4096, 256, 32), (700, 48, 40)])
def test_round_trip(hip, oracle, m, k, r):
    fac, tau = _case(m, k)
    C = _block(m, r)
    rc, _, qtc, _ = _ormqr(hip, fac, tau, C, True)
    assert rc == 0
    rc, _, back, _ = _ormqr(hip, fac, tau, qtc, False)
    assert rc == 0
    _check(f"Q (Q^T C) {m}x{k} r={r}", np.abs(back - C).max() / np.abs(C).max())
    nC, nQ = np.linalg.norm(C.astype(np.longdouble)), np.linalg.norm(qtc.astype(np.longdouble))
    _check(f"||Q^T C||_F {m}x{k} r={r}", float(abs(nQ - nC) / nC))


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the wide path
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [True, False], ids=["QT", "Q"])
@pytest.mark.parametrize("m,k", [(700, 48), (2053, 70)])
def test_wide_path(hip, oracle, m, k, trans):
    fac, tau = _case(m, k)
    outs = {}
    for r in (33, 40):
        C = _block(m, r)
        rc, _, outs[r], _ = _ormqr(hip, fac, tau, C, trans)
        assert rc == 0
        _check(f"wide {m}x{k} r={r}", np.abs(outs[r] - _expected(m, k, r, trans)).max() / np.abs(C).max())
    C33 = _block(m, 33)
    rc, _, thin, _ = _ormqr(hip, fac, tau, np.asfortranarray(C33[:, :32]), trans)
    assert rc == 0
    _check(f"wide against thin {m}x{k}", np.abs(outs[33][:, :32] - thin).max() / np.abs(C33).max())


# ---------------------------------------------------------------------------------------------------------------------------
# 7. bit reproducibility
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [True, False], ids=["QT", "Q"])
@pytest.mark.parametrize("m,k,r", [(4096, 256, 32), (40000, 32, 3), (2053, 70, 40)])
def test_bit_reproducible(hip, oracle, m, k, r, trans):
    fac, tau = _case(m, k)
    C = _block(m, r)
    a = _ormqr(hip, fac, tau, C, trans)[2]
    b = _ormqr(hip, fac, tau, C, trans)[2]
    assert np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------------
# 8. refusals and empty problems
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["right", "k>m", "lda<m", "ldc<m", "null-C"])
def test_refusals(hip, oracle, what):
    m, n, r = 97, 33, 5
    fac, tau = _case(m, n)
    C = _block(m, r)
    if what == "right":
        rc, outA, out, _ = _ormqr(hip, fac, tau, C, True, side=1)
    elif what == "k>m":
        wide = np.asfortranarray(np.hstack([fac] * 3))[:, :98]
        rc, outA, out, _ = _ormqr(hip, wide, np.resize(tau, 98), C, True, k=98)
        fac = wide
    elif what == "lda<m":
        import torch
        from capital_amd import capi
        dA, dC, dtau = capi.to_device(fac), capi.to_device(C), torch.from_numpy(np.array(tau)).cuda()
        torch.cuda.synchronize()
        rc = hip.L.capi_dormqr(hip.h, 0, 1, m, r, n, capi.ptr(dA), m - 1, capi.ptr(dtau), capi.ptr(dC), m)
        hip.sync()
        outA, out = capi.to_host(dA), capi.to_host(dC)
    elif what == "ldc<m":
        import torch
        from capital_amd import capi
        dA, dC, dtau = capi.to_device(fac), capi.to_device(C), torch.from_numpy(np.array(tau)).cuda()
        torch.cuda.synchronize()
        rc = hip.L.capi_dormqr(hip.h, 0, 1, m, r, n, capi.ptr(dA), m, capi.ptr(dtau), capi.ptr(dC), m - 1)
        hip.sync()
        outA, out = capi.to_host(dA), capi.to_host(dC)
    else:
        rc, outA, out, _ = _ormqr(hip, fac, tau, C, True, null_c=True)
    print(what, rc, hip.L.capi_last_error(hip.h).decode())
    assert rc == EINVAL
    assert np.array_equal(_bits(out), _bits(C)) and np.array_equal(_bits(outA), _bits(fac))


def test_empty_problems(hip, oracle):
    m, n = 97, 33
    fac, tau = _case(m, n)
    C = _block(m, 5)
    rc, _, out, _ = _ormqr(hip, fac, tau, C, True, k=0, null_tau=True)
    assert rc == 0 and np.array_equal(_bits(out), _bits(C))
    import torch
    from capital_amd import capi
    dA, dC, dtau = capi.to_device(fac), capi.to_device(C), torch.from_numpy(np.array(tau)).cuda()
    torch.cuda.synchronize()
    assert hip.L.capi_dormqr(hip.h, 0, 1, m, 0, n, capi.ptr(dA), m, capi.ptr(dtau), capi.ptr(dC), m) == 0
    hip.sync()
    assert np.array_equal(_bits(capi.to_host(dC)), _bits(C))


# ---------------------------------------------------------------------------------------------------------------------------
# 9. the handle's info word
# ---------------------------------------------------------------------------------------------------------------------------
def test_pending_info_survives(hip, oracle):
    from capital_amd import capi
    n0 = 150
    S = oracle.distribute_symmetric(n0, n0, 0, 0, 1, 1)
    S[100, 100] = -5.0
    dS, dX = capi.to_device(S), capi.zeros(n0, n0)
    hip.call("capi_reset_info")
    try:
        hip.call("capi_dpotrf_trtri", n0, capi.ptr(dS), n0, capi.ptr(dX), n0)
        assert hip.info() == 101
        for r in (5, 40):
            fac, tau = _case(700, 48)
            rc, _, out, _ = _ormqr(hip, fac, tau, _block(700, r), True)
            assert rc == 0 and hip.info() == 101, r
            _check(f"pending info r={r}", np.abs(out - _expected(700, 48, r, True)).max() / np.abs(_block(700, r)).max())
    finally:
        hip.call("capi_reset_info")
    assert hip.info() == 0
