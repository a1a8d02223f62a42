"""capi_dgeqrf / capi_dorgqr (csrc/qr_f64.hip) where tests/test_gpu_lapack.py does not go: padded leading dimensions, widths off the
32 grid and the gates of the tall path, dorgqr with k < n, the slot cap of the column reductions, bit reproducibility, tau = 0 and
rank deficiency, conditioning either side of the 1e6 switch, the borrowed info word, and the Householder panels at tall shapes.

"Parity" is what the tests over there mean by it: R (relative to max |R|), the stored reflectors and tau against the oracle's
column-by-column dgeqr2 on the unpadded matrix, each to 1e-12; capi_dorgqr against the oracle's dorg2r on the same reflectors, 1e-12.
Every comparison prints err/tol before it asserts."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _conditioning import U64, orthogonal

pytestmark = pytest.mark.gpu

TOL = 1e-12
CB = 10.0            # eta_gpu <= CB max(eta_ref, u): the rule, and the constant, of tests/test_gpu_conditioning.py
FILL = 7.25


def _padded(A, ld, fill):
    """A on top of ld - m rows of `fill`: the device image is column-major with leading dimension ld."""
    m = A.shape[0]
    out = np.full((ld, A.shape[1]), fill, order="F")
    out[:m] = A
    return out


_bits = lambda a: np.ascontiguousarray(a).view(np.int64)


def _frozen(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs


def _random(m, n):
    return np.asfortranarray(np.random.default_rng(m * 1000 + n).random((m, n)) - 0.5)


def _reference(A):
    """(A, the oracle's dgeqr2 image of it, its tau), read-only: shared between the tests"""
    import oracle
    ref = A.copy(order="F")
    tau = oracle.dgeqrf(ref)
    return _frozen(A, ref, tau)


@functools.lru_cache(maxsize=None)
def _case(m, n, kind="random"):
    A = _random(m, n)
    if kind == "zero_col":                                     # column 40 zero: rank n - 1, tau[40] = 0
        A[:, 40] = 0.0
    elif kind == "dup_col":                                    # column 50 a copy of column 10
        A[:, 50] = A[:, 10]
    elif kind == "e1":                                         # first column a multiple of e_1: H_0 = I
        A[:, 0] = 0.0
        A[0, 0] = -0.7
    elif kind == "trapezoid":                                  # [T; 0], T upper triangular and well conditioned, diagonal of both signs
        rng = np.random.default_rng(m + n)
        T = 0.2 * np.triu(rng.random((n, n)) - 0.5, 1) + np.diag(np.where(rng.random(n) < 0.5, -1.0, 1.0) * (0.5 + rng.random(n)))
        A[:] = 0.0
        A[:n] = T
    else:
        assert kind == "random"
    return _reference(A)


def _geqrf(hip, A, lda=None):
    """capi_dgeqrf on A with leading dimension lda (rows m.. hold FILL): (device image, the whole host image, tau)"""
    import torch
    from capital_amd import capi
    m, n = A.shape
    lda = m if lda is None else lda
    dA = capi.to_device(_padded(A, lda, FILL))
    dtau = torch.zeros(min(m, n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    hip.call("capi_dgeqrf", m, n, capi.ptr(dA), lda, capi.ptr(dtau))
    hip.sync()
    return dA, capi.to_host(dA), dtau.cpu().numpy()


def _orgqr(hip, fac, tau, n_out, k, lda=None):
    """capi_dorgqr(m, n_out, k) on the first n_out columns of the geqrf image fac (m rows): the whole host image"""
    import torch
    from capital_amd import capi
    m = fac.shape[0]
    lda = m if lda is None else lda
    dA = capi.to_device(_padded(fac[:, :n_out], lda, FILL))
    dtau = None if tau is None else torch.from_numpy(np.array(tau, dtype=np.float64)).cuda()
    torch.cuda.synchronize()
    hip.call("capi_dorgqr", m, n_out, k, capi.ptr(dA), lda, capi.ptr(dtau))
    hip.sync()
    return capi.to_host(dA)


def _check(what, err, tol=TOL):
    print(f"{what}: err/tol {err:.3e}/{tol:.1e} = {err / tol:.3f}")
    assert err <= tol, (what, err, tol)


def _geqrf_errors(out, tau, ref, tau_ref):
    k = min(ref.shape)
    Rref = np.triu(ref[:k])
    return (np.abs(np.triu(out[:k]) - Rref).max() / np.abs(Rref).max(), np.abs(np.tril(out, -1) - np.tril(ref, -1)).max(),
            np.abs(tau - tau_ref).max())


def _assert_geqrf_parity(what, out, tau, ref, tau_ref):
    eR, eV, eT = _geqrf_errors(out, tau, ref, tau_ref)
    _check(f"{what} R", eR)
    _check(f"{what} reflectors", eV)
    _check(f"{what} tau", eT)


def _assert_orgqr_parity(what, oracle, Q, fac, tau, n_out, k):
    ref = np.asfortranarray(fac[:, :n_out]).copy(order="F")
    oracle.dorgqr(ref, np.ascontiguousarray(tau[:k]), k)
    _check(f"{what} dorgqr k={k}", np.abs(Q - ref).max())


def _identity(m, n):
    E = np.zeros((m, n), order="F")
    E[np.arange(n), np.arange(n)] = 1.0
    return E


# ---------------------------------------------------------------------------------------------------------------------------
# 1. padded leading dimension
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(100, 37), (300, 96), (33, 70), (2600, 40), (20011, 96)])
def test_padded_leading_dimension(hip, oracle, m, n):
    """lda = m + 3 on the column path, the wide shape and both tall routines (2600 x 40: a ragged last LU block as well): parity, and
    the three rows between m and lda come back bit for bit from geqrf and from dorgqr"""
    A, ref, tau_ref = _case(m, n)
    lda = m + 3
    pad = _bits(np.full((3, n), FILL))
    _, out, tau = _geqrf(hip, A, lda)
    _assert_geqrf_parity(f"lda {m}x{n}", out[:m], tau, ref, tau_ref)
    assert np.array_equal(_bits(out[m:]), pad)
    if m < n:
        return
    Q = _orgqr(hip, out[:m], tau, n, n, lda)
    _assert_orgqr_parity(f"lda {m}x{n}", oracle, Q[:m], out[:m], tau, n, n)
    assert np.array_equal(_bits(Q[m:]), pad)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. tall widths off the 32 grid, and the gates n >= 32, m >= 64 n
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(64 * 32 + 5, 32), (64 * 33 + 5, 33), (64 * 40 + 5, 40), (64 * 100 + 5, 100), (64 * 250 + 5, 250),
                                 (2048, 32), (2047, 32), (64 * 31 + 5, 31)])
def test_tall_widths_and_gates(hip, oracle, m, n):
    """n mod 32 in {0, 1, 8, 4, 26}: the last LU panel of the reconstruction is narrower than 32 and its dtrsm strip 32 x (n mod 32);
    m = 64 n and 64 n - 1, n = 32 and 31: either side of both gates.  The output is LAPACK's on both sides."""
    A, ref, tau_ref = _case(m, n)
    _, out, tau = _geqrf(hip, A)
    _assert_geqrf_parity(f"tall {m}x{n}", out, tau, ref, tau_ref)
    Q = _orgqr(hip, out, tau, n, n)
    _assert_orgqr_parity(f"tall {m}x{n}", oracle, Q, out, tau, n, n)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. dorgqr with k < n
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fac300(hip):
    _, out, tau = _geqrf(hip, _case(300, 96)[0])
    return _frozen(out, tau)


@pytest.mark.parametrize("n_out,k", [(96, 0), (96, 1), (96, 31), (96, 32), (96, 33), (96, 64), (96, 95), (50, 20)])
def test_orgqr_fewer_reflectors(hip, oracle, fac300, n_out, k):
    """Q = H_1 ... H_k [I; 0] for k < n: a short last block reflector (k mod 32 = 1, 31), whole blocks only (32, 64), fewer columns
    than geqrf factored (50), and k = 0 with tau == NULL, which must give [I; 0] exactly"""
    fac, tau = fac300
    Q = _orgqr(hip, fac, tau if k else None, n_out, k)
    _assert_orgqr_parity(f"300x{n_out}", oracle, Q, fac, tau, n_out, k)
    if k == 0:
        assert np.array_equal(Q, _identity(300, n_out))


def test_orgqr_fewer_reflectors_tall(hip, oracle):
    """k = 64 of 96 on a tall shape: the one-block routine applies all n reflectors, so k != n must take the panels"""
    m, n, k = 20011, 96, 64
    _, ref, tau_ref = _case(m, n)
    Q = _orgqr(hip, ref, tau_ref, n, k)
    _assert_orgqr_parity(f"{m}x{n}", oracle, Q, ref, tau_ref, n, k)


@pytest.mark.parametrize("m,n,k,dlda,null_tau,says", [(50, 60, 10, 0, False, "dims"), (60, 50, 51, 0, False, "dims"),
                                                      (60, 50, 10, -1, False, "operands"), (60, 50, 10, 0, True, "operands")],
                         ids=["n>m", "k>n", "lda<m", "null-tau"])
def test_orgqr_argument_errors(hip, m, n, k, dlda, null_tau, says):
    """invalid arguments: a nonzero return code, a message behind capi_last_error, and nothing launched -- A comes back bit for bit"""
    import torch
    from capital_amd import capi
    A = np.asfortranarray(np.random.default_rng(m + n + k).random((max(m, n), max(m, n))) - 0.5)
    dA = capi.to_device(A)
    dtau = torch.full((max(m, n),), 0.5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc =hip.L.capi_dorgqr(hip.h, m, n, k, capi.ptr(dA), m + dlda, None if null_tau else capi.ptr(dtau))
    msg = hip.L.capi_last_error(hip.h).decode()
    print(rc, msg)
    assert rc != 0
    assert "qr_f64" in msg and f"invalid argument: {says}" in msg
    hip.sync()
    assert np.array_equal(_bits(capi.to_host(dA)), _bits(A))
    assert np.all(dtau.cpu().numpy() == 0.5)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the slot cap of the column reductions
# ---------------------------------------------------------------------------------------------------------------------------
def test_slot_cap(hip, oracle):
    """rows > 1024 * 1024: nslots() stops at QPART = 1024 workgroups, each striding over more than 1024 rows.  n = 8 < 32 keeps this
    tall shape on the column path.  R and tau at 1e-12 (sums over 1e6 rows round to about sqrt(m) u = 1e-13), Q = dorgqr by the rule of
    the conditioning tests, and a second run bit for bit."""
    m, n = 1024 * 1024 + 4097, 8
    A, ref, tau_ref = _case(m, n)
    _, out, tau = _geqrf(hip, A)
    eR, eV, eT = _geqrf_errors(out, tau, ref, tau_ref)
    print(f"slot cap {m}x{n} reflectors (not asserted): err/tol {eV:.3e}/{TOL:.1e}")
    _check(f"slot cap {m}x{n} R", eR)
    _check(f"slot cap {m}x{n} tau", eT)
    Q = _orgqr(hip, out, tau, n, n)
    Qref = ref.copy(order="F")
    oracle.dorgqr(Qref, tau_ref, n)
    _assert_ld_qr(f"slot cap {m}x{n}", oracle, A, Q, out, Qref, ref)
    _, out2, tau2 = _geqrf(hip, A)
    assert np.array_equal(_bits(out2), _bits(out)) and np.array_equal(_bits(tau2), _bits(tau))


def _assert_ld_qr(what, oracle, A, Q, fac, Qref, ref):
    """both numbers of oracle.ld_qr at most CB max(the oracle's own run, u)"""
    n = A.shape[1]
    R, Rref = np.asfortranarray(np.triu(fac[:n])), np.asfortranarray(np.triu(ref[:n]))
    orth, res = oracle.ld_qr(A, Q, R)
    orth_ref, res_ref = oracle.ld_qr(A, Qref, Rref)
    print(f"{what}: orth {orth:.3e} (ref {orth_ref:.3e}, ratio {orth / max(orth_ref, U64):.2f})  "
          f"res {res:.3e} (ref {res_ref:.3e}, ratio {res / max(res_ref, U64):.2f})")
    assert orth <= CB * max(orth_ref, U64), (what, orth, orth_ref)
    assert res <= CB * max(res_ref, U64), (what, res, res_ref)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. reproducibility
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(5000, 64), (20011, 96)])
def test_geqrf_is_bit_reproducible(hip, m, n):
    """the same input twice: the image and tau are bit-identical (fixed slots added in a fixed order; no atomics on either path)"""
    A = _case(m, n)[0]
    _, out1, tau1 = _geqrf(hip, A)
    _, out2, tau2 = _geqrf(hip, A)
    assert np.array_equal(_bits(out1), _bits(out2))
    assert np.array_equal(_bits(tau1), _bits(tau2))


# ---------------------------------------------------------------------------------------------------------------------------
# 6. rank deficiency and tau = 0
# ---------------------------------------------------------------------------------------------------------------------------
def test_zero_column(hip, oracle):
    """column 40 zero: it stays zero under H_1 .. H_40, so xnorm2 == 0 and tau[40] = 0 exactly, as in dlarfg"""
    A, ref, tau_ref = _case(300, 96, "zero_col")
    _, out, tau = _geqrf(hip, A)
    _assert_geqrf_parity("zero column 300x96", out, tau, ref, tau_ref)
    assert tau[40] == 0.0 and tau_ref[40] == 0.0


def test_upper_trapezoidal_input_is_left_alone(hip):
    """[T; 0]: every column is reduced already -- every tau is 0, A comes back bit for bit, and dorgqr gives [I; 0] exactly"""
    A = _case(300, 96, "trapezoid")[0]
    _, out, tau = _geqrf(hip, A)
    assert np.all(tau == 0.0)
    assert np.array_equal(_bits(out), _bits(A))
    Q = _orgqr(hip, out, tau, 96, 96)
    assert np.array_equal(Q, _identity(300, 96))


def test_duplicate_column(hip, oracle):
    """column 50 = column 10: what is left of it below the diagonal is rounding noise, so its reflector is arbitrary and elementwise
    parity ill-posed.  What must hold: the factorisation (ld_qr, by the rule of the conditioning tests), reflector entries at most
    1 in magnitude (dlarfg's pivot choice) and every tau in {0} or [1, 2]."""
    m, n = 300, 96
    A, ref, tau_ref = _case(m, n, "dup_col")
    _, out, tau = _geqrf(hip, A)
    Q = _orgqr(hip, out, tau, n, n)
    Qref = ref.copy(order="F")
    oracle.dorgqr(Qref, tau_ref, n)
    _assert_ld_qr("duplicate column 300x96", oracle, A, Q, out, Qref, ref)
    vmax = np.abs(np.tril(out, -1)).max()
    print(f"duplicate column: max |v| {vmax:.17g}  tau in [{tau.min():.6f}, {tau.max():.6f}]")
    assert vmax <= 1.0 + 1e-12
    assert np.all((tau == 0.0) | ((tau >= 1.0) & (tau <= 2.0)))


def test_zero_column_tall(hip, oracle):
    """6200 x 96 with column 40 zero: the Gram matrix is singular, its factorisation fails and the Householder panels must run --
    LAPACK's output with tau[40] = 0, the handle's info word back at 0, and dorgqr (the panels again: one tau is zero) at parity"""
    m, n = 6200, 96
    A, ref, tau_ref = _case(m, n, "zero_col")
    hip.call("capi_reset_info")
    _, out, tau = _geqrf(hip, A)
    assert hip.info() == 0
    _assert_geqrf_parity("zero column 6200x96", out, tau, ref, tau_ref)
    assert tau[40] == 0.0
    Q = _orgqr(hip, out, tau, n, n)
    _assert_orgqr_parity("zero column 6200x96", oracle, Q, out, tau, n, n)


@pytest.mark.parametrize("kind", ["e1", "trapezoid"])
def test_reduced_columns_tall(hip, oracle, kind):
    """6200 x 96 with column 0 = -0.7 e_1, and [T; 0]: well conditioned, so CholeskyQR2 + reconstruction runs.  Of the two valid
    reflectors of a column that is already reduced the output must hold dlarfg's -- tau = 0, the row of R as it was -- not
    I - 2 e_j e_j^T (tau = 2, the row negated): plain parity, as at m = 64 n - 1."""
    m, n = 6200, 96
    A, ref, tau_ref = _case(m, n, kind)
    assert tau_ref[0] == 0.0 and (kind == "e1" or np.all(tau_ref == 0.0))
    _, out, tau = _geqrf(hip, A)
    print(f"{kind}: tau[:4] {tau[:4]}  zero taus {int((tau == 0.0).sum())} (oracle {int((tau_ref == 0.0).sum())})")
    _assert_geqrf_parity(f"{kind} 6200x96", out, tau, ref, tau_ref)
    assert np.array_equal(tau == 0.0, tau_ref == 0.0)
    Q = _orgqr(hip, out, tau, n, n)
    _assert_orgqr_parity(f"{kind} 6200x96", oracle, Q, out, tau, n, n)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. conditioning at the switch (diagonal ratio of the first sweep's R at most 1e6)
# ---------------------------------------------------------------------------------------------------------------------------
def _f1_panel(m, n, kappa, seed):
    """A = U diag(sigma) V^T, sigma log-spaced 1 .. 1/kappa, U (m x n) with orthonormal columns, V Haar orthogonal"""
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((m, n)))
    V = orthogonal(n, rng)
    return np.asfortranarray((U * np.logspace(0, -np.log10(kappa), n)[None, :]) @ V.T)


def _graded_panel(m, n, exponent, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray((rng.random((m, n)) - 0.5) * np.logspace(0, -exponent, n)[None, :])


CONDITIONING = [("f1", 4096, 64, 1e3), ("f1", 4096, 64, 1e5), ("f1", 4096, 64, 1e7), ("f1", 4096, 64, 1e9),
                ("graded", 4096, 64, 5.9), ("graded", 4096, 64, 6.1), ("f1", 600, 200, 1e12)]


@pytest.mark.parametrize("family,m,n,par", CONDITIONING, ids=[f"{f}-{m}x{n}-{p:g}" for f, m, n, p in CONDITIONING])
def test_conditioning_at_the_switch(hip, oracle, family, m, n, par):
    """F1 panels (the first sweep's diagonal ratio is about kappa / 25: 1e7 reconstructs, 1e9 falls back), column-graded panels with
    ratio 10^5.9 and 10^6.1, and a 600 x 200 panel at kappa 1e12 on the column path.  Q = dorgqr(geqrf(A)) and R: orthogonality and
    residual in long double at most CB max(the oracle's Householder run, u), and the absolute bounds of test_geqrf_orgqr_properties.
    Elementwise parity on the graded panels only: on F1 the reflectors of the two algorithms differ by kappa u."""
    A = _f1_panel(m, n, par, seed=int(m + n + np.log10(par))) if family == "f1" else _graded_panel(m, n, par, seed=int(10 * par))
    _, ref, tau_ref = _reference(A)
    _, out, tau = _geqrf(hip, A)
    Q = _orgqr(hip, out, tau, n, n)
    Qref = ref.copy(order="F")
    oracle.dorgqr(Qref, tau_ref, n)
    what = f"{family} {m}x{n} {par:g}"
    R = np.triu(out[:n])
    e_orth, e_res = np.abs(Q.T @ Q - np.eye(n)).max(), np.abs(Q @ R - A).max()
    print(f"{what}: max |Q^T Q - I| {e_orth:.3e} /1e-13   max |Q R - A| {e_res:.3e} /{1e-13 * n * np.abs(A).max():.3e}")
    if family == "graded":
        _assert_geqrf_parity(what, out, tau, ref, tau_ref)
    else:
        print(f"{what} elementwise (not asserted): R %.3e reflectors %.3e tau %.3e" % _geqrf_errors(out, tau, ref, tau_ref))
    _assert_ld_qr(what, oracle, A, Q, out, Qref, ref)
    assert e_orth <= 1e-13
    assert e_res <= 1e-13 * n * np.abs(A).max()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. the info word the tall path borrows
# ---------------------------------------------------------------------------------------------------------------------------
def test_pending_info_survives_tall_geqrf(hip, oracle):
    """geqrf's tall path saves, resets and restores the handle's LAPACK info around its two Gram factorisations.  A caller's pending
    101 (capi_dpotrf_trtri on the non-SPD matrix of test_potrf_reports_non_spd) is still there after a reconstruction, and after a
    panel whose Gram factorisation fails and leaves its own info behind; both outputs are LAPACK's."""
    from capital_amd import capi
    n0 = 150
    S = oracle.distribute_symmetric(n0, n0, 0, 0, 1, 1)
    S[100, 100] = -5.0
    dS, dX = capi.to_device(S), capi.zeros(n0, n0)
    hip.call("capi_reset_info")
    try:
        hip.call("capi_dpotrf_trtri", n0, capi.ptr(dS), n0, capi.ptr(dX), n0)
        assert hip.info() == 101
        for kind in ("random", "zero_col"):
            A, ref, tau_ref = _case(6200, 96, kind)
            _, out, tau = _geqrf(hip, A)
            assert hip.info() == 101, kind
            _assert_geqrf_parity(f"pending info, {kind} 6200x96", out, tau, ref, tau_ref)
    finally:
        hip.call("capi_reset_info")
    assert hip.info() == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 9. the Householder panels at tall shapes
# ---------------------------------------------------------------------------------------------------------------------------
def test_panels_at_tall_shapes():
    """CAPI_GEQRF_NO_RECONSTRUCT is read once per process, so a child runs with it set: geqrf + dorgqr column by column on
    20011 x 96 and 16384 x 256 -- the path every fallback of the tall routines ends on -- against the oracle, 1e-12"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, "tests", "_gpu_geqrf_panels_main.py")],
                         env=dict(os.environ, CAPI_GEQRF_NO_RECONSTRUCT="1"), cwd=root, capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stderr[-2000:]
    rows = re.findall(r"^panels (\d+)x(\d+): R ([0-9.e+-]+) reflectors ([0-9.e+-]+) tau ([0-9.e+-]+) Q ([0-9.e+-]+)$", res.stdout, re.M)
    assert [(int(a), int(b)) for a, b, *_ in rows] == [(20011, 96), (16384, 256)], res.stdout[-2000:]
    for m, n, *errs in rows:
        for name, e in zip(("R", "reflectors", "tau", "Q"), errs):
            _check(f"panels {m}x{n} {name}", float(e))
