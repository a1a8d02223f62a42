"""Shifted CholeskyQR (qr::cacqr with num_shifted > 0, capital_amd/src/alg/qr/cacqr/cacqr.h) on tall panels with kappa(A) = 1e10 and
1e12 -- beyond CholeskyQR2's 1e8 -- through driver.Cacqr, and its two n x n entry points alone through capi.

Bounds, as in tests/test_gpu_conditioning.py: orthogonality ||Q^T Q - I||_F and residual ||A - Q R||_F / ||A||_F in long double
(oracle.ld_qr), each <= C max(reference, u) with C = 10 and u = 2^-53 -- the margin of "same algorithm, another summation order".
`reference` is the larger of the figure of tests/_scqr_ref.py (the algorithm in numpy) and of Householder QR (numpy.linalg.qr) on the
same input.  The inputs leave the panel that enters the first plain sweep at cond <= 1e7, a factor ten inside CholeskyQR's limit."""
import functools

import numpy as np
import pytest

import _scqr_ref as ref
from _scqr_ref import U64

pytestmark = pytest.mark.gpu

CB = 10.0

# (m, n, kappa, num_iter, num_shifted, graded)
CASES = [(1 << 14, 256, 1e10, 3, 1, True), (1 << 16, 256, 1e10, 3, 1, False), (1 << 14, 1024, 1e10, 3, 1, True),
         (1 << 14, 256, 1e12, 4, 2, False), (1 << 16, 256, 1e12, 4, 2, True), (1 << 14, 1024, 1e12, 4, 2, False)]
IDS = [f"{m}x{n}-k{k:.0e}-{it}_{sh}-{'graded' if g else 'plain'}" for m, n, k, it, sh, g in CASES]


@functools.lru_cache(maxsize=2)
def _panel(m, n, kappa, graded):
    return ref.panel(m, n, kappa, seed=int(m + n + np.log10(kappa)), graded=graded)


@pytest.fixture(scope="module")
def drv():
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    yield driver
    driver.finalize()


def _run(drv, A, variant, shifted, **kw):
    q = drv.Cacqr(A.shape[0], A.shape[1], c=1, variant=variant, shifted=shifted, **kw)
    try:
        q.set_A(A)
        q.factor()
        return q.Q(), q.R(), (q.sweep_stats() if shifted else None)
    finally:
        q.close()


@pytest.mark.parametrize("m,n,kappa,num_iter,num_shifted,graded", CASES, ids=IDS)
def test_shifted_cqr_on_ill_conditioned_panels(drv, oracle, m, n, kappa, num_iter, num_shifted, graded):
    """orthogonality and residual against the numpy restatement and Householder QR; R upper triangular with a positive diagonal; the
    diagnostic tells the sweeps apart; and CholeskyQR2 on the same input still raises, naming the pivot."""
    A = _panel(m, n, kappa, graded)
    Q, R, stats = _run(drv, A, num_iter, num_shifted)
    Qs, Rs, stats_ref = ref.scqr(A, num_iter, num_shifted)
    Qh, Rh = np.linalg.qr(A)
    orth, res = oracle.ld_qr(A, Q, R)
    orth_s, res_s = oracle.ld_qr(A, Qs, Rs)
    orth_h, res_h = oracle.ld_qr(A, np.asfortranarray(Qh), np.asfortranarray(Rh))
    print(f"scqr {m}x{n} kappa={kappa:.0e} {num_iter}/{num_shifted} graded={graded}: orth {orth:.3e} (numpy {orth_s:.3e}, Householder {orth_h:.3e})  "
          f"res {res:.3e} (numpy {res_s:.3e}, Householder {res_h:.3e})")
    print("    cond_bound per sweep: " + ", ".join(f"{s['cond_bound']:.3e}" for s in stats) + "   numpy: " +
          ", ".join(f"{s['cond_bound']:.3e}" for s in stats_ref) + "   shifts: " + ", ".join(f"{s['shift']:.3e}" for s in stats))
    assert orth <= CB * max(orth_s, orth_h, U64), (orth, orth_s, orth_h)
    assert res <= CB * max(res_s, res_h, U64), (res, res_s, res_h)
    assert np.all(np.tril(R, -1) == 0) and np.all(np.diag(R) > 0)
    assert len(stats) == num_iter
    assert all(s["shift"] > 0 for s in stats[:num_shifted]) and all(s["shift"] == 0 for s in stats[num_shifted:])
    assert stats[-1]["cond_bound"] <= 4.0, stats
    if kappa >= 1e12:
        assert stats[0]["cond_bound"] >= 1e8, stats
    with pytest.raises(drv.DriverError, match=r"not positive definite \(pivot \d+\)"):
        _run(drv, A, 2, 0)


@pytest.mark.parametrize("m,n", [(16384, 256), (8192, 130)])
def test_scale_equivariance_shifted(drv, m, n):
    """3 / 1 on a kappa 1e10 panel and on the same panel with its columns scaled by powers of two: R(A D) = R(A) D and Q(A D) = Q(A),
    bit for bit.  An equilibration that rounds (log2, sqrt), or a shift taken on the unequilibrated Gram matrix, fails this."""
    A = ref.panel(m, n, 1e10, seed=n)
    e = ref.grading_exponents(n, seed=m, lo=-100, hi=100)
    Q0, R0, st0 = _run(drv, A, 3, 1)
    Q1, R1, st1 = _run(drv, np.asfortranarray(np.ldexp(A, e[None, :])), 3, 1)
    np.testing.assert_array_equal(Q1, Q0)
    np.testing.assert_array_equal(R1, np.ldexp(R0, e[None, :]))
    assert st0 == st1


@pytest.mark.parametrize("num_iter,num_shifted,kappa", [(3, 1, 1e10), (4, 2, 1e12)])
def test_panel32_intermediates_bit_identical(drv, num_iter, num_shifted, kappa, monkeypatch):
    """width 256, whole 32-row tiles: the run whose intermediate panels Q1, Q2 (, Q3) are panel32 images equals the column-major run"""
    A = _panel(1 << 14, 256, kappa, graded=(num_iter == 3))
    Qt, Rt, st_t = _run(drv, A, num_iter, num_shifted)
    monkeypatch.setenv("CAPITAL_NO_PANEL32", "1")
    Qc, Rc, st_c = _run(drv, A, num_iter, num_shifted)
    monkeypatch.delenv("CAPITAL_NO_PANEL32")
    np.testing.assert_array_equal(Qt, Qc)
    np.testing.assert_array_equal(Rt, Rc)
    assert st_t == st_c


def test_plain_three_and_four_sweeps(drv, oracle):
    """num_shifted == 0: variant 3 and 4 run that many plain sweeps (Q stays orthonormal, R = R_k .. R_1 reproduces A)"""
    A = ref.panel(8192, 64, 1e4, seed=5)
    for variant in (3, 4):
        Q, R, _ = _run(drv, A, variant, 0)
        Qs, Rs, _ = ref.scqr(A, variant, 0)
        orth, res = oracle.ld_qr(A, Q, R)
        orth_s, res_s = oracle.ld_qr(A, Qs, Rs)
        assert orth <= CB * max(orth_s, U64) and res <= CB * max(res_s, U64), (variant, orth, orth_s, res, res_s)


def test_set_shift_rejects_bad_arguments(drv):
    with pytest.raises(drv.DriverError, match="set_shift"):
        drv.Cacqr(4096, 32, variant=2, shifted=3)
    with pytest.raises(drv.DriverError, match="set_shift"):
        drv.Cacqr(4096, 32, variant=3, shifted=1, shift_scale=-1.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the two entry points alone
# ---------------------------------------------------------------------------------------------------------------------------------
def _dev(A, ld, fill=np.nan):
    from capital_amd import capi
    m, n = A.shape
    P = np.full((ld, n), fill, order="F")
    P[:m] = A
    return capi.to_device(P)


def _host(t, m):
    from capital_amd import capi
    return np.asfortranarray(capi.to_host(t)[:m])


def _gram(n, seed):
    """an SPD matrix with a graded diagonal (exponents over 2^-60 .. 2^60) and NaN below the diagonal"""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n + 8, n))
    G = B.T @ B
    e = rng.integers(-30, 31, n)
    G = np.ldexp(G, e[:, None] + e[None, :]) * rng.uniform(1.0, 4.0)
    G = np.triu(G)
    G[np.tril_indices(n, -1)] = np.nan
    return np.asfortranarray(G)


@pytest.mark.parametrize("n,pad", [(1, 0), (1, 3), (31, 1), (256, 0), (1000, 8), (1024, 0), (1024, 1)])
def test_equilibrate_shift_entry_point(hip, n, pad):
    """scales and the scaled off-diagonal entries exact, s and the trace (sums of n terms) to 4 n ulp; NaN below the diagonal of G and in
    the padding rows is neither read nor overwritten"""
    import torch
    from capital_amd import capi
    m_global, scale = 123457 * n + 11, 0.75
    G = _gram(n, n + pad)
    ld = n + pad
    dG = _dev(G, ld)
    dsc = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
    rec = torch.full((4,), np.nan, dtype=torch.float64, device="cuda")
    hip.call("capi_reset_info")
    hip.call("capi_dgram_equilibrate_shift", n, capi.ptr(dG), ld, m_global, scale, capi.ptr(dsc), capi.ptr(rec))
    assert hip.info() == 0
    Gp, d, s, tr, info = ref.equilibrate_shift(G, m_global, scale)
    assert info == 0
    got, r = _host(dG, n), rec.cpu().numpy()
    np.testing.assert_array_equal(dsc.cpu().numpy(), d)
    assert abs(r[1] - tr) <= 4 * n * np.spacing(tr), (r[1], tr)
    assert abs(r[0] - s) <= 4 * n * np.spacing(s), (r[0], s)
    up = np.triu(np.ones((n, n), bool), 1)
    np.testing.assert_array_equal(got[up], Gp[up])
    e = np.frexp(d)[1] - 1
    np.testing.assert_array_equal(np.diag(got), np.ldexp(np.diag(G), -2 * e) + r[0])   # the diagonal carries the GPU's own s
    assert np.isnan(got[np.tril_indices(n, -1)]).all()
    if pad:
        assert np.isnan(capi.to_host(dG)[n:]).all()


@pytest.mark.parametrize("n,pad", [(1, 0), (31, 1), (256, 0), (1000, 8), (1024, 0)])
def test_tri_rescale_entry_point(hip, n, pad):
    """R D and D^-1 X exact; the two norm products of the unscaled triangles (sums of at most n terms) to 4 n ulp; NaN below the diagonals is not read;
    dscale = NULL only takes the norms"""
    import torch
    from capital_amd import capi
    rng = np.random.default_rng(n)
    Rp = np.triu(rng.standard_normal((n, n))) + 2 * np.eye(n)
    Xp = np.triu(rng.standard_normal((n, n))) + 2 * np.eye(n)
    Rp[np.tril_indices(n, -1)] = np.nan
    Xp[np.tril_indices(n, -1)] = np.nan
    d = np.ldexp(1.0, rng.integers(-300, 301, n))
    ld = n + pad
    R, X, nr, nx = ref.tri_rescale(np.triu(Rp), np.triu(Xp), d)
    for dscale in (d, None):
        dR, dX = _dev(np.asfortranarray(Rp), ld), _dev(np.asfortranarray(Xp), ld)
        dd = torch.from_numpy(d).cuda()
        rec = torch.full((4,), np.nan, dtype=torch.float64, device="cuda")
        hip.call("capi_reset_info")
        hip.call("capi_dtri_rescale", n, capi.ptr(dR), ld, capi.ptr(dX), ld, capi.ptr(dd) if dscale is not None else None, capi.ptr(rec))
        assert hip.info() == 0
        gR, gX, r = _host(dR, n), _host(dX, n), rec.cpu().numpy()
        up = np.triu(np.ones((n, n), bool))
        np.testing.assert_array_equal(gR[up], (R if dscale is not None else Rp)[up])
        np.testing.assert_array_equal(gX[up], (X if dscale is not None else Xp)[up])
        assert np.isnan(gR[~up]).all() and np.isnan(gX[~up]).all()
        assert np.isnan(r[:2]).all()                                               # the first half of the record belongs to the other call
        assert abs(r[2] - nr) <= 4 * n * np.spacing(nr) and abs(r[3] - nx) <= 4 * n * np.spacing(nx), (r, nr, nx)


def test_entry_points_set_info(hip):
    """a zero, negative or non-finite diagonal entry of G sets info to its 1-based index (the first one); so does a scale that takes a
    diagonal entry of R or R^-1 out of the normal range"""
    import torch
    from capital_amd import capi
    n = 300
    G0 = np.triu(_gram(n, 3))
    for j, v in ((0, 0.0), (17, -1.0), (255, np.nan), (256, np.inf), (299, 0.0)):
        G = G0.copy(order="F")
        G[j, j] = v
        G[299, 299] = 0.0                                                          # a later one as well: the first is reported
        dG = _dev(G, n)
        dsc, rec = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(4, dtype=torch.float64, device="cuda")
        hip.call("capi_reset_info")
        hip.call("capi_dgram_equilibrate_shift", n, capi.ptr(dG), n, 1 << 20, 1.0, capi.ptr(dsc), capi.ptr(rec))
        assert hip.info() == j + 1, (j, v)
        assert ref.equilibrate_shift(G, 1 << 20)[4] == j + 1
    Rp = np.asfortranarray(np.eye(n) * 2.0 ** 600)
    Xp = np.asfortranarray(np.eye(n) * 2.0 ** -600)
    d = np.ones(n)
    d[41] = d[200] = 2.0 ** 500                                                    # 2^1100 overflows, 2^-1100 underflows
    dR, dX, dd = _dev(Rp, n), _dev(Xp, n), torch.from_numpy(d).cuda()
    rec = torch.empty(4, dtype=torch.float64, device="cuda")
    hip.call("capi_reset_info")
    hip.call("capi_dtri_rescale", n, capi.ptr(dR), n, capi.ptr(dX), n, capi.ptr(dd), capi.ptr(rec))
    assert hip.info() == 42
    hip.call("capi_reset_info")
