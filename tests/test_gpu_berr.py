"""capi_dberr (capital_amd/csrc/bounds_f64.hip): dporfs's two elementwise steps -- the componentwise backward error max_i |rho_i| / w_i with its guard
for tiny w_i, and the weights |rho| + (n + 1) eps w of the forward bound -- against a numpy restatement.  Entries are powers of two (or zero), so the
quotients are exact and so is (n + 1) eps w; the one rounding left is the sum |rho| + (n + 1) eps w, which a fused multiply-add and numpy's two
operations may round differently: equality to 2 ulp.  capi_dcolamax rides along."""
import numpy as np
import pytest

from test_gpu_resid_sym import EINVAL, In, Out, norms_out

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
TINY = np.finfo(np.float64).tiny


def restated(Rho, W):
    n = Rho.shape[0]
    safe1 = (n + 1) * TINY
    safe2 = safe1 / EPS
    a = np.abs(Rho)
    big = W > safe2
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(big, a / W, (a + safe1) / (W + safe1))
    wt = a + ((n + 1) * EPS) * W
    return q.max(axis=0), np.where(big, wt, wt + safe1)


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def operands(n, r, seed):
    rng = np.random.default_rng(seed)
    Rho = np.ldexp(rng.choice([-1.0, 1.0], (n, r)), rng.integers(-60, -20, (n, r)))
    W = np.ldexp(1.0, rng.integers(-30, 30, (n, r)))
    k = max(1, n // 16)
    for j in range(r):
        rows = rng.permutation(n)
        W[rows[:k], j] = 0.0                      # w = 0 and rho = 0: the quotient safe1 / safe1, not 0 / 0
        Rho[rows[:k], j] = 0.0
        W[rows[k:2 * k], j] = 0.0                 # w = 0, rho != 0: (|rho| + safe1) / safe1, huge and finite
        W[rows[2 * k:3 * k], j] = np.ldexp(1.0, rng.integers(-1020, -990, len(rows[2 * k:3 * k])))      # 0 < w < safe2
        Rho[rows[3 * k:4 * k], j] = 0.0           # rho = 0 over an ordinary w
    return np.asfortranarray(Rho), np.asfortranarray(W)


@pytest.mark.parametrize("n,r", [(1, 1), (255, 7), (256, 32), (257, 1), (1000, 17), (5000, 3)])
def test_against_the_restatement(hip, n, r):
    Rho, W = operands(n, r, 100 * n + r)
    assert (W[:, 0] == 0).any() or n == 1
    dR, dW, be = In(Rho, n + 3), Out(W), norms_out(r)
    hip.call("capi_dberr", n, r, dR.ptr, dR.ld, dW.ptr, dW.ld, be.ptr)
    hip.sync()
    ref_b, ref_w = restated(Rho, W)
    got_b, got_w = be.get()[:, 0], dW.get()
    assert np.all(np.isfinite(got_b)) and np.all(np.isfinite(got_w))
    print(f"dberr n={n} r={r}: berr {got_b.min():.3e} .. {got_b.max():.3e}, max ulps berr {ulps(got_b, ref_b).max():.1f} weights {ulps(got_w, ref_w).max():.1f}")
    assert ulps(got_b, ref_b).max() <= 2
    assert ulps(got_w, ref_w).max() <= 2
    # the column maxima of |Rho|, by capi_dcolamax
    mx = norms_out(r)
    hip.call("capi_dcolamax", n, r, dR.ptr, dR.ld, mx.ptr)
    hip.sync()
    np.testing.assert_array_equal(mx.get()[:, 0], np.abs(Rho).max(axis=0))


def test_ordinary_quotients_are_exact(hip):
    """no guard in play: berr is a quotient of two powers of two, the largest of the column"""
    n, r = 777, 5
    rng = np.random.default_rng(5)
    Rho = np.asfortranarray(np.ldexp(rng.choice([-1.0, 1.0], (n, r)), rng.integers(-60, -50, (n, r))))
    W = np.asfortranarray(np.ldexp(1.0, rng.integers(-3, 4, (n, r))))
    dR, dW, be = In(Rho), Out(W), norms_out(r)
    hip.call("capi_dberr", n, r, dR.ptr, dR.ld, dW.ptr, dW.ld, be.ptr)
    hip.sync()
    np.testing.assert_array_equal(be.get()[:, 0], (np.abs(Rho) / W).max(axis=0))


def test_too_many_columns_touch_nothing(hip):
    n = 40
    Rho, W = operands(n, 33, 1)
    for r in (33, 0):
        dW, be = Out(W), Out(np.full((33, 1), 5.0))
        dR = In(Rho)
        rc = hip.L.capi_dberr(hip.h, n, r, dR.ptr, dR.ld, dW.ptr, dW.ld, be.ptr)
        hip.sync()
        assert rc == EINVAL
        np.testing.assert_array_equal(dW.get(), W)
        np.testing.assert_array_equal(be.get()[:, 0], np.full(33, 5.0))
