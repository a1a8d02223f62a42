"""capi_dgesvj (R = U diag(sigma) V^T for an upper triangular R by one-sided Jacobi on the device; capital_amd/csrc/svd_f64.hip and the pair schedule
of jacobi_plan.h) on the GPU, through the raw C-ABI.

R is the positive-diagonal R of numpy's QR of _scqr_ref.panel(64 n, n, kappa, seed); the orders are the smallest at which the schedule, the odd-n
rest, the reductions past one wave and past one 256-thread group and the sort can go wrong; n = 33 and n = 130 have padded leading dimensions;
everything below R's diagonal is NaN in every case.
The rule is DESIGN.md section 2a's, per metric: gpu <= 10 max(numpy.linalg.svd's value, the value of tests/_jacobi_ref.py, u) -- the GPU is never
compared with itself -- and, so that a restatement that mirrors a flaw cannot hide it, a cap: every metric <= 2e-11, the residual and the sigma
metric <= 1e-12 (10 x the worst values of the UNPOLISHED numpy restatement on these inputs: 1.8e-12, 1e-13 and 6e-14)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _jacobi_ref as jr
import _scqr_ref as ref
from _scqr_ref import U64

pytestmark = pytest.mark.gpu
EINVAL = -1
SENTINEL = -7777.25
NS = [1, 2, 3, 31, 32, 33, 64, 65, 130, 257]
KAPPAS = [1e2, 1e7, 1e12]
CASES = [(n, KAPPAS[i % 3]) for i, n in enumerate(NS)]
PADDED = {33: (3, 5, 1), 130: (6, 1, 3)}          # n -> what ldr, ldu, ldv exceed n by
NAMES = ("residual", "orthogonality of U", "orthogonality of V", "sigma")
CAPS = (1e-12, 2e-11, 2e-11, 1e-12)


@functools.lru_cache(maxsize=None)
def problem(n, kappa):
    """(R, sigma of numpy, metrics of numpy.linalg.svd, metrics of the numpy restatement), computed once and shared"""
    A = ref.panel(64 * n, n, kappa, n)
    R = np.linalg.qr(A, mode="r")
    R = np.asfortranarray(np.triu(R * np.where(np.diag(R) < 0.0, -1.0, 1.0)[:, None]))
    Un, sn, Vtn = np.linalg.svd(R)
    Uj, sj, Vj, sweeps = jr.jacobi_svd(R)
    assert 1 <= sweeps <= jr.MAX_SWEEPS
    for a in (R, sn):
        a.setflags(write=False)
    return R, sn, jr.metrics(R, Un, sn, Vtn.T, sn), jr.metrics(R, Uj, sj, Vj, sn)


class Block:
    """an l x c device block with leading dimension ld, in a sentinel-filled buffer"""

    def __init__(self, l, c, ld, fill=None):
        import torch
        self.l, self.c, self.ld = l, c, ld
        host = np.full((c, ld), SENTINEL)
        if fill is not None:
            host[:, :l] = fill.T
        self.t = torch.from_numpy(host).cuda()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def raw(self):
        return self.t.cpu().numpy()

    def get(self):
        host = self.raw()
        assert np.all(host[:, self.l:] == SENTINEL), "the padding rows were written"
        return np.asfortranarray(host[:, :self.l].T)


def place_R(R, ldr):
    """R with NaN below its diagonal (and SENTINEL in the padding rows)"""
    n = R.shape[0]
    return Block(n, n, ldr, np.where(np.arange(n)[:, None] <= np.arange(n)[None, :], R, np.nan))


def gesvj(hip, dR, n, want_u=True, want_v=True, ldu=None, ldv=None):
    ldu, ldv = ldu or n, ldv or n
    dU = Block(n, n, ldu) if want_u else None
    dV = Block(n, n, ldv) if want_v else None
    ds = Block(n, 1, n)
    sweeps = C.c_int(-99)
    hip.call("capi_dgesvj", n, dR.ptr, dR.ld, dU.ptr if want_u else None, ldu, ds.ptr, dV.ptr if want_v else None, ldv, C.byref(sweeps))
    hip.sync()
    return (dU.get() if want_u else None), ds.get()[:, 0], (dV.get() if want_v else None), sweeps.value


@pytest.mark.parametrize("n,kappa", CASES, ids=[f"n{n}-k{k:.0e}" for n, k in CASES])
def test_against_two_references(hip, n, kappa):
    R, sn, m_np, m_jr = problem(n, kappa)
    pr, pu, pv = PADDED.get(n, (0, 0, 0))
    dR = place_R(R, n + pr)
    before = dR.raw().copy()
    U, s, V, sweeps = gesvj(hip, dR, n, ldu=n + pu, ldv=n + pv)
    U2, s2, V2, sweeps2 = gesvj(hip, dR, n, ldu=n + pu, ldv=n + pv)
    _, s_v, V_v, _ = gesvj(hip, dR, n, want_u=False, ldv=n + pv)
    _, s_0, _, _ = gesvj(hip, dR, n, want_u=False, want_v=False)
    np.testing.assert_array_equal(dR.raw(), before)                         # R is not written (NaN == NaN here)
    m_gpu = jr.metrics(R, U, s, V, sn)
    print(f"gesvj n={n} kappa={kappa:.0e}: sweeps {sweeps}")
    for name, g, a, b in zip(NAMES, m_gpu, m_np, m_jr):
        print(f"  {name}: gpu {g:.3e}, numpy.linalg.svd {a:.3e}, numpy restatement {b:.3e}")
    assert 1 <= sweeps <= 30 and sweeps2 == sweeps
    assert np.all(np.isfinite(U)) and np.all(np.isfinite(V)) and np.all(s >= 0.0) and np.all(np.diff(s) <= 0.0)
    for name, g, a, b, cap in zip(NAMES, m_gpu, m_np, m_jr, CAPS):
        assert g <= 10.0 * max(a, b, U64), (name, g, a, b)
        assert g <= cap, (name, g, cap)
    for a, b in ((U2, U), (s2, s), (V2, V)):                                # two calls give identical bits
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(s_v, s)                                   # V alone and the values alone: the same sigma, bit for bit
    np.testing.assert_array_equal(s_0, s)
    np.testing.assert_array_equal(V_v, V)


def test_orders_out_of_range_touch_nothing(hip):
    R, _, _, _ = problem(3, KAPPAS[2])
    dR = place_R(R, 3)
    dU, dV, ds = Block(3, 3, 3), Block(3, 3, 3), Block(3, 1, 3)
    for n in (0, 2049, -1):
        sweeps = C.c_int(-99)
        rc = hip.L.capi_dgesvj(hip.h, n, dR.ptr, max(n, 3), dU.ptr, max(n, 3), ds.ptr, dV.ptr, max(n, 3), C.byref(sweeps))
        hip.sync()
        assert rc == EINVAL and sweeps.value == -99, (n, rc)
        for blk in (dU, dV, ds):
            assert np.all(blk.raw() == SENTINEL)
    # a leading dimension below n, and U aliasing V
    assert hip.L.capi_dgesvj(hip.h, 3, dR.ptr, 2, dU.ptr, 3, ds.ptr, dV.ptr, 3, C.byref(sweeps)) == EINVAL
    assert hip.L.capi_dgesvj(hip.h, 3, dR.ptr, 3, dU.ptr, 3, ds.ptr, dU.ptr, 3, C.byref(sweeps)) == EINVAL
