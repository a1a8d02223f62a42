"""capi_dchud / capi_dchud_inv (the rank-r update and downdate of an upper triangular factor and of its inverse; capital_amd/csrc/chud_f64.hip and
the schedule of chud_plan.h) on the GPU, against the criteria of the update:

    factor    rho = ||T'^T T' - A1||_F / ||A_big||_F <= 32 max(rho_ref, u), rho_ref the same figure for scipy.linalg.cholesky(A1)
    inverse   ||Tinv' T' - I||_F <= 16 max(eps0, eps1, n u), eps_i that of SciPy's factor and solve_triangular inverse of A_i

(tests/_chud_ref.py has the inputs and the bounds; tests/test_chud_host.py shows that the formulas reach them in NumPy.)  In every storage the call may
touch nothing but the triangle: NaN below the diagonal and in the padding rows, the rest of a larger packed triangle and the words around the buffers
must come back as the same bytes."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import _chud_ref as ref
import _conditioning as cond
from test_gpu_tri_thin import EINVAL, dev, pstart

pytestmark = pytest.mark.gpu

NS = [1, 2, 31, 33, 64, 65, 257, 1000]
RS = [1, 2, 17, 32]
STORES = ["ld", "ld+3", "packed", "view37"]
SENTINEL = -7777.25


@functools.lru_cache(maxsize=None)
def case(n, r, sign):
    """(A0, V, A1, R0, Rinv0, factor bound, inverse bound), computed once and never written"""
    A0, V, A1 = ref.problem(n, r, sign)
    R0 = np.asfortranarray(ref.chol_upper(A0))
    out = (A0, V, A1, R0, np.asfortranarray(ref.tri_inv(R0)), ref.factor_bound(A0, A1), ref.inverse_bound(A0, A1))
    for a in out[:5]:
        a.setflags(write=False)
    return out


class Tri:
    """an upper triangle on the device as `store` says, with NaN (rect) or other numbers (the larger packed triangle) wherever the call must not look"""

    def __init__(self, U, store, fill=np.nan):
        n = self.n = U.shape[0]
        self.store = store
        if store in ("packed", "view37"):
            c0 = self.col0 = 37 if store == "view37" else 0
            N = c0 + n + (5 if c0 else 0)
            host = np.random.default_rng(N).standard_normal(1 + pstart(N) + 1)
            host[0] = host[-1] = np.nan                                     # a NaN word in front of and behind the triangle
            self.mask = np.ones(host.shape, bool)
            for j in range(n):
                s = 1 + pstart(c0 + j) + c0
                host[s:s + j + 1] = U[:j + 1, j]
                self.mask[s:s + j + 1] = False
            self.ldt, self.off = 0, 1 + pstart(c0) + c0
        else:
            ld = self.ldt = n + (3 if store == "ld+3" else 0)
            self.col0, self.off = 0, 0
            full = np.full((ld, n), fill)
            full[:n, :] = np.where(np.arange(n)[:, None] <= np.arange(n)[None, :], U, fill)
            host = full.T.reshape(-1).copy()
            m = np.ones((ld, n), bool)
            m[:n, :] = np.arange(n)[:, None] > np.arange(n)[None, :]
            self.mask = m.T.reshape(-1).copy()
        self.before = host.copy()
        self.t = dev(host)

    @property
    def ptr(self):
        return self.t.data_ptr() + 8 * self.off

    def raw(self):
        return self.t.cpu().numpy()

    def get(self):
        """the triangle as a dense array (zeros below), after checking that every other word has the bytes it had"""
        host, n = self.raw(), self.n
        assert host[self.mask].tobytes() == self.before[self.mask].tobytes(), "something outside the triangle was written"
        U = np.zeros((n, n), order="F")
        for j in range(n):
            s = self.off + (pstart(self.col0 + j) - pstart(self.col0) if self.ldt == 0 else j * self.ldt)
            U[:j + 1, j] = host[s:s + j + 1]
        return U


class Buf:
    """`count` doubles on the device, three doubles into a sentinel-filled buffer"""

    def __init__(self, values, count=None):
        values = np.asarray(values, dtype=np.float64).reshape(-1)
        self.count = len(values) if count is None else count
        host = np.full(3 + self.count + 7, SENTINEL)
        host[3:3 + len(values)] = values
        self.t = dev(host)

    @property
    def ptr(self):
        return self.t.data_ptr() + 24

    def get(self):
        host = self.t.cpu().numpy()
        assert np.all(host[:3] == SENTINEL) and np.all(host[3 + self.count:] == SENTINEL), "something outside the buffer was written"
        return host[3:3 + self.count].copy()


def log_doubles(hip, n, r):
    b = hip.L.capi_dchud_log_bytes(n, r)
    assert b % 8 == 0 and b >= 8 * n * (r + 2)
    return b // 8


def chud(hip, sign, T, V, raw=False, r=None, n=None):
    """runs capi_dchud on the Tri T and the host V (n x r); returns (status, info, log buffer, V buffer)"""
    n = T.n if n is None else n
    r = V.shape[1] if r is None else r
    dV = Buf(np.asfortranarray(V).T.reshape(-1))
    lg = Buf(np.zeros(0), count=max(1, log_doubles(hip, n, min(max(r, 1), 32))))
    info = C.c_int(-99)
    rc = hip.L.capi_dchud(hip.h, sign, n, r, T.ptr, T.ldt, T.col0, dV.ptr, max(n, 1), lg.ptr, C.byref(info))
    hip.sync()
    if not raw:
        assert rc == 0, hip.L.capi_last_error(hip.h).decode()
    return rc, info.value, lg, dV


def chud_inv(hip, sign, r, Ti, lg, k0, k1):
    hip.call("capi_dchud_inv", sign, Ti.n, r, Ti.ptr, Ti.ldt, Ti.col0, lg.ptr, k0, k1)
    hip.sync()


CASES = list(itertools.product(NS, RS, (1, -1), STORES))


@pytest.mark.parametrize("n,r,sign,store", CASES, ids=[f"n{n}-r{r}-{'up' if s > 0 else 'down'}-{st}" for n, r, s, st in CASES])
def test_factor_and_inverse_criteria(hip, n, r, sign, store):
    A0, V, A1, R0, Ri0, rho_max, eps_max = case(n, r, sign)
    T, Ti = Tri(R0, store), Tri(Ri0, store)
    rc, info, lg, dV = chud(hip, sign, T, V)
    assert info == 0
    chud_inv(hip, sign, r, Ti, lg, 0, n)
    R1, Ri1 = T.get(), Ti.get()                                            # (get() checks that nothing outside the triangles was written)
    lg.get(), dV.get()
    assert (np.diag(R1) > 0).all()
    rho, eps = ref.factor_error(R1, A0, A1), ref.inverse_error(Ri1, R1)
    print(f"capi_dchud n={n} r={r} sign={sign:+d} {store}: rho {rho / ref.U64:.1f} u (bound {rho_max / ref.U64:.1f} u, {rho / (rho_max / 32):.2f} x ref), "
          f"||Tinv' T' - I|| {eps:.2e} (bound {eps_max:.2e}, {eps / (eps_max / 16):.2f} x ref)")
    assert rho <= rho_max
    assert eps <= eps_max


@pytest.mark.parametrize("store", ["ld+3", "view37"])
@pytest.mark.parametrize("sign", [1, -1], ids=["up", "down"])
@pytest.mark.parametrize("n,h1", [(33, 16), (1000, 500)])
def test_block_diagonal_inverse_in_two_ranges(hip, n, h1, sign, store):
    """the inverses of the two diagonal blocks, each against its own block of T'; the block between them holds a canary that must survive"""
    r = 17
    A0, V, A1, R0, Ri0, rho_max, eps_max = case(n, r, sign)
    Bi = np.zeros((n, n), order="F")
    Bi[:h1, :h1] = ref.tri_inv(R0[:h1, :h1])
    Bi[h1:, h1:] = ref.tri_inv(R0[h1:, h1:])
    Bi[:h1, h1:] = 7.25
    T, Ti = Tri(R0, store), Tri(Bi, store)
    rc, info, lg, dV = chud(hip, sign, T, V)
    assert info == 0
    chud_inv(hip, sign, r, Ti, lg, 0, h1)
    chud_inv(hip, sign, r, Ti, lg, h1, n)
    R1, out = T.get(), Ti.get()
    assert (out[:h1, h1:] == 7.25).all()
    for a, b in ((0, h1), (h1, n)):
        eps = ref.inverse_error(out[a:b, a:b], R1[a:b, a:b])
        print(f"capi_dchud_inv n={n} block [{a}, {b}) sign={sign:+d} {store}: {eps:.2e} (bound {eps_max:.2e})")
        assert eps <= eps_max


@pytest.mark.parametrize("store", STORES)
def test_two_runs_give_the_same_bytes(hip, store):
    n, r, sign = 257, 17, -1
    A0, V, A1, R0, Ri0, _, _ = case(n, r, sign)
    got = []
    for fill in (0.0, np.nan, np.nan):
        T, Ti = Tri(R0, store, fill), Tri(Ri0, store, fill)
        rc, info, lg, dV = chud(hip, sign, T, V)
        chud_inv(hip, sign, r, Ti, lg, 0, n)
        got.append((T.get().tobytes(), Ti.get().tobytes(), lg.get()[:n * (r + 2)].tobytes(), info))
    assert got[0] == got[1] == got[2] and got[0][3] == 0                   # NaN below the diagonal: the same bits as zeros there; two runs: the same bits


def test_log_records_the_steps(hip):
    """x_k, alpha_k, beta_k per step, as the NumPy restatement has them (to rounding: the kernel takes the divisions as reciprocals)"""
    n, r, sign = 65, 2, 1
    A0, V, A1, R0, _, _, _ = case(n, r, sign)
    T = Tri(R0, "ld")
    rc, info, lg, dV = chud(hip, sign, T, V)
    want = ref.chud(R0, V, sign)[1]
    got = lg.get()[:n * (r + 2)].reshape(n, r + 2)
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 64 * n * ref.U64 * scale
    np.testing.assert_array_equal(got[:, r + 1], np.diag(T.get()))         # beta_k is the new diagonal


def test_argument_errors_touch_nothing(hip):
    n = 40
    A0, V33, _ = ref.problem(n, 33, 1)
    R0 = ref.chol_upper(A0)
    T = Tri(R0, "ld")
    for kw in (dict(r=33), dict(r=0)):
        rc, info, lg, dV = chud(hip, 1, T, V33, raw=True, **kw)
        assert rc == EINVAL and info == -99
        np.testing.assert_array_equal(T.get(), R0)
        np.testing.assert_array_equal(dV.get(), V33.T.reshape(-1))
    V = V33[:, :3]
    rc, info, lg, dV = chud(hip, 0, T, V, raw=True)                         # sign
    assert rc == EINVAL and info == -99
    dVb = Buf(V.T.reshape(-1))
    lgb = Buf(np.zeros(0), count=n * 5)
    info = C.c_int(-99)
    assert hip.L.capi_dchud(hip.h, 1, n, 3, T.ptr, n - 1, 0, dVb.ptr, n, lgb.ptr, C.byref(info)) == EINVAL       # ldt
    assert hip.L.capi_dchud(hip.h, 1, n, 3, T.ptr, n, 0, dVb.ptr, n - 1, lgb.ptr, C.byref(info)) == EINVAL       # ldv
    assert hip.L.capi_dchud(hip.h, 1, n, 3, T.ptr + 4, n, 0, dVb.ptr, n, lgb.ptr, C.byref(info)) == EINVAL       # alignment
    assert hip.L.capi_dchud_inv(hip.h, 1, n, 33, T.ptr, n, 0, lgb.ptr, 0, n) == EINVAL
    assert hip.L.capi_dchud_inv(hip.h, 1, n, 3, T.ptr, n, 0, lgb.ptr, 5, 4) == EINVAL
    assert hip.L.capi_dchud_inv(hip.h, 1, n, 3, T.ptr, n, 0, lgb.ptr, 0, n + 1) == EINVAL
    assert info.value == -99
    hip.sync()
    np.testing.assert_array_equal(T.get(), R0)
    np.testing.assert_array_equal(dVb.get(), V.T.reshape(-1))
    # n == 0 is OK, touches nothing and reports success
    assert hip.L.capi_dchud(hip.h, -1, 0, 3, None, 0, 0, None, 1, None, C.byref(info)) == 0 and info.value == 0
    assert hip.L.capi_dchud_inv(hip.h, -1, 0, 3, None, 0, 0, None, 0, 0) == 0
    assert hip.L.capi_dchud_inv(hip.h, 1, n, 3, T.ptr, n, 0, lgb.ptr, 7, 7) == 0                                  # an empty range
    assert hip.L.capi_dchud_log_bytes(n, 33) == 0 and hip.L.capi_dchud_log_bytes(-1, 3) == 0
    hip.sync()
    np.testing.assert_array_equal(T.get(), R0)


@pytest.mark.parametrize("store", ["ld", "packed"])
def test_exact_downdate_failure(hip, store):
    """T = I of order 64, V = 2 e_5: steps 1 .. 5 have x = 0 and change nothing, step 6 meets 1 - 4 < 0"""
    V = np.zeros((64, 1), order="F")
    V[5, 0] = 2.0
    T = Tri(np.eye(64), store)
    rc, info, lg, dV = chud(hip, -1, T, V)
    assert rc == 0 and info == 6
    np.testing.assert_array_equal(T.get()[:5], np.eye(64)[:5])             # the rows before the failing step are finished
    T = Tri(np.eye(64), store)
    rc, info, lg, dV = chud(hip, +1, T, V)                                   # the same V as an update: fine
    want = np.eye(64)
    want[5, 5] = np.sqrt(5.0)
    assert info == 0
    np.testing.assert_array_equal(T.get(), want)


def test_generic_downdate_failure(hip):
    """V = 1.001 sqrt(lambda_max) q_max: A - V V^T has a negative eigenvalue, so some step must stop; rounding may move it, its position is not asserted.
    The panels after the stop return at entry."""
    n = 257
    A = cond.f1_spectrum(n, 1e2)
    T = Tri(ref.chol_upper(A), "ld+3")
    rc, info, lg, dV = chud(hip, -1, T, ref.failing_v(A))
    assert rc == 0 and 1 <= info <= n
    T.get()                                                                # nothing outside the triangle was written
    # the handle goes on working: the next call starts from a clear flag
    A0, V, A1, R0, _, rho_max, _ = case(n, 1, 1)
    T = Tri(R0, "ld")
    assert chud(hip, 1, T, V)[1] == 0
    assert ref.factor_error(T.get(), A0, A1) <= rho_max
