"""capi_dlr_diag, capi_drow_pow and capi_ddiag_add (capital_amd/csrc/lowrank_f64.hip) through the C-ABI against numpy.

capi_drow_pow is compiled without fused multiply-adds and the header states its order of operations, so powers +1 and -1 are compared BIT FOR BIT with
alpha * (x * d) + beta * y and alpha * (x / d) + beta * y as numpy rounds them; power -1/2 (w = 1 / sqrt(d) once per row, t = x w) is held to 2 ulp of
x / sqrt(d).  Shapes: 33 x 9 with ldx = 36, ldy = 40 (the 16-byte form, an odd last row), the same on an allocation that is only 8-byte aligned and with odd
leading dimensions (the 8-byte form), 700 x 166 (two row tiles, 21 column tiles of 8, a ragged last pass), 300 x 1, 1 x 1, and 700 x 3 in the 8-byte form
(rows tid and tid + 256 over two row tiles).  Every buffer carries guard words, and the padding rows of Y a NaN sentinel that must survive."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EINVAL = -1
U64 = 2.0 ** -53
LD = np.longdouble
SENTINEL = -7777.25


def dev(host):
    import torch
    return torch.from_numpy(np.ascontiguousarray(host)).cuda()


class Buf:
    """`count` doubles, `off` doubles into a buffer filled with SENTINEL, seven guard words behind them (tests/test_gpu_equil_kernels.py's Buf)"""

    def __init__(self, start, off=4):
        start = np.ascontiguousarray(start, dtype=np.float64).reshape(-1)
        self.m, self.off = len(start), off
        host = np.full(self.off + self.m + 7, SENTINEL)
        host[self.off:self.off + self.m] = start
        self.t = dev(host)

    @property
    def ptr(self):
        return self.t.data_ptr() + 8 * self.off

    def get(self):
        host = self.t.cpu().numpy()
        assert np.all(host[:self.off] == SENTINEL) and np.all(host[self.off + self.m:] == SENTINEL), "a guard word was written"
        return host[self.off:self.off + self.m].copy()


def column_major(M, ld, fill):
    """M (m x k) in column-major storage with leading dimension ld, the padding rows holding `fill`: the flat array"""
    m, k = M.shape
    full = np.full((ld, k), fill)
    full[:m] = M
    return full.T.reshape(-1)


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---- capi_dlr_diag ----
def lr_diag(hip, n, shift, diag, schur):
    dg = Buf(diag) if diag is not None else None
    sc = Buf(schur) if schur is not None else None
    d, rec = Buf(np.full(n, np.nan)), Buf(np.full(4, np.nan))
    hip.call("capi_dlr_diag", n, float(shift), dg.ptr if dg else None, sc.ptr if sc else None, d.ptr, rec.ptr)
    hip.sync()
    return d.get(), rec.get()


@pytest.mark.parametrize("n", [1, 33, 700])
def test_lr_diag_matches_numpy(hip, n):
    rng = np.random.default_rng(n)
    diag = 10.0 ** rng.uniform(-6, 2, n)
    schur = np.where(rng.random(n) < 0.3, 0.0, 10.0 ** rng.uniform(-12, 0, n))
    shift = 0.37e-3
    for dv, sv in ((None, None), (diag, None), (None, schur), (diag, schur)):
        d, rec = lr_diag(hip, n, shift, dv, sv)
        want = np.full(n, shift)
        if dv is not None:
            want = want + dv
        if sv is not None:
            want = want + sv
        assert same_bytes(d, want), (n, dv is not None, sv is not None)
        logs = np.log(want.astype(LD))
        err = abs(float(rec[0] - logs.sum())) / float(np.abs(logs).sum())
        print(f"lr_diag n={n} diag={dv is not None} schur={sv is not None}: sum log d {rec[0]:.15e}, relative error {err:.2e}")
        assert err <= 1e-13
        assert rec[1] == want.min() and rec[2] == want.max() and rec[3] == 0.0
        again = lr_diag(hip, n, shift, dv, sv)
        assert same_bytes(again[0], d) and same_bytes(again[1], rec)                  # one fixed order of the sum


@pytest.mark.parametrize("value", [0.0, -3.0, np.nan, np.inf], ids=["zero", "negative", "nan", "inf"])
def test_lr_diag_names_the_first_bad_entry(hip, value):
    n = 2500                                                                         # more than two rounds of the workgroup's 1024 threads
    good = 10.0 ** np.random.default_rng(7).uniform(-8, 8, n)
    for where in ([0], [n // 2], [n - 1], [2200, 1030, 17 + 1024, 2400]):
        x = good.copy()
        x[where] = value
        d, rec = lr_diag(hip, n, 0.0, x, None)
        assert rec[3] == min(where) + 1, (where, rec)
    # a bad sum: shift + diag is fine, the Schur entry makes it -inf
    s = np.zeros(n)
    s[1500] = -np.inf
    assert lr_diag(hip, n, 1.0, good, s)[1][3] == 1501


# ---- capi_drow_pow ----
# (m, r, ldx, ldy, off): off = 4 is a 16-byte aligned block, off = 3 one that is only 8-byte aligned
SHAPES = [(33, 9, 36, 40, 4), (33, 9, 36, 40, 3), (33, 9, 37, 39, 4), (700, 166, 700, 700, 4), (300, 1, 300, 300, 4), (1, 1, 1, 1, 4), (700, 3, 701, 703, 4)]


def row_pow(hip, m, r, power, d, alpha, X, ldx, beta, Y, ldy, norms=True):
    nrm = Buf(np.full(r, np.nan)) if norms else None
    hip.call("capi_drow_pow", m, r, float(power), d.ptr, float(alpha), X.ptr, ldx, float(beta), Y.ptr, ldy, nrm.ptr if norms else None)
    hip.sync()
    return nrm.get() if norms else None


def restate(power, d, alpha, X, beta, Y):
    """the header's order of operations"""
    dc = d[:, None]
    t = X * dc if power == 1.0 else (X / dc if power == -1.0 else X * (1.0 / np.sqrt(dc)))
    a = alpha * t
    return a + beta * Y if beta != 0.0 else a


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize("power", [1.0, -1.0, -0.5])
def test_row_pow(hip, shape, power):
    m, r, ldx, ldy, off = shape
    rng = np.random.default_rng(m * 1000 + r)
    dv = 10.0 ** rng.uniform(-6, 3, m)
    X, Y0 = rng.standard_normal((m, r)), rng.standard_normal((m, r))
    d = Buf(dv)
    for alpha, beta in ((1.0, 0.0), (-1.0, 1.0), (0.7, -1.3)):
        want = restate(power, dv, alpha, X, beta, Y0)
        src = Buf(column_major(X, ldx, np.nan), off=off)
        # beta == 0: Y is not read -- it is full of NaN; the padding rows hold a NaN sentinel in every case
        dst = Buf(column_major(Y0 if beta != 0.0 else np.full((m, r), np.nan), ldy, np.nan), off=off)
        nrm = row_pow(hip, m, r, power, d, alpha, src, ldx, beta, dst, ldy)
        got_flat = dst.get()
        got = got_flat.reshape(r, ldy).T[:m]
        assert np.all(np.isnan(got_flat.reshape(r, ldy).T[m:])), "a padding row of Y was written"
        assert same_bytes(src.get(), column_major(X, ldx, np.nan))
        assert np.all(np.isfinite(got))
        if power == -0.5:
            # w = 1 / sqrt(d) and t = x w carry three roundings where x / sqrt(d) carries two: 2 ulp; alpha t + beta y adds its own two roundings
            t = (X.astype(LD) / np.sqrt(dv.astype(LD))[:, None])
            exact = alpha * t + (beta * Y0.astype(LD) if beta != 0.0 else 0)
            slack = 2 * np.spacing(np.abs(alpha * t).astype(np.float64)) + (2 * U64 * (np.abs(alpha * t) + np.abs(beta * Y0)) if beta != 0.0 else 0)
            assert np.all(np.abs(got.astype(LD) - exact) <= slack), (shape, alpha, beta)
            print(f"row_pow {shape} power -1/2 alpha {alpha} beta {beta}: equal to numpy's x * (1 / sqrt(d)) form bit for bit: {same_bytes(got, want)}")
        else:
            assert same_bytes(got, want), (shape, power, alpha, beta, float(np.max(np.abs(got - want))))
        exact = (got.astype(LD) ** 2).sum(axis=0)
        err = np.abs(nrm.astype(LD) - exact) / np.where(exact > 0, exact, 1)
        assert np.all(err <= 1e-13), (shape, float(err.max()))
        # two calls give the same bytes
        dst2 = Buf(column_major(Y0 if beta != 0.0 else np.full((m, r), np.nan), ldy, np.nan), off=off)
        nrm2 = row_pow(hip, m, r, power, d, alpha, src, ldx, beta, dst2, ldy)
        assert same_bytes(dst2.get()[~np.isnan(got_flat)], got_flat[~np.isnan(got_flat)]) and same_bytes(nrm2, nrm)
        # Y == X, without norms: nothing but Y is written
        io = Buf(column_major(X, ldx, np.nan), off=off)
        row_pow(hip, m, r, power, d, alpha, io, ldx, beta, io, ldx, norms=False)
        alias = io.get().reshape(r, ldx).T
        want_alias = restate(power, dv, alpha, X, beta, X)
        assert np.all(np.isnan(alias[m:]))
        if power == -0.5:
            assert np.all(np.abs(alias[:m] - want_alias) <= 8 * U64 * (np.abs(alpha * X / np.sqrt(dv)[:, None]) + np.abs(beta * X)))
        else:
            assert same_bytes(alias[:m], want_alias), (shape, power, alpha, beta)
    d.get()


def test_row_pow_a_nan_shows_in_its_own_norm_alone(hip):
    m, r = 10, 5
    X = np.ones((m, r))
    X[4, r - 1] = np.nan
    d, io, nrm = Buf(np.full(m, 4.0)), Buf(column_major(X, m, 0.0)), Buf(np.full(r, 7.0))
    hip.call("capi_drow_pow", m, r, -0.5, d.ptr, 1.0, io.ptr, m, 0.0, io.ptr, m, nrm.ptr)
    hip.sync()
    got = nrm.get()
    assert np.isnan(got[r - 1]) and np.all(got[:r - 1] == 0.25 * m)


# ---- capi_ddiag_add ----
@pytest.mark.parametrize("n", [1, 33, 300])
def test_diag_add_touches_the_diagonal_alone(hip, n):
    ldc = n + 3
    C0 = np.random.default_rng(n).standard_normal((n, n))
    C0[np.tril_indices(n, -1)] = np.nan                                              # off-diagonal bytes of every kind
    buf = Buf(column_major(C0, ldc, np.nan))
    hip.call("capi_ddiag_add", n, 1.0, buf.ptr, ldc)
    hip.sync()
    want = C0.copy()
    want[np.arange(n), np.arange(n)] = np.diag(C0) + 1.0
    assert same_bytes(buf.get(), column_major(want, ldc, np.nan))


def test_conventions_and_refusals(hip):
    m, r = 40, 3
    rng = np.random.default_rng(3)
    X0 = rng.standard_normal(m * r)
    X, Y, d = Buf(X0), Buf(np.full(m * r, 5.0)), Buf(np.full(m, 2.0))
    nrm, rec = Buf(np.full(r, 5.0)), Buf(np.full(4, 5.0))
    L = hip.L
    pw = L.capi_drow_pow
    for args in ((m, r, 2.0, d.ptr, 1.0, X.ptr, m, 0.0, Y.ptr, m, nrm.ptr), (m, r, 0.5, d.ptr, 1.0, X.ptr, m, 0.0, Y.ptr, m, nrm.ptr),
                 (m, r, float("nan"), d.ptr, 1.0, X.ptr, m, 0.0, Y.ptr, m, nrm.ptr), (-1, r, 1.0, d.ptr, 1.0, X.ptr, m, 0.0, Y.ptr, m, nrm.ptr),
                 (m, -1, 1.0, d.ptr, 1.0, X.ptr, m, 0.0, Y.ptr, m, nrm.ptr), (m, r, 1.0, None, 1.0, X.ptr, m, 0.0, Y.ptr, m, nrm.ptr),
                 (m, r, 1.0, d.ptr, 1.0, None, m, 0.0, Y.ptr, m, nrm.ptr), (m, r, 1.0, d.ptr, 1.0, X.ptr, m, 0.0, None, m, nrm.ptr),
                 (m, r, -1.0, d.ptr, 1.0, X.ptr, m - 1, 0.0, Y.ptr, m, nrm.ptr), (m, r, -1.0, d.ptr, 1.0, X.ptr, m, 0.0, Y.ptr, m - 1, nrm.ptr),
                 (m, r, 1.0, d.ptr, 1.0, X.ptr, m, 0.0, X.ptr, m + 2, nrm.ptr)):
        assert pw(hip.h, *args) == EINVAL, args
    # a size of 0 is a no-op, with or without pointers; a power out of range is refused even then
    assert pw(hip.h, 0, r, 1.0, None, 1.0, None, 1, 0.0, None, 1, None) == 0
    assert pw(hip.h, m, 0, -0.5, None, 1.0, None, m, 0.0, None, m, None) == 0
    assert pw(hip.h, m, 0, 2.0, None, 1.0, None, m, 0.0, None, m, None) == EINVAL
    assert L.capi_dlr_diag(hip.h, -1, 1.0, None, None, d.ptr, rec.ptr) == EINVAL
    assert L.capi_dlr_diag(hip.h, m, 1.0, None, None, None, rec.ptr) == EINVAL
    assert L.capi_dlr_diag(hip.h, m, 1.0, None, None, d.ptr, None) == EINVAL
    assert L.capi_dlr_diag(hip.h, 0, 1.0, None, None, None, None) == 0
    assert L.capi_ddiag_add(hip.h, -1, 1.0, Y.ptr, m) == EINVAL
    assert L.capi_ddiag_add(hip.h, 3, 1.0, None, m) == EINVAL
    assert L.capi_ddiag_add(hip.h, 3, 1.0, Y.ptr, 2) == EINVAL
    assert L.capi_ddiag_add(hip.h, 0, 1.0, None, 1) == 0
    hip.sync()
    assert same_bytes(X.get(), X0) and np.all(Y.get() == 5.0) and np.all(d.get() == 2.0) and np.all(nrm.get() == 5.0) and np.all(rec.get() == 5.0)
