"""capi_dpoequ2, capi_dsym_scale2 and capi_drow_scale2 (capital_amd/csrc/equil_f64.hip) through the C-ABI against the numpy restatement of the
exponent rule (tests/_equil_ref.py).  The scale factors are powers of two, so everything but the column norms is compared BIT FOR BIT.

Shapes: n = 1, 2, 31, 32, 33, 255, 256, 257, 1000 (one element; below, at and above a pass of 8 columns and a tile of 64; 1000: two row tiles, whole
tiles beside the tiles the diagonal crosses) with lda = n and n + 3 (odd and even leading dimensions both occur: the 16-byte and the 8-byte form), and
n = 1100 with an even lda on an allocation that is only 8-byte aligned; r = 1, 5, 32, 40.  Every buffer carries guard words.
Column norms: the squares are rounded once each and m non-negative terms summed in some fixed order: within (m + 1) u of the longdouble sum."""
import numpy as np
import pytest

import _conditioning as cond
import _equil_ref as ref

pytestmark = pytest.mark.gpu

EINVAL = -1
U64 = 2.0 ** -53
LD = np.longdouble
SENTINEL = -7777.25
NS = [1, 2, 31, 32, 33, 255, 256, 257, 1000]


def dev(host):
    import torch
    return torch.from_numpy(np.ascontiguousarray(host)).cuda()


class Buf:
    """`count` doubles, `off` doubles into a buffer filled with SENTINEL, seven guard words behind them (tests/test_gpu_tri_rownorm2.py's Out)"""

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


def graded_matrix(n, rng):
    """a symmetric matrix whose diagonal spans 16 decades, with its exponents"""
    C = rng.standard_normal((n, n))
    C = cond.symmetrize(C @ C.T / n + np.eye(n))
    D0 = 10.0 ** rng.uniform(-8, 8, n)
    A = cond.symmetrize(D0[:, None] * C * D0[None, :])
    return A, ref.exponents(np.diag(A))


def poequ2(hip, n, Aptr, lda, dscale0=None):
    ds = Buf(np.full(n, np.nan) if dscale0 is None else dscale0)
    rec = Buf(np.full(4, np.nan))
    hip.call("capi_dpoequ2", n, Aptr, lda, ds.ptr, rec.ptr)
    hip.sync()
    return ds.get(), rec.get()


@pytest.mark.parametrize("n", NS)
def test_poequ2_matches_the_restatement(hip, n):
    rng = np.random.default_rng(n)
    for pad in (0, 3):
        lda = n + pad
        A, _ = graded_matrix(n, rng)
        if n >= 31:                                                         # edge values on the diagonal: only the diagonal is read
            edges = np.array([np.finfo(np.float64).max, np.finfo(np.float64).tiny, 5e-324, 2.0 ** -1030, 2.0 ** 101, 2.0 ** 100, 1.0, np.nextafter(1.0, 0)])
            A[np.arange(8) * 3, np.arange(8) * 3] = edges
        full = np.full((lda, n), np.nan)                                    # NaN everywhere off the diagonal
        full[np.arange(n), np.arange(n)] = np.diag(A)
        dA = dev(full.T.reshape(-1))
        ds, rec = poequ2(hip, n, dA.data_ptr(), lda)
        want_ds, want_rec = ref.poequ2(np.diag(A))
        assert ds.tobytes() == want_ds.tobytes() and rec.tobytes() == want_rec.tobytes(), (n, lda, rec, want_rec)
        again = poequ2(hip, n, dA.data_ptr(), lda)
        assert again[0].tobytes() == ds.tobytes() and again[1].tobytes() == rec.tobytes()


@pytest.mark.parametrize("value", [0.0, -3.0, np.nan, np.inf], ids=["zero", "negative", "nan", "inf"])
def test_poequ2_bad_diagonal_entries(hip, value):
    n = 300
    d = 10.0 ** np.random.default_rng(7).uniform(-8, 8, n)
    for where in ([0], [n // 2], [n - 1], [200, 17, 250]):                  # the first bad entry wins
        x = d.copy()
        x[where] = value
        dA = dev(np.diag(x).reshape(-1))
        ds, rec = poequ2(hip, n, dA.data_ptr(), n)
        assert np.all(ds == 1.0) and rec[3] == min(where) + 1 and rec[0] == 1.0 and rec[1] == 0.0 and rec[2] == 0.0
        want_ds, want_rec = ref.poequ2(x)
        assert ds.tobytes() == want_ds.tobytes() and rec.tobytes() == want_rec.tobytes()


def sym_scale2(hip, n, Aptr, lda, dptr, sign, raw=False):
    if raw:
        rc = hip.L.capi_dsym_scale2(hip.h, n, Aptr, lda, dptr, sign)
        hip.sync()
        return rc
    hip.call("capi_dsym_scale2", n, Aptr, lda, dptr, sign)
    hip.sync()


def check_sym_scale(hip, n, lda, rng, lower, off=4):
    A, e = graded_matrix(n, rng)
    junk = rng.standard_normal((n, n)) * 1e300
    low = np.full((n, n), np.nan) if lower == "nan" else junk
    start = np.where(np.arange(n)[:, None] <= np.arange(n)[None, :], A, low)
    flat0 = column_major(start, lda, np.nan if lower == "nan" else SENTINEL)
    buf = Buf(flat0, off=off)
    ds = Buf(np.ldexp(1.0, e.astype(np.int32)))
    want = start.copy()
    iu = np.triu_indices(n)
    want[iu] = ref.sym_scale(A, e, 1)[iu]
    sym_scale2(hip, n, buf.ptr, lda, ds.ptr, 1)
    got = buf.get()
    assert got.tobytes() == column_major(want, lda, np.nan if lower == "nan" else SENTINEL).tobytes(), (n, lda, lower)
    d = got.reshape(n, lda)[np.arange(n), np.arange(n)]
    assert np.all((d >= 0.5) & (d < 2.0))
    sym_scale2(hip, n, buf.ptr, lda, ds.ptr, -1)                            # and back: every bit, the lower triangle and the padding included
    assert buf.get().tobytes() == flat0.tobytes(), (n, lda, lower)
    ds.get()


@pytest.mark.parametrize("n", NS)
def test_sym_scale2_scales_the_upper_triangle_alone(hip, n):
    rng = np.random.default_rng(100 + n)
    for pad in (0, 3):
        for lower in ("nan", "junk"):
            check_sym_scale(hip, n, n + pad, rng, lower)


def test_sym_scale2_even_lda_on_an_8_byte_aligned_block(hip):
    """lda even but A only 8-byte aligned: the 8-byte form; 1100: whole tiles and a ragged edge in both row tiles"""
    rng = np.random.default_rng(9)
    check_sym_scale(hip, 1100, 1100, rng, "nan", off=3)
    check_sym_scale(hip, 1100, 1102, rng, "junk", off=4)


def test_sym_scale2_passes_zero_inf_and_nan_through_and_rounds_once(hip):
    n = 40
    e = np.random.default_rng(2).integers(-30, 30, n)
    A = np.triu(np.ones((n, n)))
    A[0, 1], A[0, 2], A[0, 3], A[1, 4], A[2, 5] = 0.0, np.inf, np.nan, -np.inf, -0.0
    A[3, 6] = np.ldexp(1.0 + 2.0 ** -52, -1060 + int(e[3] + e[6]))         # lands below the normal range: one rounding, as np.ldexp
    buf = Buf(column_major(A, n, 0.0))
    ds = Buf(np.ldexp(1.0, e.astype(np.int32)))
    sym_scale2(hip, n, buf.ptr, n, ds.ptr, 1)
    want = np.triu(ref.sym_scale(A, e, 1))
    assert buf.get().tobytes() == column_major(want, n, 0.0).tobytes()
    # exponents at the ends of dscale's range: 2^512 and 2^-537 in one product of scale factors overflow as two multiplications; one addition does not
    e2 = np.array([512, -537, 512, -537])
    A2 = np.triu(np.ldexp(np.ones((4, 4)), (e2[:, None] + e2[None, :]).astype(np.int32).clip(-1074, 1023)))
    buf = Buf(column_major(A2, 4, 0.0))
    ds = Buf(np.ldexp(1.0, e2.astype(np.int32)))
    sym_scale2(hip, 4, buf.ptr, 4, ds.ptr, 1)
    assert buf.get().tobytes() == column_major(np.triu(ref.sym_scale(A2, e2, 1)), 4, 0.0).tobytes()


def test_amax_rule_a_tiny_matrix_has_scond_one(hip):
    """ldexp(C, -1000): scond = 1, and the host layer's rule scales it only because amax < SMALL"""
    n = 257
    C = cond.f1_spectrum(n, 1e2, seed=3)
    s = 1.0 / np.sqrt(np.diag(C))
    C = cond.symmetrize(0.75 * s[:, None] * C * s[None, :])                 # diagonal 0.75 (to rounding), inside [0.5, 1): one exponent
    assert np.all((np.diag(C) >= 0.5) & (np.diag(C) < 1.0))
    T = np.ldexp(C, -1000)
    buf = Buf(column_major(T, n, np.nan))
    ds, rec = poequ2(hip, n, buf.ptr, n)
    assert rec[0] == 1.0 and rec[1] == T.diagonal().max() and rec[1] < ref.SMALL and rec[3] == 0.0
    assert ref.scales_by_rule(rec[0], rec[1]) and not ref.scales_by_rule(rec[0], rec[1] * 2.0 ** 1000)
    dsb = Buf(ds)
    sym_scale2(hip, n, buf.ptr, n, dsb.ptr, 1)
    got = buf.get().reshape(n, n).T
    e = ref.exponents(np.diag(T))
    assert np.all(e == -500)
    assert np.triu(got).tobytes() == np.triu(ref.sym_scale(T, e, 1)).tobytes()

def test_conventions_and_refusals(hip):
    n = 40
    rng = np.random.default_rng(3)
    A, e = graded_matrix(n, rng)
    flat = column_major(A, n, 0.0)
    buf, ds = Buf(flat), Buf(np.ldexp(1.0, e.astype(np.int32)))
    rec = Buf(np.full(4, 5.0))
    for args in ((-1, buf.ptr, n, ds.ptr, 1), (n, buf.ptr, n - 1, ds.ptr, 1), (n, buf.ptr, n, ds.ptr, 0), (n, buf.ptr, n, ds.ptr, 2), (n, None, n, ds.ptr, 1),
                 (n, buf.ptr, n, None, -1)):
        assert sym_scale2(hip, *args, raw=True) == EINVAL
    assert sym_scale2(hip, 0, None, 1, None, 1, raw=True) == 0                # a size of 0 is a no-op
    assert buf.get().tobytes() == flat.tobytes()
    L = hip.L
    assert L.capi_dpoequ2(hip.h, -1, buf.ptr, n, ds.ptr, rec.ptr) == EINVAL
    assert L.capi_dpoequ2(hip.h, n, buf.ptr, n - 1, ds.ptr, rec.ptr) == EINVAL
    assert L.capi_dpoequ2(hip.h, n, None, n, ds.ptr, rec.ptr) == EINVAL
    assert L.capi_dpoequ2(hip.h, n, buf.ptr, n, None, rec.ptr) == EINVAL
    assert L.capi_dpoequ2(hip.h, n, buf.ptr, n, ds.ptr, None) == EINVAL
    assert L.capi_dpoequ2(hip.h, 0, None, 1, None, None) == 0
    X = Buf(rng.standard_normal(n * 2))
    for args in ((-1, 2, ds.ptr, 1, X.ptr, n, X.ptr, n, None), (n, -1, ds.ptr, 1, X.ptr, n, X.ptr, n, None), (n, 2, ds.ptr, 0, X.ptr, n, X.ptr, n, None),
                 (n, 2, None, 1, X.ptr, n, X.ptr, n, None), (n, 2, ds.ptr, 1, None, n, X.ptr, n, None), (n, 2, ds.ptr, 1, X.ptr, n, None, n, None),
                 (n, 2, ds.ptr, 1, X.ptr, n - 1, X.ptr, n, None), (n, 2, ds.ptr, 1, X.ptr, n, X.ptr, n - 1, None)):
        assert L.capi_drow_scale2(hip.h, *args) == EINVAL
    assert L.capi_drow_scale2(hip.h, 0, 2, None, 1, None, 1, None, 1, None) == 0
    assert L.capi_drow_scale2(hip.h, n, 0, None, 1, None, n, None, n, None) == 0
    hip.sync()
    assert np.all(rec.get() == 5.0)
    assert ds.get().tobytes() == np.ldexp(1.0, e.astype(np.int32)).tobytes()
    X.get()


@pytest.mark.parametrize("r", [1, 5, 32, 40])
def test_row_scale2(hip, r):
    for m in (1, 33, 257, 1000):
        rng = np.random.default_rng(1000 * r + m)
        e = rng.integers(-40, 40, m)
        ds = Buf(np.ldexp(1.0, e.astype(np.int32)))
        X = rng.standard_normal((m, r))
        ldx, ldy = m + 3, m + 1
        for sign in (1, -1):
            want = ref.row_scale(X, e, sign)
            # out of place, with norms
            src, dst, nrm = Buf(column_major(X, ldx, np.nan)), Buf(column_major(np.full((m, r), np.nan), ldy, SENTINEL)), Buf(np.full(r, np.nan))
            hip.call("capi_drow_scale2", m, r, ds.ptr, sign, src.ptr, ldx, dst.ptr, ldy, nrm.ptr)
            hip.sync()
            assert dst.get().tobytes() == column_major(want, ldy, SENTINEL).tobytes(), (m, r, sign)
            assert src.get().tobytes() == column_major(X, ldx, np.nan).tobytes()
            got = nrm.get()
            exact = (want.astype(LD) ** 2).sum(axis=0)
            err = np.abs(got.astype(LD) - exact) / exact
            print(f"row_scale2 m={m} r={r} sign={sign}: max relative error of the norms {float(err.max()):.2e}, bound {(m + 1) * U64:.2e}")
            assert np.all(err <= (m + 1) * U64)
            again = Buf(np.full(r, np.nan))
            hip.call("capi_drow_scale2", m, r, ds.ptr, sign, src.ptr, ldx, dst.ptr, ldy, again.ptr)
            hip.sync()
            assert again.get().tobytes() == got.tobytes()                   # one fixed order of the sum
            # in place, without norms: nothing but Y is written (the guard words and the padding rows stand)
            io = Buf(column_major(X, ldx, SENTINEL))
            hip.call("capi_drow_scale2", m, r, ds.ptr, sign, io.ptr, ldx, io.ptr, ldx, None)
            hip.sync()
            assert io.get().tobytes() == column_major(want, ldx, SENTINEL).tobytes(), (m, r, sign)
        ds.get()
    # a NaN shows in the norm of its own column alone
    m = 10
    X = np.ones((m, r))
    X[4, r - 1] = np.nan
    ds, io, nrm = Buf(np.full(m, 2.0)), Buf(column_major(X, m, 0.0)), Buf(np.full(r, 7.0))
    hip.call("capi_drow_scale2", m, r, ds.ptr, 1, io.ptr, m, io.ptr, m, nrm.ptr)
    hip.sync()
    got = nrm.get()
    assert np.isnan(got[r - 1]) and np.all(got[:r - 1] == 4.0 * m)
