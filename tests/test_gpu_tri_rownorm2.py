"""capi_dtri_rownorm2 (out[i] <- beta out[i] + sum_j T(i, j)^2 over a triangle or rectangle in column-major or packed storage; the kernel of
capital_amd/csrc/tri_reduce_f64.hip), capi_dtri_logdiag and capi_dcolnorm2 through the C-ABI, against numpy in longdouble.

Bounds (u = 2^-53), derived, not measured.
  rownorm2: row i sums k_i non-negative terms, each square rounded once (or fused into its addition, which rounds less), so ANY summation order stays
    within (k_i + 1) u of the exact sum S_i, relatively; the final beta out0_i + S_i rounds once more, u |beta out0_i| beyond what (k_i + 1) u S_i
    covers (beta = 1 and -0.5 multiply exactly).  Asserted: |out_i - (beta out0_i + S_i)| <= 1.01 (k_i + 1) u S_i + |beta| u |out0_i|.
  logdiag: summing n terms costs at most (n - 1) u sum |log t_ii|, the device log is taken as within 1 ulp (the ROCm math library's stated accuracy),
    and the host reference's own log within another: asserted |out - ref| <= (n + 3) u sum_i |log t_ii|.
  colnorm2: (n + 1) u relative, as a row of rownorm2."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RECT, UPPERTRI = 0, 1
EINVAL = -1
U64 = 2.0 ** -53
LD = np.longdouble
SENTINEL = -7777.25
BETAS = (0.0, 1.0, -0.5)
GROUP, DEPTH = 256, 32                      # tri_thin_plan.h


def pstart(x):
    return x * (x + 1) // 2


def pack_upper(U):
    return np.concatenate([U[:j + 1, j] for j in range(U.shape[0])])


def dev(host):
    import torch
    return torch.from_numpy(np.ascontiguousarray(host)).cuda()


class Out:
    """m results three doubles into a buffer filled with SENTINEL, seven guard words behind out[m - 1]"""

    def __init__(self, start):
        self.m, self.off = len(start), 3
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


def rownorm2(hip, shape, m, n, Tptr, ldt, col0, beta, out, raw=False):
    args = (shape, m, n, Tptr, ldt, col0, beta, out.ptr)
    if raw:
        rc = hip.L.capi_dtri_rownorm2(hip.h, *args)
        hip.sync()
        return rc
    hip.call("capi_dtri_rownorm2", *args)
    hip.sync()


def check(hip, Tm, tri, Tptr, ldt, col0, rng, betas=BETAS):
    """Tm: the block as a dense m x n array; with tri only its upper triangle takes part"""
    m, n = Tm.shape
    Tl = (np.triu(Tm) if tri else Tm).astype(LD)
    S = (Tl * Tl).sum(axis=1)
    k = (n - np.arange(m)) if tri else np.full(m, n)
    for beta in betas:
        out0 = rng.standard_normal(m)
        out = Out(np.full(m, np.nan) if beta == 0.0 else out0)             # beta == 0: out is not read
        rownorm2(hip, UPPERTRI if tri else RECT, m, n, Tptr, ldt, col0, beta, out)
        got = out.get()
        want = S + (LD(beta) * out0.astype(LD) if beta != 0.0 else 0)
        bound = 1.01 * (k + 1) * U64 * S + (abs(beta) * U64 * np.abs(out0) if beta != 0.0 else 0)
        err = np.abs(got.astype(LD) - want)
        assert np.all(np.isfinite(got))
        worst = float((err / bound).max()) if m else 0.0
        print(f"rownorm2 {m} x {n} tri={tri} ldt={ldt} col0={col0} beta={beta}: max err / bound = {worst:.3f}")
        assert np.all(err <= bound), (beta, int(np.argmax(err / bound)))
        again = Out(np.full(m, np.nan) if beta == 0.0 else out0)
        rownorm2(hip, UPPERTRI if tri else RECT, m, n, Tptr, ldt, col0, beta, again)
        assert again.get().tobytes() == got.tobytes()                      # two calls give the same bytes


def column_major_with_nan(Tm, tri, pad):
    """ld = m + pad; NaN in the padding rows and, for a triangle, everywhere below the diagonal"""
    m, n = Tm.shape
    full = np.full((m + pad, n), np.nan)
    full[:m, :] = np.where(np.arange(m)[:, None] <= np.arange(n)[None, :], Tm, np.nan) if tri else Tm
    return dev(full.T.reshape(-1)), m + pad


@pytest.mark.parametrize("n", [1, 5, 31, 32, 33, 257, 1000, 2048])
def test_triangle_packed_and_column_major(hip, n):
    rng = np.random.default_rng(n)
    U = np.triu(rng.standard_normal((n, n)))
    dT = dev(np.concatenate([[np.nan], pack_upper(U), [np.nan]]))          # a NaN word in front of and behind the triangle
    check(hip, U, True, dT.data_ptr() + 8, 0, 0, rng)
    dF, ld = column_major_with_nan(U, True, 3)
    check(hip, U, True, dF.data_ptr(), ld, 0, rng)


def slices_of(hip, n):
    """the slice count of capi_dtrmm_thin's NOTRANS partition of a triangle of order n (tri_thin_plan.h: make_slices)"""
    import torch
    ngroups, kc = -(-n // GROUP), -(-n // DEPTH)
    tiles = ngroups * kc - (GROUP // DEPTH // 2) * ngroups * (ngroups - 1)
    return min(torch.cuda.get_device_properties(0).multi_processor_count, 256, tiles), ngroups


def test_packed_4096_has_several_slices_per_group_of_lines(hip):
    n = 4096
    S, ngroups = slices_of(hip, n)
    print(f"rownorm2 n={n}: {S} slices over {ngroups} groups of lines")
    assert S >= 4 * ngroups            # slices hold equal bytes: the first group of lines alone, an eighth of the triangle, is cut into S / 8 of them
    rng = np.random.default_rng(n)
    U = np.triu(rng.standard_normal((n, n)))
    dT = dev(pack_upper(U))
    check(hip, U, True, dT.data_ptr(), 0, 0, rng)


def test_sub_triangles_of_a_packed_triangle(hip):
    N = 1000
    rng = np.random.default_rng(17)
    U = np.triu(rng.standard_normal((N, N)))
    dT = dev(np.concatenate([[np.nan], pack_upper(U), [np.nan]]))
    base = dT.data_ptr() + 8
    for col0, k in ((1, 300), (37, 513), (500, 500)):
        check(hip, U[col0:col0 + k, col0:col0 + k], True, base + 8 * (pstart(col0) + col0), 0, col0, rng)


@pytest.mark.parametrize("m,n", [(5, 300), (300, 5), (1000, 129)])
def test_rectangles(hip, m, n):
    rng = np.random.default_rng(m + 7 * n)
    Tm = np.asfortranarray(rng.standard_normal((m, n)))
    dF, ld = column_major_with_nan(Tm, False, 3)
    check(hip, Tm, False, dF.data_ptr(), ld, 0, rng)
    # rows 0 .. m - 1 of the columns h .. h + n - 1 of a packed triangle of order h + n, h = m: the block lies above the diagonal
    h = m
    U = np.triu(rng.standard_normal((h + n, h + n)))
    dT = dev(np.concatenate([[np.nan], pack_upper(U), [np.nan]]))
    check(hip, U[:m, h:], False, dT.data_ptr() + 8 + 8 * pstart(h), 0, h, rng)


def test_conventions_and_refusals(hip):
    rng = np.random.default_rng(3)
    n = 40
    U = np.triu(rng.standard_normal((n, n)))
    dT = dev(U.T.reshape(-1))
    out0 = rng.standard_normal(n)
    bad = ((2, n, n, n, 0), (UPPERTRI, n, n - 1, n, 0), (RECT, -1, n, n, 0), (RECT, n, -1, n, 0), (RECT, n, n, n - 1, 0), (UPPERTRI, n, n, 0, -1))
    for shape, m_, n_, ldt, col0 in bad:
        out = Out(out0)
        assert rownorm2(hip, shape, m_, n_, dT.data_ptr(), ldt, col0, 1.0, out, raw=True) == EINVAL
        np.testing.assert_array_equal(out.get(), out0)
    out = Out(out0)                                                        # a null T with something to read
    assert rownorm2(hip, RECT, n, n, None, n, 0, 1.0, out, raw=True) == EINVAL
    np.testing.assert_array_equal(out.get(), out0)
    for beta in (2.0, 0.0):                                                # n == 0: out <- beta out
        out = Out(out0)
        assert rownorm2(hip, RECT, n, 0, dT.data_ptr(), n, 0, beta, out, raw=True) == 0
        np.testing.assert_array_equal(out.get(), beta * out0)
    out = Out(out0)                                                        # m == 0: nothing happens
    assert rownorm2(hip, RECT, 0, n, dT.data_ptr(), 1, 0, 0.0, out, raw=True) == 0
    np.testing.assert_array_equal(out.get(), out0)


def logdiag(hip, n, Tptr, ldt, col0):
    out = Out(np.full(1, np.nan))
    hip.call("capi_dtri_logdiag", n, Tptr, ldt, col0, out.ptr)
    hip.sync()
    return out.get()[0]


def check_logdiag(got, d, what):
    logs = np.log(d.astype(LD))
    ref, scale = logs.sum(), np.abs(logs).sum()
    n = len(d)
    err, bound = abs(LD(got) - ref), (n + 3) * U64 * scale
    print(f"logdiag n={n} {what}: |out - ref| = {float(err):.2e}, bound {float(bound):.2e}")
    assert np.isfinite(got) and err <= bound


@pytest.mark.parametrize("n", [1, 33, 1000, 4096])
def test_logdiag(hip, n):
    import torch
    rng = np.random.default_rng(n)
    d = rng.uniform(0.5, 2.0, n)
    # packed: the diagonal of a triangle whose other entries are NaN
    host = np.full(pstart(n) + 2, np.nan)
    host[1 + pstart(np.arange(n)) + np.arange(n)] = d
    dT = dev(host)
    check_logdiag(logdiag(hip, n, dT.data_ptr() + 8, 0, 0), d, "packed")
    # a diagonal sub-triangle at col0 > 0
    col0 = min(7, n - 1)
    if col0 > 0:
        check_logdiag(logdiag(hip, n - col0, dT.data_ptr() + 8 + 8 * (pstart(col0) + col0), 0, col0), d[col0:], f"packed col0={col0}")
    # column-major, ld = n + 1, NaN everywhere off the diagonal
    ld = n + 1
    full = torch.full((n * ld,), float("nan"), dtype=torch.float64, device="cuda")
    full[::ld + 1][:n] = torch.from_numpy(d).cuda()
    check_logdiag(logdiag(hip, n, full.data_ptr(), ld, 0), d, f"ld={ld}")


def test_logdiag_conventions(hip):
    assert logdiag(hip, 0, None, 1, 0) == 0.0                              # n == 0 gives 0
    d = np.array([2.0, 0.0, 3.0])
    dT = dev(np.diag(d).reshape(-1))
    assert logdiag(hip, 3, dT.data_ptr(), 3, 0) == -np.inf                 # no sign check
    d[1] = -1.0
    dT = dev(np.diag(d).reshape(-1))
    assert np.isnan(logdiag(hip, 3, dT.data_ptr(), 3, 0))
    out = Out(np.full(1, 5.0))
    assert hip.L.capi_dtri_logdiag(hip.h, -1, None, 1, 0, out.ptr) == EINVAL
    assert hip.L.capi_dtri_logdiag(hip.h, 3, dT.data_ptr(), 2, 0, out.ptr) == EINVAL
    hip.sync()
    assert out.get()[0] == 5.0


@pytest.mark.parametrize("r", [1, 5, 32])
def test_colnorm2(hip, r):
    for n in (1, 257, 1000, 4096):
        rng = np.random.default_rng(100 * n + r)
        X = rng.standard_normal((n, r))
        full = np.full((n + 3, r), np.nan)                                 # ld = n + 3, NaN in the padding rows
        full[:n] = X
        dX = dev(full.T.reshape(-1))
        out = Out(np.full(r, np.nan))
        hip.call("capi_dcolnorm2", n, r, dX.data_ptr(), n + 3, out.ptr)
        hip.sync()
        got = out.get()
        ref = (X.astype(LD) ** 2).sum(axis=0)
        err = np.abs(got.astype(LD) - ref) / ref
        print(f"colnorm2 n={n} r={r}: max relative error {float(err.max()):.2e}, bound {(n + 1) * U64:.2e}")
        assert np.all(err <= (n + 1) * U64)
    # a NaN shows in its own column only; n == 0 gives zeros; r out of range is refused with out untouched
    X = np.ones((10, r))
    X[4, r - 1] = np.nan
    out = Out(np.full(r, 7.0))
    dX = dev(X.T.reshape(-1))
    hip.call("capi_dcolnorm2", 10, r, dX.data_ptr(), 10, out.ptr)
    hip.sync()
    got = out.get()
    assert np.isnan(got[r - 1]) and np.all(got[:r - 1] == 10.0)
    out = Out(np.full(r, 7.0))
    hip.call("capi_dcolnorm2", 0, r, None, 1, out.ptr)
    hip.sync()
    assert np.all(out.get() == 0.0)
    out = Out(np.full(r, 7.0))
    assert hip.L.capi_dcolnorm2(hip.h, 10, 33, dX.data_ptr(), 10, out.ptr) == EINVAL
    hip.sync()
    assert np.all(out.get() == 7.0)
