"""capi_dtrmm_thin (C <- alpha op(T) B + beta C, T a triangle or rectangle in column-major or packed storage, r <= 32 columns; the kernel of
capital_amd/csrc/tri_apply_f64.hip) against numpy on INTEGER-valued operands: entries in -8..8, alpha and beta multiples of 1/2, so every partial
sum is exact in fp64 whatever the order and the comparison is for equality.  A kernel that drops a tile, reads below the diagonal, takes a
packed column from a 32-bit offset or writes a guard row fails outright."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RECT, UPPERTRI, NOTRANS, TRANS = 0, 1, 0, 1
EINVAL = -1
SENTINEL = -7777.25
AB = [(1.0, 0.0), (-1.0, 1.0), (0.5, 2.0)]


def ints(rng, shape):
    return np.asfortranarray(rng.integers(-8, 9, shape).astype(np.float64))


def pstart(x):
    return x * (x + 1) // 2


def pack_upper(U):
    return np.concatenate([U[:j + 1, j] for j in range(U.shape[0])])


def dev(host):
    import torch
    return torch.from_numpy(np.ascontiguousarray(host)).cuda()


class Out:
    """an l x r result with leading dimension l + 5, three doubles into a buffer filled with SENTINEL"""

    def __init__(self, C0):
        self.l, self.r = C0.shape
        self.ld, self.off = self.l + 5, 3
        host = np.full(self.off + self.ld * self.r + 7, SENTINEL)
        self.mask = np.ones(host.shape, bool)
        self._win(host)[:, :] = C0
        self._win(self.mask)[:, :] = False
        self.t = dev(host)

    def _win(self, a):
        return a[self.off:self.off + self.ld * self.r].reshape(self.r, self.ld).T[:self.l]

    @property
    def ptr(self):
        return self.t.data_ptr() + 8 * self.off

    def get(self):
        host = self.t.cpu().numpy()
        assert np.all(host[self.mask] == SENTINEL), "something outside the result was written"
        return np.array(self._win(host), order="F")


def thin(hip, shape, trans, m, n, r, alpha, Tptr, ldt, col0, dB, ldb, beta, out, raw=False):
    args = (shape, trans, m, n, r, alpha, Tptr, ldt, col0, dB.data_ptr(), ldb, beta, out.ptr, out.ld)
    if raw:
        rc = hip.L.capi_dtrmm_thin(hip.h, *args)
        hip.sync()
        return rc
    hip.call("capi_dtrmm_thin", *args)
    hip.sync()


def run_case(hip, Tm, shape, trans, r, ab, Tptr, ldt, col0, rng, keep=None):
    """Tm: the block as a dense m x n array (zeros where nothing takes part); returns after comparing for equality"""
    m, n = Tm.shape
    alpha, beta = ab
    lines, depth = (n, m) if trans else (m, n)
    B, C0 = ints(rng, (depth, r)), ints(rng, (lines, r))
    start = np.full((lines, r), np.nan) if beta == 0.0 else C0            # beta == 0: C is not read
    out = Out(start)
    dB = dev(B.T.reshape(-1)) if depth else dev(np.zeros(1))
    thin(hip, shape, trans, m, n, r, alpha, Tptr, ldt, col0, dB, max(1, depth), beta, out)
    ref = alpha * ((Tm.T if trans else Tm) @ B) + (beta * C0 if beta != 0.0 else 0.0)
    got = out.get()
    assert np.all(np.isfinite(got))
    np.testing.assert_array_equal(got, ref)
    return got


NS = [1, 2, 15, 16, 17, 31, 33, 127, 129, 300, 1000, 1100, 2100]
RS = [1, 3, 16, 17, 32]
STORES = ["packed", "ld", "ld+3"]
# a pruned product: every n with both directions; r, the storage and (alpha, beta) rotate along the list; the two sizes that cross the LDS blocks of
# the thin operand (256 contraction indices) come with r <= 16 and r > 16 in every storage
CASES = [(n, RS[(i + 2 * t) % 5], t, STORES[(i + t) % 3], AB[(i + t) % 3]) for i, n in enumerate(NS) for t in (0, 1)]
CASES += [(n, r, t, st, AB[(r + t) % 3]) for n in (1100, 2100) for r in (16, 17) for t in (0, 1) for st in ("packed", "ld+3")]
CASES += [(300, 32, 0, "packed", AB[1]), (300, 1, 1, "packed", AB[2]), (129, 32, 1, "ld", AB[0]), (1000, 32, 0, "ld+3", AB[1])]


@pytest.mark.parametrize("n,r,trans,store,ab", CASES, ids=[f"n{n}-r{r}-t{t}-{st}-a{ab[0]}b{ab[1]}" for n, r, t, st, ab in CASES])
def test_triangle_against_numpy(hip, n, r, trans, store, ab):
    rng = np.random.default_rng(1000 * n + 10 * r + trans)
    U = np.triu(ints(rng, (n, n)))
    if store == "packed":
        # a NaN word in front of and behind the triangle: nothing outside it may take part
        host = np.concatenate([[np.nan], pack_upper(U), [np.nan]])
        dT = dev(host)
        run_case(hip, U, UPPERTRI, trans, r, ab, dT.data_ptr() + 8, 0, 0, rng)
    else:
        ld = n + (3 if store == "ld+3" else 0)
        full = np.full((ld, n), np.nan)                                   # NaN below the diagonal and in the padding rows
        full[:n, :] = np.where(np.arange(n)[:, None] <= np.arange(n)[None, :], U, np.nan)
        dT = dev(full.T.reshape(-1))
        got = run_case(hip, U, UPPERTRI, trans, r, ab, dT.data_ptr(), ld, 0, rng)
        full0 = np.zeros((ld, n))
        full0[:n, :] = U
        dT0 = dev(full0.T.reshape(-1))
        rng = np.random.default_rng(1000 * n + 10 * r + trans)
        ints(rng, (n, n))
        got0 = run_case(hip, U, UPPERTRI, trans, r, ab, dT0.data_ptr(), ld, 0, rng)
        assert got.tobytes() == got0.tobytes()                            # NaN below the diagonal: the same bits as zeros there


@pytest.mark.parametrize("m,n", [(5, 300), (300, 5), (1000, 129)])
@pytest.mark.parametrize("trans", [0, 1])
def test_rectangle_full_storage(hip, m, n, trans):
    rng = np.random.default_rng(m + 7 * n + trans)
    Tm = ints(rng, (m, n))
    for r, pad, ab in ((3, 0, AB[0]), (17, 3, AB[1]), (32, 1, AB[2])):
        full = np.full((m + pad, n), np.nan)
        full[:m, :] = Tm
        dT = dev(full.T.reshape(-1))
        run_case(hip, Tm, RECT, trans, r, ab, dT.data_ptr(), m + pad, 0, rng)


@pytest.mark.parametrize("trans", [0, 1])
def test_views_into_a_packed_triangle(hip, trans):
    """a diagonal triangle at an odd and at an even col0, and the R12 rectangle (rows 0 .. h1 - 1 of columns h1 ..) for h1 = 128, 129"""
    N = 300
    rng = np.random.default_rng(17 + trans)
    U = np.triu(ints(rng, (N, N)))
    dT = dev(np.concatenate([[np.nan], pack_upper(U), [np.nan]]))
    base = dT.data_ptr() + 8
    for col0, k, r, ab in ((129, 150, 17, AB[1]), (128, 172, 3, AB[0]), (1, 40, 32, AB[2])):
        run_case(hip, U[col0:col0 + k, col0:col0 + k], UPPERTRI, trans, r, ab, base + 8 * (pstart(col0) + col0), 0, col0, rng)
    for h1, r, ab in ((128, 16, AB[2]), (129, 32, AB[1]), (129, 1, AB[0])):
        run_case(hip, U[:h1, h1:], RECT, trans, r, ab, base + 8 * pstart(h1), 0, h1, rng)


@pytest.mark.parametrize("trans", [0, 1])
def test_offsets_beyond_32_bits(hip, trans):
    """a 16 x 64 view at col0 = 70000: the last column starts 4.4e6 doubles behind the first, at packed index 2.45e9 of its triangle -- the offset
    arithmetic must be 64-bit (x (x + 1) alone overflows 32 bits from x = 65536 on)"""
    col0, m, n = 70000, 16, 64
    count = (pstart(col0 + n) - pstart(col0))
    assert count == (70064 * 70065 - 70000 * 70001) // 2
    rng = np.random.default_rng(5 + trans)
    host = rng.integers(-8, 9, count).astype(np.float64)
    Tm = np.asfortranarray(np.stack([host[pstart(col0 + j) - pstart(col0):][:m] for j in range(n)], axis=1))
    dT = dev(host)
    run_case(hip, Tm, RECT, trans, 5, AB[1], dT.data_ptr(), 0, col0, rng)


def test_argument_errors_touch_nothing(hip):
    rng = np.random.default_rng(3)
    n = 40
    U = np.triu(ints(rng, (n, n)))
    dT, dB = dev(U.T.reshape(-1)), dev(ints(rng, (n, 33)).T.reshape(-1))
    C0 = ints(rng, (n, 33))
    for shape, m_, n_, r in ((UPPERTRI, n, n, 33), (UPPERTRI, n, n - 1, 3), (RECT, -1, n, 3), (RECT, n, -1, 3), (UPPERTRI, n, n, 0)):
        out = Out(C0)
        assert thin(hip, shape, NOTRANS, m_, n_, r, 1.0, dT.data_ptr(), n, 0, dB, n, 0.0, out, raw=True) == EINVAL
        np.testing.assert_array_equal(out.get(), C0)
    # m == 0 (TRANS: C is n x r) and n == 0 (NOTRANS: C is m x r): C <- beta C
    for trans, m_, n_ in ((TRANS, 0, n), (NOTRANS, n, 0)):
        out = Out(C0[:, :5])
        assert thin(hip, RECT, trans, m_, n_, 5, 1.0, dT.data_ptr(), max(1, m_), 0, dB, n, 2.0, out, raw=True) == 0
        np.testing.assert_array_equal(out.get(), 2.0 * C0[:, :5])


@pytest.mark.parametrize("trans", [0, 1])
def test_random_data_is_reproducible_and_at_the_parity_bar(hip, trans):
    n, r = 2100, 32
    rng = np.random.default_rng(11 + trans)
    U = np.triu(rng.standard_normal((n, n)))
    B = np.asfortranarray(rng.standard_normal((n, r)))
    dT, dB = dev(pack_upper(U)), dev(B.T.reshape(-1))
    outs = []
    for _ in range(2):
        out = Out(np.zeros((n, r)))
        thin(hip, UPPERTRI, trans, n, n, r, 1.0, dT.data_ptr(), 0, 0, dB, n, 0.0, out)
        outs.append(out.get())
    assert outs[0].tobytes() == outs[1].tobytes()
    ref = (U.T if trans else U) @ B
    err = np.abs(outs[0] - ref).max() / np.abs(ref).max()
    print(f"dtrmm_thin n={n} r={r} trans={trans}: max |C - numpy| / max |C| = {err:.2e}")
    assert err <= 1e-12
