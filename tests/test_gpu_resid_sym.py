"""capi_dresid_sym (Rout <- B - S X with its squared column norms, S the symmetric matrix given by A's upper triangle; the kernel of
capital_amd/csrc/sym_apply_f64.hip) against numpy on INTEGER-valued operands: entries in -8..8, so every partial sum -- and every sum of squares,
below 2^53 at these sizes -- is exact in fp64 whatever the order, and the comparison is for equality.  A's lower triangle holds NaN: a kernel that
reads below the diagonal, multiplies an unwanted element by zero, drops a tile, counts the diagonal twice or writes a guard row fails outright."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EINVAL = -1
SENTINEL = -7777.25
OFF = 3                                                                  # doubles in front of every operand: 8-byte alignment only


def ints(rng, shape):
    return np.asfortranarray(rng.integers(-8, 9, shape).astype(np.float64))


def dev(host):
    import torch
    return torch.from_numpy(np.ascontiguousarray(host)).cuda()


class In:
    """an l x c operand, column-major with leading dimension ld, OFF doubles into a buffer of NaN"""

    def __init__(self, M, ld=None):
        l, c = M.shape
        self.ld = max(1, l) if ld is None else ld
        full = np.full((c, self.ld), np.nan)
        full[:, :l] = M.T
        self.t = dev(np.concatenate([np.full(OFF, np.nan), full.reshape(-1)]))

    @property
    def ptr(self):
        return self.t.data_ptr() + 8 * OFF


class Out:
    """an l x r result with leading dimension l + 5, three doubles into a buffer filled with SENTINEL"""

    def __init__(self, C0):
        self.l, self.r = C0.shape
        self.ld, self.off = self.l + 5, OFF
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


def upper_stored(U, lower):
    """U's upper triangle over `lower` (a scalar or an n x n array)"""
    n = U.shape[0]
    return np.where(np.arange(n)[:, None] <= np.arange(n)[None, :], U, lower)


def sym(U):
    return np.triu(U) + np.triu(U, 1).T


def resid(h, n, r, dA, dX, dB, out, nrm, raw=False):
    """out: an Out, an In (in place: Rout == B) or None; nrm: an Out (r x 1) or None"""
    args = (n, r, dA.ptr if dA else None, dA.ld if dA else 1, dX.ptr if dX else None, dX.ld if dX else 1, dB.ptr if dB else None, dB.ld if dB else 1,
            out.ptr if out is not None else None, out.ld if out is not None else 0, nrm.ptr if nrm is not None else None)
    if raw:
        rc = h.L.capi_dresid_sym(h.h, *args)
        h.sync()
        return rc
    h.call("capi_dresid_sym", *args)
    h.sync()


def norms_out(r):
    return Out(np.full((r, 1), np.nan))                              # r contiguous doubles


def run_case(h, n, r, pad, seed):
    rng = np.random.default_rng(seed)
    U, X, B = ints(rng, (n, n)), ints(rng, (n, r)), ints(rng, (n, r))
    dA, dX, dB = In(upper_stored(U, np.nan), n + pad), In(X, n + (pad and 1)), In(B, n + 2 * pad)
    out, nrm = Out(np.full((n, r), np.nan)), norms_out(r)
    resid(h, n, r, dA, dX, dB, out, nrm)
    ref = B - sym(U) @ X
    got, got2 = out.get(), nrm.get()[:, 0]
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(got2))
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(got2, (ref * ref).sum(axis=0))
    return U, X, B, dA, dX, dB, ref


# the issue's sizes, and 6000: on 256 CUs the line blocks (n / 22 rounded up to 32) pass one super-tile of 256 lines from n = 5633 on, so 6000 is the
# smallest round size that walks 2 x 2 super-tiles per block (the X_I double buffer, the read-modify-write of the row slots, two column slots)
NS = [1, 2, 15, 16, 17, 31, 33, 127, 129, 255, 256, 257, 300, 1000, 1100, 2100, 6000]
RS = [1, 3, 16, 17, 32]
CASES = [(n, RS[(i + t) % 5], 3 * t) for i, n in enumerate(NS) for t in (0, 1)]
CASES += [(257, 32, 0), (2100, 16, 3), (2100, 17, 0), (1100, 1, 3)]
# the fused kernel runs below 8 columns, two capi_dtrmm_thin passes and the diagonal's correction from 8 on: both sides of that threshold, and the
# sizes that cross a line block, a super-tile and the LDS block of X once more with r < 8
CASES += [(300, 7, 0), (300, 8, 3), (257, 5, 0), (2100, 7, 3), (6000, 7, 3), (6000, 8, 0)]


@pytest.mark.parametrize("n,r,pad", CASES, ids=[f"n{n}-r{r}-ld+{pad}" for n, r, pad in CASES])
def test_against_numpy_with_nan_below_the_diagonal(hip, n, r, pad):
    run_case(hip, n, r, pad, 1000 * n + 10 * r + pad)


@pytest.mark.parametrize("n,r,pad", [(2100, 7, 0), (2100, 1, 3), (2100, 17, 3), (4000, 3, 3), (4000, 6, 0), (4000, 32, 0)])
def test_few_large_blocks(n, r, pad):
    """32 CUs (an own handle whose compute stream keeps 224 CUs free): p = 7, so n = 2100 gives line blocks of 320 (two super-tiles a side, the
    second ragged) and n = 4000 blocks of 576 (three): the fused kernel's walks over several super-tiles (r < 8), at sizes where the default plan
    has one; r >= 8 runs capi_dtrmm_thin under the same mask"""
    from capital_amd import capi
    hnd = capi.Handle(0, own_stream=True)
    try:
        assert hnd.L.capi_reserve_cus(hnd.h, 224) == 0
        run_case(hnd, n, r, pad, 7 * n + r)
    finally:
        hnd.close()


def test_forms(hip):
    n, r = 300, 5
    U, X, B, dA, dX, dB, ref = run_case(hip, n, r, 3, 42)
    ref2 = (ref * ref).sum(axis=0)
    # Rout == NULL: the norms alone
    nrm = norms_out(r)
    resid(hip, n, r, dA, dX, dB, None, nrm)
    np.testing.assert_array_equal(nrm.get()[:, 0], ref2)
    # colnorm2 == NULL: the residual alone
    out = Out(np.full((n, r), np.nan))
    resid(hip, n, r, dA, dX, dB, out, None)
    np.testing.assert_array_equal(out.get(), ref)
    # Rout == B: in place (B in a guarded buffer)
    inplace, nrm = Out(B), norms_out(r)
    resid(hip, n, r, dA, dX, inplace, inplace, nrm)
    np.testing.assert_array_equal(inplace.get(), ref)
    np.testing.assert_array_equal(nrm.get()[:, 0], ref2)
    # n == 0: colnorm2 <- 0
    nrm = norms_out(r)
    assert resid(hip, 0, r, None, None, None, None, nrm, raw=True) == 0
    np.testing.assert_array_equal(nrm.get()[:, 0], np.zeros(r))


def test_too_many_columns_touch_nothing(hip):
    n = 40
    rng = np.random.default_rng(3)
    U, X, B = ints(rng, (n, n)), ints(rng, (n, 33)), ints(rng, (n, 33))
    R0 = ints(rng, (n, 33))
    for r in (33, 0):
        out, nrm = Out(R0), Out(np.full((33, 1), 5.0))
        assert resid(hip, n, r, In(upper_stored(U, np.nan)), In(X), In(B), out, nrm, raw=True) == EINVAL
        np.testing.assert_array_equal(out.get(), R0)
        np.testing.assert_array_equal(nrm.get()[:, 0], np.full(33, 5.0))


@pytest.mark.parametrize("n,r", [(300, 17), (1100, 3), (2100, 7)])
def test_finite_lower_triangle_is_ignored(hip, n, r):
    """other finite values below the diagonal: the same bits as symmetric storage"""
    rng = np.random.default_rng(n + r)
    U, X, B = rng.standard_normal((n, n)), rng.standard_normal((n, r)), rng.standard_normal((n, r))
    dX, dB = In(X), In(B)
    got = []
    for lower in (sym(U), 100.0 * rng.standard_normal((n, n))):
        out, nrm = Out(np.zeros((n, r))), norms_out(r)
        resid(hip, n, r, In(upper_stored(U, lower), n + 3), dX, dB, out, nrm)
        got.append(out.get().tobytes() + nrm.get().tobytes())
    assert got[0] == got[1]


@pytest.mark.parametrize("r", [17, 5])
def test_random_data_is_reproducible_and_within_the_summation_bound(hip, r):
    """elementwise |err| <= gamma_(n + 1) (|S| |X| + |B|), gamma_k = k u / (1 - k u): the bound of a sum of n + 1 terms in ANY order (r = 5: the fused
    kernel; r = 17: the two-pass route)"""
    n = 2100
    rng = np.random.default_rng(11)
    U, X, B = rng.standard_normal((n, n)), rng.standard_normal((n, r)), rng.standard_normal((n, r))
    dA, dX, dB = In(upper_stored(U, np.nan), n + 3), In(X), In(B)
    outs = []
    for _ in range(2):
        out, nrm = Out(np.zeros((n, r))), norms_out(r)
        resid(hip, n, r, dA, dX, dB, out, nrm)
        outs.append((out.get(), nrm.get()[:, 0]))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    S = sym(U)
    ref = B.astype(np.longdouble) - S.astype(np.longdouble) @ X.astype(np.longdouble)
    u = 2.0 ** -53
    gamma = (n + 1) * u / (1 - (n + 1) * u)
    bound = gamma * (np.abs(S) @ np.abs(X) + np.abs(B))
    err = np.abs(outs[0][0].astype(np.longdouble) - ref).astype(np.float64)
    print(f"dresid_sym n={n} r={r}: max err / bound = {(err / bound).max():.3e}")
    assert np.all(err <= bound)
