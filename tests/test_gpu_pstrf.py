"""capi_dpstrf (Cholesky with complete pivoting of a Gram matrix, P^T G P = R^T R + diag-block(0, S); capital_amd/csrc/pstrf_f64.hip) and
capi_drow_scatter on the GPU, through the raw C-ABI.

G = A^T A as numpy forms it for the panels of tests/_pcqr_cases.py -- the same bits as the numpy restatement (tests/_pcqr_ref.py) sees -- with NaN
everywhere below the diagonal and a sentinel in the padding rows (n = 33 and n = 130 have padded leading dimensions).  The restatement is the
reference for the rank and for the size of the residual, by DESIGN.md section 2a's rule: gpu <= 10 max(restatement, u); the GPU is never compared
with itself.  Pivots are NOT compared with the CPU's: near-ties may break differently under another summation order.  What is asserted of them
is what makes a pivoted factor one: a permutation, a positive non-increasing diagonal, column dominance, and a Schur diagonal below the threshold."""
import ctypes as C
import functools

import numpy as np
import pytest

import _pcqr_cases as pc
import _pcqr_ref as pref
import _scqr_ref as ref
from _scqr_ref import U64

pytestmark = pytest.mark.gpu
EINVAL = -1
SENTINEL = -7777.25
PADDED = {33: 36, 130: 136}          # n -> ldg


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


def ints(values):
    import torch
    return torch.tensor(np.asarray(values, dtype=np.int32)).cuda()


def place_G(G, ldg):
    """the upper triangle of G with NaN below its diagonal (and SENTINEL in the padding rows)"""
    n = G.shape[0]
    return Block(n, n, ldg, np.where(np.arange(n)[:, None] <= np.arange(n)[None, :], G, np.nan))


def dpstrf(hip, G, tol, ldg=None):
    """(R image n x n with NaN below the diagonal, piv, rank, raw bytes of the block)"""
    n = G.shape[0]
    dG = place_G(G, ldg or n)
    dp = ints(np.full(n, -5))
    rank = C.c_int(-99)
    hip.call("capi_dpstrf", n, dG.ptr, dG.ld, float(tol), dp.data_ptr(), C.byref(rank))
    hip.sync()
    out = dG.get()
    low = np.tril_indices(n, -1)
    assert np.all(np.isnan(out[low])), "an entry below the diagonal was written"
    return out, dp.cpu().numpy().astype(np.int64), rank.value, dG.raw()


def check_factor(tag, G, out, piv, rank, thresh, ref_res):
    """everything the issue asks of a pivoted factor, from G's upper triangle, the GPU's trapezoid and its permutation"""
    n = G.shape[0]
    assert sorted(piv.tolist()) == list(range(n)), "piv is not a permutation"
    R = np.triu(out)[:rank]
    d = np.diag(R)
    assert np.all(np.isfinite(R)) and np.all(d > 0.0)
    assert np.all(np.diff(d) <= 1e-12 * d[0]), "the diagonal of R increases"
    # column dominance: r_jj^2 (1 + 1e-10) >= sum_{i = j .. min(l, k - 1)} r_il^2 for l > j -- the sums are reverse cumulative sums down the columns
    tail = np.cumsum((R * R)[::-1], axis=0)[::-1]
    viol = np.triu(tail - ((d * d) * (1 + 1e-10))[:, None], 1)
    assert np.all(viol <= 0.0), ("column dominance", float(viol.max()))
    res, schur = pref.pstrf_checks(G, out, piv, rank)
    print(f"dpstrf {tag}: rank {rank}, residual {res:.3e} (restatement {ref_res:.3e}), largest Schur diagonal {schur:.3e}, thresh {thresh:.3e}")
    assert res <= 10.0 * max(ref_res, U64), (res, ref_res)
    assert schur <= thresh * (1 + 1e-8), (schur, thresh)


@functools.lru_cache(maxsize=None)
def reference(m, n, k):
    """(restatement's rank, its residual by the same measure, thresh), computed once"""
    G = pc.gram(m, n, k)
    r = pc.restatement(m, n, k)
    Rf, piv, rank, thresh = pref.pstrf(G, r["tol"])
    return rank, pref.pstrf_checks(G, Rf, piv, rank)[0], thresh, r["tol"]


@pytest.mark.parametrize("m,n,k", pc.CASES, ids=pc.IDS)
def test_against_the_restatement(hip, m, n, k):
    G = pc.gram(m, n, k)
    ref_rank, ref_res, thresh, tol = reference(m, n, k)
    assert ref_rank == k
    out, piv, rank, raw = dpstrf(hip, G, tol, PADDED.get(n))
    out2, piv2, rank2, raw2 = dpstrf(hip, G, tol, PADDED.get(n))
    assert rank == ref_rank
    check_factor(f"{m}x{n}", G, out, piv, rank, thresh, ref_res)
    assert rank2 == rank and np.array_equal(piv2, piv) and raw.tobytes() == raw2.tobytes()       # two runs give identical bytes


def test_order_one(hip):
    out, piv, rank, _ = dpstrf(hip, np.array([[4.0]]), 1e-10)
    assert rank == 1 and piv.tolist() == [0] and out[0, 0] == 2.0
    out, piv, rank, _ = dpstrf(hip, np.array([[0.0]]), 0.0)
    assert rank == 0 and piv.tolist() == [0]


@functools.lru_cache(maxsize=None)
def largest():
    """G of a well-conditioned 2048-column panel, and the restatement on it"""
    A = ref.panel(4096, 2048, 1e1, 2048)
    G = np.asfortranarray(A.T @ A)
    tol = pref.floor_tol(4096, 2048)
    Rf, piv, rank, thresh = pref.pstrf(G, tol)
    return G, tol, rank, pref.pstrf_checks(G, Rf, piv, rank)[0], thresh


def test_largest_order(hip):
    G, tol, ref_rank, ref_res, thresh = largest()
    assert ref_rank == 2048
    out, piv, rank, _ = dpstrf(hip, G, tol)
    assert rank == 2048
    check_factor("n=2048", G, out, piv, rank, thresh, ref_res)


def test_zero_tolerance_factors_a_full_rank_matrix_to_the_end(hip):
    m, n, k = 2048, 32, 32
    G = pc.gram(m, n, k)
    Rf, piv_r, rank_r, _ = pref.pstrf(G, 0.0)
    out, piv, rank, _ = dpstrf(hip, G, 0.0)
    assert rank == rank_r == n
    check_factor("tol=0", G, out, piv, rank, 0.0, pref.pstrf_checks(G, Rf, piv_r, rank_r)[0])


def test_bad_arguments_touch_nothing(hip):
    G = pc.gram(2048, 2, 1)
    dG = place_G(G, 2)
    before = dG.raw().copy()
    dp = ints([-5, -5])
    for n, ldg, tol in ((0, 2, 0.0), (2049, 2049, 0.0), (2, 2, -1e-3), (2, 1, 0.0), (2, 2, float("nan"))):
        rank = C.c_int(-99)
        rc = hip.L.capi_dpstrf(hip.h, n, dG.ptr, ldg, tol, dp.data_ptr(), C.byref(rank))
        hip.sync()
        assert rc == EINVAL and rank.value == -99, (n, ldg, tol, rc)
        np.testing.assert_array_equal(dG.raw(), before)
        assert dp.cpu().tolist() == [-5, -5]
    rank = C.c_int(-99)
    assert hip.L.capi_dpstrf(hip.h, 2, None, 2, 0.0, dp.data_ptr(), C.byref(rank)) == EINVAL
    assert hip.L.capi_dpstrf(hip.h, 2, dG.ptr, 2, 0.0, None, C.byref(rank)) == EINVAL
    assert hip.L.capi_dpstrf(hip.h, 2, dG.ptr, 2, 0.0, dp.data_ptr(), None) == EINVAL
    assert rank.value == -99


@pytest.mark.parametrize("where", ["diagonal", "above"])
def test_not_a_number_ends_the_call(hip, where):
    """one NaN in the triangle: CAPI_OK, a rank in 0 .. n and a permutation; the values are unspecified"""
    m, n, k = 4160, 65, 40
    G = np.array(pc.gram(m, n, k))
    if where == "diagonal":
        G[7, 7] = np.nan
    else:
        G[3, 50] = np.nan
    out, piv, rank, _ = dpstrf(hip, G, pref.floor_tol(m, n))
    assert 0 <= rank <= n and sorted(piv.tolist()) == list(range(n))


def test_the_info_word_is_not_touched(hip):
    hip.call("capi_reset_info")
    dpstrf(hip, pc.gram(2048, 32, 1), pref.floor_tol(2048, 32))
    assert hip.info() == 0


@pytest.mark.parametrize("tri", [0, 1])
def test_row_scatter(hip, tri):
    rng = np.random.default_rng(11)
    n, k, ncols, lds, ldd = 37, 21, 23, 25, 40
    S = rng.standard_normal((k, ncols))
    piv = rng.permutation(n)
    dS = Block(k, ncols, lds, np.where(np.arange(k)[:, None] <= np.arange(ncols)[None, :], S, np.nan) if tri else S)
    dp = ints(piv)

    def run(kk, perm):
        dD = Block(n, ncols, ldd)
        hip.call("capi_drow_scatter", tri, kk, ncols, n, dS.ptr, lds, perm.data_ptr(), dD.ptr, ldd)
        hip.sync()
        return dD.get()

    want = np.zeros((n, ncols))
    want[piv[:k]] = np.triu(S) if tri else S
    np.testing.assert_array_equal(run(k, dp), want)
    np.testing.assert_array_equal(run(0, dp), np.zeros((n, ncols)))                                 # k = 0: zeros alone
    ident = np.zeros((n, ncols))
    ident[:k] = np.triu(S) if tri else S
    np.testing.assert_array_equal(run(k, ints(np.arange(n))), ident)                                # the identity permutation
    dD = Block(n, ncols, ldd)
    for bad in ((tri, k, ncols, n, dS.ptr, k - 1, dp.data_ptr(), dD.ptr, ldd), (tri, k, ncols, n, dS.ptr, lds, dp.data_ptr(), dD.ptr, n - 1),
                (tri, n + 1, ncols, n, dS.ptr, n + 1, dp.data_ptr(), dD.ptr, ldd), (2, k, ncols, n, dS.ptr, lds, dp.data_ptr(), dD.ptr, ldd)):
        assert hip.L.capi_drow_scatter(hip.h, *bad) == EINVAL
    hip.sync()
    assert np.all(dD.raw() == SENTINEL)
