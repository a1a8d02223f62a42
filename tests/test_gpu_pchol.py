"""capi_dpchol (diagonally pivoted, partial Cholesky A ~= L L^T; capital_amd/csrc/pchol_f64.hip) on the GPU, through the raw C-ABI.

A is placed as the restatement (tests/_pchol_ref.py) sees it -- the same bits -- with NaN everywhere below the diagonal and a sentinel in the padding
rows; L is a sentinel-filled block.  The restatement is the reference for the rank (where the rank is decided with a margin: the exact-rank and the
capped cases) and for the size of the residuals, by DESIGN.md section 2a's rule: gpu <= 10 max(restatement, u); the GPU is never compared with itself.
Pivots are NOT compared with the CPU's: near-ties may break differently under another summation order.  What is asserted of them is what makes a greedy
pivoted factor one: a permutation, exact zeros in the rows chosen before, a positive pivot entry, the greedy property on the running diagonal
recomputed from the GPU's L (the kernel rounds d_i - L(i, j)^2 in two steps so that this recomputation gives its own bits), and the stop rule."""
import ctypes as C

import numpy as np
import pytest

import _pchol_cases as pc
import _pchol_ref as pref
from _pchol_ref import U64

pytestmark = pytest.mark.gpu
EINVAL = -1
SENTINEL = -7777.25


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


def place_A(A, lda):
    """the upper triangle of A with NaN below its diagonal (and SENTINEL in the padding rows)"""
    n = A.shape[0]
    return Block(n, n, lda, np.where(np.arange(n)[:, None] <= np.arange(n)[None, :], A, np.nan))


def dpchol(hip, A, tol, kmax, lda=None, ldl=None):
    """dict(L n x rank, piv, d, rank, resid_trace, thresh, bytes): one call, with everything the call must leave alone checked"""
    import torch
    n = A.shape[0]
    dA = place_A(A, lda or n)
    before = dA.raw().tobytes()
    dL = Block(n, kmax, ldl or n)
    dp = torch.full((n,), -5, dtype=torch.int32).cuda()
    dd = torch.full((n,), SENTINEL, dtype=torch.float64).cuda()
    rank, trace, thresh = C.c_int(-99), C.c_double(-99.0), C.c_double(-99.0)
    hip.call("capi_dpchol_thresh", n, dA.ptr, dA.ld, float(tol), C.byref(thresh))
    hip.call("capi_dpchol", n, dA.ptr, dA.ld, float(tol), kmax, dL.ptr, dL.ld, dp.data_ptr(), dd.data_ptr(), C.byref(rank), C.byref(trace))
    hip.sync()
    assert dA.raw().tobytes() == before, "A was written"
    Lraw = dL.raw()
    k = rank.value
    assert 0 <= k <= kmax
    assert np.all(Lraw[:, n:] == SENTINEL), "the padding rows of L were written"
    assert np.all(Lraw[k:] == SENTINEL), "columns >= rank of L were written"
    return {"L": np.asfortranarray(Lraw[:k, :n].T), "piv": dp.cpu().numpy().astype(np.int64), "d": dd.cpu().numpy(), "rank": k,
            "resid_trace": trace.value, "thresh": thresh.value, "bytes": Lraw.tobytes() + dp.cpu().numpy().tobytes() + dd.cpu().numpy().tobytes()}


def check_factor(tag, A, g, kmax, ref):
    """everything the issue asks of a pivoted partial factor, from A's upper triangle and the GPU's L, piv, d"""
    n = A.shape[0]
    L, piv, d, k = g["L"], g["piv"], g["d"], g["rank"]
    assert sorted(piv.tolist()) == list(range(n)), "piv is not a permutation"
    assert np.all(np.diff(piv[k:]) > 0), "the rows not chosen are not ascending"
    assert np.all(np.isfinite(L)) and np.all(np.isfinite(d))
    chosen, rest = piv[:k], piv[k:]
    for j in range(k):
        assert np.all(L[chosen[:j], j] == 0.0), ("a row chosen before is not exactly zero", j)
        assert L[chosen[j], j] > 0.0, j
    assert np.all(d[chosen] == 0.0)
    # greedy: the pivot of step j is the largest of the running diagonal over the rows not yet chosen
    run = pref.running_diagonal(pref.sym(A), L, k)
    open_ = np.ones(n, dtype=bool)
    for j in range(k):
        assert L[chosen[j], j] ** 2 * (1 + 1e-10) >= run[j][open_].max(), ("greedy", j)
        open_[chosen[j]] = False
    # the stop rule, on the GPU's own d and on the threshold of the same call
    assert abs(g["thresh"] - ref["thresh"]) <= 1e-12 * abs(ref["thresh"])
    if k < kmax and len(rest):
        assert d[rest].max() <= g["thresh"] * (1 + 1e-8), (d[rest].max(), g["thresh"])
    r1, r2 = pref.residuals(A, L, piv, k, d)
    print(f"dpchol {tag}: rank {k} (restatement {ref['rank']}), residuals {r1:.3e} {r2:.3e} (restatement {ref['res'][0]:.3e} {ref['res'][1]:.3e}), "
          f"resid_trace {g['resid_trace']:.6e}, thresh {g['thresh']:.3e}")
    assert r1 <= 10.0 * max(ref["res"][0], U64), (r1, ref["res"][0])
    assert r2 <= 10.0 * max(ref["res"][1], U64), (r2, ref["res"][1])
    want = float(np.sum(d[rest]))
    assert abs(g["resid_trace"] - want) <= 1e-12 * abs(want), (g["resid_trace"], want)


@pytest.mark.parametrize("name", [c for c in pc.CASES if c not in ("one", "zero")])
def test_against_the_restatement(hip, name):
    A, tol, kmax, lda, ldl = pc.case(name)
    ref = pc.restatement(name)
    g = dpchol(hip, A, tol, kmax, lda, ldl)
    g2 = dpchol(hip, A, tol, kmax, lda, ldl)
    check_factor(name, A, g, kmax, ref)
    if name in pc.EXACT_CASES:
        assert g["rank"] == ref["rank"] == pc.EXACT_CASES[name]
    if name in pc.CAPPED_CASES:
        assert g["rank"] == ref["rank"] == pc.CAPPED_CASES[name]
    assert g2["rank"] == g["rank"] and g2["resid_trace"] == g["resid_trace"] and g2["bytes"] == g["bytes"]        # two runs give identical bytes


def test_order_one(hip):
    g = dpchol(hip, np.array([[4.0]]), -1.0, 1)
    assert g["rank"] == 1 and g["piv"].tolist() == [0] and g["L"][0, 0] == 2.0 and g["d"][0] == 0.0 and g["resid_trace"] == 0.0
    g = dpchol(hip, np.array([[4.0]]), 0.5, 1)
    assert g["rank"] == 1 and g["thresh"] == 2.0
    g = dpchol(hip, np.array([[0.0]]), -1.0, 1)
    assert g["rank"] == 0 and g["piv"].tolist() == [0]


def test_zero_matrix_has_rank_zero(hip):
    A, tol, kmax, _, _ = pc.case("zero")
    g = dpchol(hip, A, tol, kmax)
    assert g["rank"] == 0 and g["piv"].tolist() == list(range(A.shape[0])) and np.all(g["d"] == 0.0) and g["resid_trace"] == 0.0


@pytest.mark.parametrize("where", ["diagonal", "above"])
@pytest.mark.parametrize("tol", [-1.0, 1e-12])
def test_not_a_number_ends_the_call(hip, where, tol):
    """one NaN in the triangle: CAPI_OK, a rank in 0 .. max_rank and a permutation; the values are unspecified"""
    A = np.array(pc.exact_rank(*pc.EXACT[0]))
    n = A.shape[0]
    if where == "diagonal":
        A[7, 7] = np.nan
    else:
        A[3, 270] = np.nan
    g = dpchol(hip, A, tol, n)
    assert 0 <= g["rank"] <= n and sorted(g["piv"].tolist()) == list(range(n))


def test_bad_arguments_touch_nothing(hip):
    import torch
    n = 33
    A = pc.exact_rank(33, 9, 1)
    dA = place_A(A, 36)
    dL = Block(n, n, 40)
    a0, l0 = dA.raw().copy(), dL.raw().copy()
    dp = torch.full((n,), -5, dtype=torch.int32).cuda()
    dd = torch.full((n,), SENTINEL, dtype=torch.float64).cuda()
    rank, trace = C.c_int(-99), C.c_double(-99.0)
    good = dict(n=n, A=dA.ptr, lda=36, tol=-1.0, kmax=n, L=dL.ptr, ldl=40, piv=dp.data_ptr(), d=dd.data_ptr(), rank=C.byref(rank), trace=C.byref(trace))
    bad = (dict(n=0), dict(n=1 << 31), dict(lda=32), dict(ldl=32), dict(kmax=0), dict(kmax=n + 1), dict(tol=float("nan")), dict(A=None), dict(L=None),
           dict(piv=None), dict(d=None), dict(rank=None), dict(trace=None))
    for change in bad:
        a = dict(good, **change)
        rc = hip.L.capi_dpchol(hip.h, a["n"], a["A"], a["lda"], a["tol"], a["kmax"], a["L"], a["ldl"], a["piv"], a["d"], a["rank"], a["trace"])
        assert rc == EINVAL, change
    # max_rank beyond CAPI_PCHOL_MAX_RANK (the other arguments would be fine for an order that large: nothing is launched, so nothing is read)
    assert hip.L.capi_dpchol(hip.h, 5000, dA.ptr, 5000, -1.0, 4097, dL.ptr, 5000, dp.data_ptr(), dd.data_ptr(), C.byref(rank), C.byref(trace)) == EINVAL
    thresh = C.c_double(-99.0)
    assert hip.L.capi_dpchol_thresh(hip.h, n, dA.ptr, 32, -1.0, C.byref(thresh)) == EINVAL
    assert hip.L.capi_dpchol_thresh(hip.h, n, dA.ptr, 36, float("nan"), C.byref(thresh)) == EINVAL
    hip.sync()
    assert rank.value == -99 and trace.value == -99.0 and thresh.value == -99.0
    np.testing.assert_array_equal(dA.raw(), a0)
    np.testing.assert_array_equal(dL.raw(), l0)
    assert np.all(dp.cpu().numpy() == -5) and np.all(dd.cpu().numpy() == SENTINEL)


def test_the_info_word_is_not_touched(hip):
    hip.call("capi_reset_info")
    A, tol, kmax, _, _ = pc.case("pad33")
    dpchol(hip, A, tol, kmax)
    assert hip.info() == 0
