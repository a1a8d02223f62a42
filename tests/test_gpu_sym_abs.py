"""capi_dsym_abs (W <- |S| |X| + |B| with its column maxima, S the symmetric matrix given by A's upper triangle; capital_amd/csrc/sym_apply_f64.hip)
against numpy, in the manner of test_gpu_resid_sym.py: INTEGER operands in -8..8 of both signs, so every sum is exact in fp64 whatever its order
and the comparison is for equality.  A kernel that forgets the absolute value of A, of X or of B fails on sign alone; A's lower triangle holds NaN,
so one that reads below the diagonal or multiplies an unwanted element by zero fails outright; outputs lie between sentinels."""
import numpy as np
import pytest

from test_gpu_resid_sym import EINVAL, In, Out, ints, norms_out, sym, upper_stored

pytestmark = pytest.mark.gpu


def sym_abs(h, n, r, dA, dX, dB, out, mx, raw=False):
    """dB: an In or None (the product alone); out: an Out, or None; mx: an Out (r x 1) or None"""
    args = (n, r, dA.ptr if dA else None, dA.ld if dA else 1, dX.ptr if dX else None, dX.ld if dX else 1, dB.ptr if dB is not None else None,
            dB.ld if dB is not None else 0, out.ptr if out is not None else None, out.ld if out is not None else 0, mx.ptr if mx is not None else None)
    if raw:
        rc = h.L.capi_dsym_abs(h.h, *args)
        h.sync()
        return rc
    h.call("capi_dsym_abs", *args)
    h.sync()


def reference(U, X, B=None):
    W = np.abs(sym(U)) @ np.abs(X)
    return W + np.abs(B) if B is not None else W


def run_case(h, n, r, pad, seed):
    rng = np.random.default_rng(seed)
    U, X, B = ints(rng, (n, n)), ints(rng, (n, r)), ints(rng, (n, r))
    assert n < 8 or ((U < 0).any() and (X < 0).any() and (B < 0).any())
    dA, dX, dB = In(upper_stored(U, np.nan), n + pad), In(X, n + (pad and 1)), In(B, n + 2 * pad)
    out, mx = Out(np.full((n, r), np.nan)), norms_out(r)
    sym_abs(h, n, r, dA, dX, dB, out, mx)
    ref = reference(U, X, B)
    got, gmax = out.get(), mx.get()[:, 0]
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(gmax, ref.max(axis=0))
    return U, X, B, dA, dX, dB, ref


# ragged blocks and diagonal tiles (1 .. 257), more than one line block (1000, 2050: 22 line blocks on 256 CUs); the 16-column pass boundary (16, 17),
# the threshold at which capi_dresid_sym leaves the fused kernel and this call does not (7, 8), and the most columns
NS = [1, 31, 32, 33, 255, 256, 257, 1000, 2050]
RS = [1, 7, 8, 16, 17, 32]
CASES = [(n, r, 3 * ((i + k) % 2)) for i, n in enumerate(NS) for k, r in enumerate(RS)]


@pytest.mark.parametrize("n,r,pad", CASES, ids=[f"n{n}-r{r}-ld+{pad}" for n, r, pad in CASES])
def test_against_numpy_with_nan_below_the_diagonal(hip, n, r, pad):
    run_case(hip, n, r, pad, 1000 * n + 10 * r + pad)


@pytest.mark.parametrize("n,r,pad", [(2050, 7, 3), (2050, 17, 0), (4000, 32, 3)])
def test_few_large_blocks(n, r, pad):
    """32 CUs (an own handle whose compute stream keeps 224 CUs free): 7 line blocks of 320 or 576 lines, so a block walks several super-tiles of
    256 (the X_I double buffer, the read-modify-write of the row slots), which the default plan does not at these orders"""
    from capital_amd import capi
    hnd = capi.Handle(0, own_stream=True)
    try:
        assert hnd.L.capi_reserve_cus(hnd.h, 224) == 0
        run_case(hnd, n, r, pad, 7 * n + r)
    finally:
        hnd.close()


def test_forms(hip):
    n, r = 300, 17
    U, X, B, dA, dX, dB, ref = run_case(hip, n, r, 3, 42)
    # B == NULL: the product alone
    out, mx = Out(np.full((n, r), np.nan)), norms_out(r)
    sym_abs(hip, n, r, dA, dX, None, out, mx)
    np.testing.assert_array_equal(out.get(), reference(U, X))
    np.testing.assert_array_equal(mx.get()[:, 0], reference(U, X).max(axis=0))
    # colmax == NULL: W alone
    out = Out(np.full((n, r), np.nan))
    sym_abs(hip, n, r, dA, dX, dB, out, None)
    np.testing.assert_array_equal(out.get(), ref)
    # W == NULL: the maxima alone
    mx = norms_out(r)
    sym_abs(hip, n, r, dA, dX, dB, None, mx)
    np.testing.assert_array_equal(mx.get()[:, 0], ref.max(axis=0))
    # W == B: in place (B in a guarded buffer)
    inplace, mx = Out(B), norms_out(r)
    sym_abs(hip, n, r, dA, dX, inplace, inplace, mx)
    np.testing.assert_array_equal(inplace.get(), ref)
    np.testing.assert_array_equal(mx.get()[:, 0], ref.max(axis=0))
    # n == 0: colmax <- 0
    mx = norms_out(r)
    assert sym_abs(hip, 0, r, None, None, None, None, mx, raw=True) == 0
    np.testing.assert_array_equal(mx.get()[:, 0], np.zeros(r))


@pytest.mark.parametrize("n", [257, 1000])
def test_ones_give_the_one_norm(hip, n):
    rng = np.random.default_rng(n)
    U = ints(rng, (n, n))
    mx = norms_out(1)
    sym_abs(hip, n, 1, In(upper_stored(U, np.nan), n + 3), In(np.ones((n, 1))), None, None, mx)
    assert mx.get()[0, 0] == np.linalg.norm(sym(U), 1)


def test_too_many_columns_touch_nothing(hip):
    n = 40
    rng = np.random.default_rng(3)
    U, X, B = ints(rng, (n, n)), ints(rng, (n, 33)), ints(rng, (n, 33))
    W0 = ints(rng, (n, 33))
    for r in (33, 0):
        out, mx = Out(W0), Out(np.full((33, 1), 5.0))
        assert sym_abs(hip, n, r, In(upper_stored(U, np.nan)), In(X), In(B), out, mx, raw=True) == EINVAL
        np.testing.assert_array_equal(out.get(), W0)
        np.testing.assert_array_equal(mx.get()[:, 0], np.full(33, 5.0))


@pytest.mark.parametrize("n,r", [(1000, 7), (2050, 32)])
def test_two_runs_are_bit_identical(hip, n, r):
    """random data: the sums round, in one fixed order; and they stay inside the bound of a sum of n + 1 terms in any order"""
    rng = np.random.default_rng(n + r)
    U, X, B = rng.standard_normal((n, n)), rng.standard_normal((n, r)), rng.standard_normal((n, r))
    dA, dX, dB = In(upper_stored(U, np.nan), n + 3), In(X), In(B)
    got = []
    for _ in range(2):
        out, mx = Out(np.zeros((n, r))), norms_out(r)
        sym_abs(hip, n, r, dA, dX, dB, out, mx)
        got.append((out.get(), mx.get()[:, 0]))
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()
    np.testing.assert_array_equal(got[0][1], got[0][0].max(axis=0))
    ref = reference(U.astype(np.longdouble), X.astype(np.longdouble), B.astype(np.longdouble))
    u = 2.0 ** -53
    gamma = (n + 1) * u / (1 - (n + 1) * u)
    assert np.all(np.abs(got[0][0] - ref) <= gamma * ref)
