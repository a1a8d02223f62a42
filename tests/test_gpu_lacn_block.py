"""capi_dlacn_block (capital_amd/csrc/bounds_f64.hip): the Hager-Higham 1-norm estimator (LAPACK dlacn2) for r columns in lockstep, driven through the
C-ABI with an operator of the test's own: capi_dgemm with an explicit symmetric integer matrix M (n = 200, entries in -4..4), and power-of-two
weight vectors.  Against a numpy restatement of the recurrence, column by column.

What is exact.  Sign vectors and unit vectors times M, times powers of two, are integers times powers of two: every such product and every sum of
them is exact in fp64 in any order, so the estimate -- the 1-norm of such a vector -- must be EQUAL.  Two vectors of the recurrence are not of that
kind: the start x = 1/n (its product decides only signs, and a comparison est <= estold between numbers two orders of magnitude apart) and the
last stage's x_i = (-1)^i (1 + i / (n - 1)), whose value t = 2 ||M x||_1 / (3 n) enters as max(est, t).  M has no zero row sum, so the signs of the
first product do not hang on rounding; where t wins, the estimate is compared to 1e-13 instead (stated in the assertion below).

What the estimate bounds.  With weights the operator is diag(w) M (the products of dlacn2's KASE 1 are scaled after, those of KASE 2 before the
product): est <= ||diag(w) M||_1 = ||M diag(w)||_inf, evaluated exactly."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_resid_sym import EINVAL, In, Out, norms_out

pytestmark = pytest.mark.gpu
N = 200
ITMAX = 5


def sym_int_matrix(n, seed):
    rng = np.random.default_rng(seed)
    U = rng.integers(-4, 5, (n, n))
    M = np.triu(U) + np.triu(U, 1).T
    for i in np.flatnonzero(M.sum(axis=1) == 0):          # no zero row sum: sign(M (1/n)) must not hang on the rounding of 1/n
        M[i, i] += 1 if M[i, i] < 4 else -1
    assert (M == M.T).all() and (M.sum(axis=1) != 0).all() and np.abs(M).max() <= 4
    return np.asfortranarray(M.astype(np.float64))


def weights(n, spec):
    """one column per (big, seed): powers of two in 2^-2 .. 2^2, `big` of them raised to 2^10.  A few dominant weights make the estimator climb:
    over a random M with even weights it finds its column at the first attempt"""
    cols = []
    for big, seed in spec:
        rng = np.random.default_rng(100 * big + seed)
        w = np.ldexp(1.0, rng.integers(-2, 3, n))
        w[rng.permutation(n)[:big]] = 2.0 ** 10
        cols.append(w)
    return np.asfortranarray(np.array(cols).T)


def sgn(x):
    return np.where(x >= 0, 1.0, -1.0)


def restated(M, w):
    """dlacn2's recurrence for one column, as include/capital_hip.h and csrc/bounds_f64.hip state it; w None: the plain norm.  Returns (est, products, the last stage's value won)"""
    n = M.shape[0]
    w = np.ones(n) if w is None else w
    kase1 = lambda x: (M @ x) * w                          # diag(w) M x
    kase2 = lambda x: M @ (x * w)                          # its transpose
    x = kase1(np.full(n, 1.0 / n))
    applies = 1
    if n == 1:
        return abs(x[0]), applies, False
    est = np.abs(x).sum()
    isgn = sgn(x)
    x = kase2(isgn)
    applies += 1
    j = int(np.argmax(np.abs(x)))
    it = 2
    while True:
        e = np.zeros(n)
        e[j] = 1.0
        x = kase1(e)
        applies += 1
        estold, est = est, np.abs(x).sum()
        if (sgn(x) == isgn).all() or est <= estold:
            break
        isgn = sgn(x)
        x = kase2(isgn)
        applies += 1
        jlast, j = j, int(np.argmax(np.abs(x)))
        if abs(x[jlast]) != abs(x[j]) and it < ITMAX:
            it += 1
            continue
        break
    alt = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1.0 + np.arange(n) / (n - 1))
    x = kase1(alt)
    applies += 1
    t = 2.0 * (np.abs(x).sum() / (3 * n))
    return max(est, t), applies, t > est


def run_protocol(hip, M, Wt, r):
    """drives the estimator with capi_dgemm as the operator.  Returns (est, products per column, est after every call)"""
    from capital_amd import capi
    import torch
    n = M.shape[0]
    dM = In(M, n + 3)
    dW = In(Wt, n + 1) if Wt is not None else None
    xs = [Out(np.full((n, r), np.nan)), Out(np.full((n, r), np.nan))]
    est = Out(np.full((r, 1), -1.0))
    nbytes = hip.L.capi_dlacn_state_bytes(n, r)
    assert nbytes >= 8 * r * n
    state = torch.full((nbytes // 8 + 2,), float("nan"), dtype=torch.float64, device="cuda")
    active = C.c_int(-5)
    step = lambda init, x: hip.call("capi_dlacn_block", init, n, r, x.ptr, x.ld, dW.ptr if dW else None, dW.ld if dW else 0, state.data_ptr(), est.ptr,
                                    C.byref(active))
    step(1, xs[0])
    assert active.value == r
    np.testing.assert_array_equal(est.get()[:, 0], np.full(r, -1.0))          # est is written when a column finishes, not before
    applies, done_at, history = 0, np.zeros(r, int), []
    while active.value > 0:
        assert applies < 11, "still active after 11 products"
        hip.call("capi_dgemm", capi.NOTRANS, capi.NOTRANS, n, r, n, 1.0, dM.ptr, dM.ld, xs[0].ptr, xs[0].ld, 0.0, xs[1].ptr, xs[1].ld)
        xs.reverse()
        applies += 1
        step(0, xs[0])
        x = xs[0].get()
        frozen = ~x.any(axis=0)
        done_at[(done_at == 0) & frozen] = applies
        assert active.value == r - frozen.sum()
        history.append(est.get()[:, 0].copy())
    # a further call: nothing is active, nothing moves
    hip.call("capi_dgemm", capi.NOTRANS, capi.NOTRANS, n, r, n, 1.0, dM.ptr, dM.ld, xs[0].ptr, xs[0].ld, 0.0, xs[1].ptr, xs[1].ld)
    step(0, xs[1])
    assert active.value == 0
    history.append(est.get()[:, 0].copy())
    return history[-1], done_at, history


def check(hip, M, Wt, r):
    n = M.shape[0]
    got, done_at, history = run_protocol(hip, M, Wt, r)
    for j in range(r):
        w = Wt[:, j] if Wt is not None else None
        ref, applies, last_won = restated(M, w)
        exact = (np.abs(M) * (w[:, None] if w is not None else 1.0)).sum(axis=0).max()
        print(f"dlacn n={n} column {j}: est {got[j]:.17g} (restated {ref:.17g}), products {done_at[j]} ({applies}), ||diag(w) M||_1 = {exact:.17g}, "
              f"ratio {got[j] / exact:.3f}{', the last stage won' if last_won else ''}")
        assert done_at[j] == applies <= 11
        if last_won:
            assert abs(got[j] - ref) <= 1e-13 * ref               # t is a sum of rounded terms: see the module's docstring
        else:
            assert got[j] == ref
        assert got[j] <= exact
        for k, e in enumerate(history):                           # untouched before the column finishes, frozen after
            assert e[j] == (got[j] if k + 1 >= done_at[j] else -1.0)
    return done_at


def test_five_columns_finish_at_different_steps(hip):
    M = sym_int_matrix(N, 1)
    Wt = weights(N, [(2, 1), (5, 3), (14, 22), (0, 1), (5, 15)])
    done_at = check(hip, M, Wt, 5)
    np.testing.assert_array_equal(done_at, [5, 7, 9, 5, 7])       # (what the restatement gives on these inputs: three different lengths)


def test_no_weights(hip):
    check(hip, sym_int_matrix(N, 8), None, 3)


def test_order_one(hip):
    """n = 1 finishes after the first product with est = |x|"""
    M = np.asfortranarray([[-3.0]])
    got, done_at, _ = run_protocol(hip, M, np.asfortranarray([[0.5, 4.0]]), 2)
    np.testing.assert_array_equal(got, [1.5, 12.0])
    np.testing.assert_array_equal(done_at, [1, 1])
    got, done_at, _ = run_protocol(hip, M, None, 1)
    assert got[0] == 3.0 and done_at[0] == 1


def test_refusals(hip):
    import torch
    n, r = 50, 2
    x = Out(np.full((n, r), 1.0))
    est = Out(np.full((r, 1), -1.0))
    state = torch.full((hip.L.capi_dlacn_state_bytes(n, r) // 8 + 2,), float("nan"), dtype=torch.float64, device="cuda")
    active = C.c_int(-5)
    assert hip.L.capi_dlacn_state_bytes(n, 33) == 0 and hip.L.capi_dlacn_state_bytes(0, 1) == 0
    # too many columns: nothing is touched
    assert hip.L.capi_dlacn_block(hip.h, 1, n, 33, x.ptr, x.ld, None, 0, state.data_ptr(), est.ptr, C.byref(active)) == EINVAL
    hip.sync()
    np.testing.assert_array_equal(x.get(), np.full((n, r), 1.0))
    assert torch.isnan(state).all() and active.value == -5
    # a state that no init has written is not a state of the estimator
    assert hip.L.capi_dlacn_block(hip.h, 0, n, r, x.ptr, x.ld, None, 0, state.data_ptr(), est.ptr, C.byref(active)) == EINVAL
    hip.sync()
    np.testing.assert_array_equal(est.get()[:, 0], np.full(r, -1.0))
