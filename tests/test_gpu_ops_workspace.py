"""The operations on the resident factors do not depend on what an earlier operation left in their workspace.

cholinv: solve, rcond, solve_expert and update take their work from one arena that is not zeroed (SaveIntermediates keeps it from call to call,
FlushIntermediates gets it anew, possibly the same memory).  Problem P first runs a solve whose right-hand sides are all NaN, which leaves NaN in
every block a solve takes, then a fixed sequence; problem Q runs the sequence alone.  Every array and scalar that the sequence returns must be the same,
bit for bit.  n = 1000 with bc_mult = -3 and split = 1: the top level splits at 500, complete_inv = 0 then takes the blocked apply with its second
work block, and n > 512 gives capi_dtrsm_thin more than one leaf.

cacqr: one object runs factor_pivoted -> lstsq -> factor -> lstsq -> svd; each result must equal, bit for bit, that of the same call on a fresh object
that ran only the step before it.  2048 x 64 takes the streaming projection, 16384 x 256 (m_loc = 64 n) the capi_dgemm projection on factor()'s pair."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1000


@pytest.fixture(scope="module")
def drv():
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    yield driver
    driver.finalize()


@pytest.fixture(scope="module")
def rhs():
    rng = np.random.default_rng(1000)
    B = np.asfortranarray(rng.standard_normal((N, 33)))
    V = np.asfortranarray(rng.standard_normal((N, 3)) * 0.25)
    for a in (B, V):
        a.setflags(write=False)
    return B, V


FORMS = {"inverse": {}, "substitution": {"substitution": True}, "trsm": {"trsm_mode": True}}
# TRSM mode with Serialize + FlushIntermediates is refused: capi_dtrsm takes full storage and only the packed R is resident
CASES = [(f, s, fl) for f, s, fl in itertools.product(FORMS, (False, True), (False, True)) if not (f == "trsm" and s and fl)]


def cholinv_sequence(drv, B, V, form, serialize, flush, poison):
    """factor, [a solve on NaN], solve(5), rcond, solve_expert(33: two column blocks), update(3), solve(5): everything returned, in order"""
    p = drv.Cholinv(N, complete_inv=0, split=1, bc_mult=-3, serialize=serialize, flush_intermediates=flush, **FORMS[form])
    try:
        p.generate()
        p.factor()
        assert p.stats()["levels"] >= 1
        if poison:
            X, res = p.solve(np.full((N, 32), np.nan, order="F"), refine=1)
            assert np.isnan(X).all() and np.isnan(res).all()
        out = {}
        out["solve5.X"], out["solve5.res"] = p.solve(B[:, :5], refine=1)
        out["rcond"], out["anorm1"], out["rcond.applies"] = p.rcond(details=True)
        out["expert33.X"], out["expert33.res"], out["expert33.ferr"], out["expert33.berr"] = p.solve_expert(B, refine=1)
        p.update(V)
        out["update.R"] = p.R()
        if form != "trsm":
            out["update.Rinv"] = p.Rinv()
        out["update.A"] = p.A()
        out["solve5b.X"], out["solve5b.res"] = p.solve(B[:, :5], refine=1)
        return out
    finally:
        p.close()


@pytest.mark.parametrize("form,serialize,flush", CASES)
def test_cholinv_results_do_not_depend_on_stale_work(drv, rhs, form, serialize, flush):
    B, V = rhs
    P = cholinv_sequence(drv, B, V, form, serialize, flush, poison=True)
    Q = cholinv_sequence(drv, B, V, form, serialize, flush, poison=False)
    assert P.keys() == Q.keys()
    for k in Q:
        assert np.isfinite(Q[k]).all(), k
        np.testing.assert_array_equal(P[k], Q[k], err_msg=k)
    assert 0.0 < Q["rcond"] <= 1.0 and Q["anorm1"] > 0.0


def planted(m, n, rank, seed):
    """(an m x n matrix of exact rank `rank`, a well-conditioned m x n matrix, m x 33 right-hand sides)"""
    rng = np.random.default_rng(seed)
    low = np.asfortranarray(rng.standard_normal((m, rank)) @ rng.standard_normal((rank, n)))
    return low, np.asfortranarray(rng.standard_normal((m, n))), np.asfortranarray(rng.standard_normal((m, 33)))


def same(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.isfinite(w).all(), (what, k)
        np.testing.assert_array_equal(g, w, err_msg=f"{what}[{k}]")


@pytest.mark.parametrize("m,n,rank", [(2048, 64, 40), (16384, 256, 200)])
def test_cacqr_results_do_not_depend_on_earlier_operations(drv, m, n, rank):
    low, full, B = planted(m, n, rank, 7 * n)

    def fresh(A):
        q = drv.Cacqr(m, n, variant=2)
        q.set_A(A)
        return q

    def pivoted(q):
        k = q.factor_pivoted()
        return k, q.piv, q.R_pivoted(), q.Q_pivoted()

    def plain(q):
        q.factor()
        return q.Q(), q.R()

    O = fresh(low)
    try:
        o_piv = pivoted(O)
        assert o_piv[0] == rank
        o_ls1 = O.lstsq(B)
        O.set_A(full)                                      # factor() needs full column rank: the Gram matrix of `low` is singular
        o_qr = plain(O)
        o_ls2 = O.lstsq(B)
        o_svd = O.svd()
    finally:
        O.close()

    F = fresh(low)                                         # factor_pivoted -> lstsq
    try:
        same(pivoted(F), o_piv, "factor_pivoted")
        same(F.lstsq(B), o_ls1, "lstsq on the pivoted factors")
    finally:
        F.close()
    F = fresh(full)                                        # factor -> lstsq
    try:
        same(plain(F), o_qr, "factor after factor_pivoted and lstsq")
        same(F.lstsq(B), o_ls2, "lstsq after factor")
    finally:
        F.close()
    F = fresh(full)                                        # factor -> svd
    try:
        F.factor()
        same(F.svd(), o_svd, "svd after lstsq")
    finally:
        F.close()
