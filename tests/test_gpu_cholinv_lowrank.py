"""cholesky::cholinv::lowrank_prepare / lowrank_solve / lowrank_quadratic_forms through driver.Cholinv on the GPU: M = L L^T + D on the factor that
factor_pivoted() leaves, on the cases of tests/_lowrank_cases.py.

What the device is measured against.  M is DEFINED by the resident L and d -- A is not read by any of these operations -- so the longdouble reference of a
device run is the Cholesky solve of L_dev L_dev^T + diag(d_dev), with the L and the Schur diagonal that the device's own factor_pivoted() returned (the
same A, tolerance and cap as the restatement's; the ranks must agree).  The two L differ in the last bits, and kappa(M) of those bits would drown the
error that is to be measured: 10 e_rest is 1e-14 .. 3e-11 here, kappa(M) u is 1e-12 .. 5e-8.  e_rest, the restatement's own error, is taken on the
restatement's L against its own reference (tests/_lowrank_cases.py): the same algorithm on the same problem to the last bits of its input.

Per gated case (||C||_1 u <= 1e-7), at r = 3 and r = 33 right-hand sides (the first 3 and all of the case's 33):
  X              per column, relative 2-norm error <= 10 max(e_rest, 8 u), e_rest over that column set (the 10 x rule) -- and <= 16 ||C||_1 u
  residual norms |resnorm_j - ||b_j - (L (L^T x_j) + d x_j)||_2| <= 1e-10 || |L| (|L|^T |x_j|) + d |x_j| + |b_j| ||_2, numpy on the returned X and the device's L
  logdet         within 64 u S + 64 k ||C||_1 u of the reference
  cnorm1         within 1e-12 of numpy's ||C||_1 on the restatement's C, the restatement run on the device's L and d like everything else (on rbf700 the
                 two L differ by 1e-10 in ||C||_1: the late pivots of a kernel matrix are differences of O(1) numbers at the 1e-8 level)
  quadratic forms  within 16 ||C||_1 u sum b^2 / d of the reference
A report-only case is asked for finite results; its errors are printed beside ||C||_1 u.  set_A gets NaN below the diagonal: only the upper triangle of A
is ever read."""
import numpy as np
import pytest

import _lowrank_cases as lc
import _lowrank_ref as lref
import _pchol_cases as pc
from _lowrank_ref import U64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def drv():
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    yield driver
    driver.finalize()


def upper_only(A):
    n = A.shape[0]
    return np.where(np.arange(n)[:, None] > np.arange(n)[None, :], np.nan, A)


def pivoted(drv, name):
    """a Cholinv on the case's A with its factor_pivoted() done, as the restatement's was"""
    A, tol, kmax, _, _ = pc.case(name)
    p = drv.Cholinv(A.shape[0])
    p.set_A(upper_only(A))
    rank, _, _ = p.factor_pivoted(rtol=0.0 if tol < 0 else tol, max_rank=kmax)
    assert rank == pc.restatement(name)["rank"]
    return p


@pytest.mark.parametrize("name,label", lc.CASES, ids=["-".join(c) for c in lc.CASES])
def test_solve_logdet_and_quadratic_forms(drv, name, label):
    shift, diag, schur = lc.diag_args(name, label)
    rs = lc.restated(name, label)
    gated = lc.gated(name, label)
    p = pivoted(drv, name)
    try:
        n = p.n
        B = lc.rhs(n)
        out = p.lowrank_prepare(shift=shift, diag=diag, schur=schur)
        L, k = p.L_pivoted(), out["rank"]
        d = lref.diag_vector(n, shift, diag, p.schur_diagonal() if schur else None)
        X3, res3 = p.lowrank_solve(B[:, :3])
        X33, res33 = p.lowrank_solve(B)
        Xn, none = p.lowrank_solve(B, residual=False)
        q = p.lowrank_quadratic_forms(B)
        assert p.lowrank_logdet() == out["logdet"]
    finally:
        p.close()
    assert k == L.shape[1] and none is None and Xn.tobytes() == X33.tobytes()
    assert X33[:, :3].tobytes() == X3.tobytes() and res33[:3].tobytes() == res3.tobytes()       # a column does not depend on its neighbours
    for a in (X33, res33, q, np.array([out["logdet"], out["cnorm1"]])):
        assert np.all(np.isfinite(a))
    Xr, ldr, qr = lref.reference(L, d, B)
    cu = out["cnorm1"] * U64
    err = lref.column_errors(X33, Xr)
    e_rest = lc.restatement_errors(name, label)
    b2 = np.sum(B * B / d[:, None], axis=0)
    eq = np.abs(q - qr) / b2
    prep = lref.prepare(L, d)
    el, bl = abs(out["logdet"] - ldr), 64 * U64 * prep["S"] + 64 * k * cu
    res_np = lref.residual_norms(L, d, B, X33)
    res_scale = lref.residual_scale(L, d, B, X33)
    print(f"lowrank {name} {label} ({'gated' if gated else 'report-only'}): k {k} |C|_1 u {cu:.2e}  X err r=3 {err[:3].max():.2e} (restatement {e_rest[:3].max():.2e}) "
          f"r=33 {err.max():.2e} (restatement {e_rest.max():.2e}) = {err.max() / cu:.3f} |C|_1 u  q err {eq.max():.2e} = {eq.max() / cu:.3f} |C|_1 u  "
          f"relres {float(np.max(res33 / np.linalg.norm(B, axis=0))):.2e}  resnorm diff {float(np.max(np.abs(res33 - res_np) / res_scale)):.2e} of its scale  "
          f"logdet err {el:.2e} = {el / bl:.2e} of its bound  cnorm1 {out['cnorm1']:.15e} (numpy on the device's L {prep['cnorm1']:.15e}, on the restatement's L {rs['prep']['cnorm1']:.15e})")
    if not gated:
        return
    assert cu <= lc.GATE
    for cols in (slice(0, 3), slice(0, 33)):
        assert err[cols].max() <= 10.0 * max(e_rest[cols].max(), 8 * U64), (name, label, cols)
        assert err[cols].max() <= 16.0 * cu
    assert np.all(np.abs(res33 - res_np) <= 1e-10 * res_scale)
    assert el <= bl
    assert abs(out["cnorm1"] - prep["cnorm1"]) <= 1e-12 * prep["cnorm1"]
    assert np.all(eq <= 16.0 * cu)


def test_uniform_shift_twice_reuses_the_gram_matrix(drv):
    """sigma^2 = 1e-2 abar, then 1e-6 abar on one factor: the second prepare runs on the cached G = L^T L and gives the bytes of a fresh object prepared at
    1e-6 abar directly.  A new factor_pivoted() discards both G and the prepared state."""
    name = "rbf700"
    a = lc.abar(name)
    B = lc.rhs(700)[:, :3]
    p, fresh = pivoted(drv, name), pivoted(drv, name)
    try:
        first = p.lowrank_prepare(shift=1e-2 * a)
        X1, _ = p.lowrank_solve(B)
        second = p.lowrank_prepare(shift=1e-6 * a)
        X2, res2 = p.lowrank_solve(B)
        q2 = p.lowrank_quadratic_forms(B)
        direct = fresh.lowrank_prepare(shift=1e-6 * a)
        Xd, resd = fresh.lowrank_solve(B)
        qd = fresh.lowrank_quadratic_forms(B)
        assert first["logdet"] != second["logdet"] and X1.tobytes() != X2.tobytes()
        assert second == direct
        assert X2.tobytes() == Xd.tobytes() and res2.tobytes() == resd.tobytes() and q2.tobytes() == qd.tobytes()
        # a new factor: the prepared state is gone, and so is G
        rank, _, _ = p.factor_pivoted(max_rank=20)
        assert rank == 20
        with pytest.raises(drv.DriverError, match="lowrank_prepare"):
            p.lowrank_solve(B)
        with pytest.raises(drv.DriverError):
            p.lowrank_logdet()
        out = p.lowrank_prepare(shift=1e-2 * a)
        X20, _ = p.lowrank_solve(B)
        L, d = p.L_pivoted(), np.full(700, 1e-2 * a)
    finally:
        p.close()
        fresh.close()
    assert out["rank"] == 20 and L.shape == (700, 20)
    Xr, ldr, _ = lref.reference(L, d, B)
    prep = lref.prepare(L, d, uniform=True)
    cu = out["cnorm1"] * U64
    err = lref.column_errors(X20, Xr)
    print(f"lowrank rbf700 k=20 after a new factor_pivoted: |C|_1 u {cu:.2e}  X err {err.max():.2e}  logdet err {abs(out['logdet'] - ldr):.2e}")
    assert err.max() <= 16.0 * cu
    assert abs(out["logdet"] - ldr) <= 64 * U64 * prep["S"] + 64 * 20 * cu
    assert abs(out["cnorm1"] - prep["cnorm1"]) <= 1e-12 * prep["cnorm1"]


def test_order_2500_across_tiles(drv):
    """spd2500cap130 (n = 2500, k = 130: C crosses a 128-tile, L several row tiles), FITC's diagonal with shift 1e-3.  No longdouble reference at this
    size: the residual is held to 10 x the restatement's on the same L and d, and X to 16 ||C||_1 u of the restatement's."""
    name = "spd2500cap130"
    p = pivoted(drv, name)
    try:
        n = p.n
        B = lc.rhs(n)
        out = p.lowrank_prepare(shift=1e-3, schur=True)
        L, d = p.L_pivoted(), lref.diag_vector(n, 1e-3, None, p.schur_diagonal())
        X, res = p.lowrank_solve(B)
        q = p.lowrank_quadratic_forms(B)
    finally:
        p.close()
    assert out["rank"] == 130
    prep = lref.prepare(L, d)
    Xs = lref.solve(L, d, prep["Rc"], B)
    qs, b2 = lref.quadratic_forms(L, d, prep["Rc"], B)
    bn = np.linalg.norm(B, axis=0)
    rel, rel_s = lref.residual_norms(L, d, B, X) / bn, lref.residual_norms(L, d, B, Xs) / bn
    cu = out["cnorm1"] * U64
    err = lref.column_errors(X, Xs)
    print(f"lowrank {name}: |C|_1 u {cu:.2e}  relres {rel.max():.2e} (restatement {rel_s.max():.2e})  X against the restatement {err.max():.2e} = {err.max() / cu:.3f} |C|_1 u  "
          f"q {float(np.max(np.abs(q - qs) / b2)):.2e}  logdet {out['logdet']:.12e} (restatement {prep['logdet']:.12e})")
    assert rel.max() <= 10.0 * rel_s.max()
    assert err.max() <= 16.0 * cu
    assert np.all(np.abs(res - lref.residual_norms(L, d, B, X)) <= 1e-10 * lref.residual_scale(L, d, B, X))
    assert np.all(np.abs(q - qs) <= 16.0 * cu * b2)
    assert abs(out["logdet"] - prep["logdet"]) <= 64 * U64 * prep["S"] + 64 * 130 * cu
    assert abs(out["cnorm1"] - prep["cnorm1"]) <= 1e-12 * prep["cnorm1"]


def test_the_factors_of_factor_are_left_alone(drv):
    n = 300
    B = np.asfortranarray(np.random.default_rng(n).standard_normal((n, 3)))
    p = drv.Cholinv(n)
    try:
        p.generate()
        p.factor()
        A0, R0 = p.A(), p.R()
        X0, res0 = p.solve(B)
        rank, _, _ = p.factor_pivoted(max_rank=20)
        assert rank == 20
        out = p.lowrank_prepare(shift=0.5)
        Xl, _ = p.lowrank_solve(B)
        assert out["rank"] == 20 and np.all(np.isfinite(Xl))
        X1, res1 = p.solve(B)
        assert X1.tobytes() == X0.tobytes() and res1.tobytes() == res0.tobytes()
        assert p.A().tobytes() == A0.tobytes() and p.R().tobytes() == R0.tobytes()
        p.factor()                                                                # .. and factor() still runs and reports a clean info word
        assert p.R().tobytes() == R0.tobytes()
    finally:
        p.close()


def test_refusals_leave_the_operator_unprepared(drv):
    name = "exact300"                                                            # rank 40 of 300: forty chosen rows have Schur diagonal 0
    A = pc.case(name)[0]
    n = A.shape[0]
    B = lc.rhs(n)[:, :3]
    p = drv.Cholinv(n)
    try:
        p.set_A(upper_only(A))

        def refused():
            with pytest.raises(drv.DriverError):
                p.lowrank_solve(B)
            with pytest.raises(drv.DriverError):
                p.lowrank_quadratic_forms(B)

        with pytest.raises(drv.DriverError, match="factor_pivoted"):             # before any factor_pivoted
            p.lowrank_prepare(shift=1.0)
        refused()
        rank, _, _ = p.factor_pivoted(rtol=pc.EXACT_TOL)
        refused()                                                                 # factored, not prepared
        sd = p.schur_diagonal()
        assert np.all(sd[p.piv()[:rank]] == 0.0)
        first_bad = int(np.flatnonzero(~(sd > 0.0))[0])
        with pytest.raises(drv.DriverError, match=r"d_%d \(1-based\)" % (first_bad + 1)):
            p.lowrank_prepare(shift=0.0, schur=True)                              # d = the Schur diagonal alone: 0 at every chosen row
        refused()
        with pytest.raises(drv.DriverError, match=r"d_1 \(1-based\)"):
            p.lowrank_prepare(shift=0.0)                                          # d = 0 everywhere
        refused()
        p.lowrank_prepare(shift=1.0)                                              # a prepared operator ..
        p.lowrank_solve(B)
        for bad in (-1.0, float("nan"), float("inf")):                            # .. is unprepared by a refused prepare
            with pytest.raises(drv.DriverError):
                p.lowrank_prepare(shift=bad)
            refused()
        with pytest.raises(drv.DriverError):
            p.lowrank_prepare(shift=1.0, diag=np.ones(n - 1))
        refused()
        p.lowrank_prepare(shift=1.0)
        with pytest.raises(drv.DriverError):
            p.lowrank_solve(np.ones((n - 1, 2)))
        with pytest.raises(drv.DriverError):
            p.lowrank_quadratic_forms(np.ones((n - 1, 2)))
        X, _ = p.lowrank_solve(B)                                                 # a refused B leaves the prepared operator as it is
        assert np.all(np.isfinite(X))
    finally:
        p.close()


def test_two_identical_solves_return_the_same_bytes(drv):
    p = pivoted(drv, "rbf700cap33")
    try:
        B = lc.rhs(700)
        p.lowrank_prepare(shift=1e-4, schur=True)
        X1, r1 = p.lowrank_solve(B)
        q1 = p.lowrank_quadratic_forms(B)
        X2, r2 = p.lowrank_solve(B)
        q2 = p.lowrank_quadratic_forms(B)
    finally:
        p.close()
    assert X1.tobytes() == X2.tobytes() and r1.tobytes() == r2.tobytes() and q1.tobytes() == q2.tobytes()
