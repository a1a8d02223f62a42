"""cholesky::cholinv::factor_pivoted through driver.Cholinv on the GPU: the pivoted partial Cholesky where factor() refuses.

The exact-rank matrices of tests/_pchol_cases.py (n = 300 of rank 40, n = 1100 of rank 70): factor() raises on them, factor_pivoted() returns the rank
with L, piv, the Schur diagonal and the trace of what was left out, held to the criteria of tests/test_gpu_pchol.py against the numpy restatement.  And
on an SPD matrix factor_pivoted() leaves the factors of factor() alone: a solve() after it returns the bytes of a solve() before it."""
import numpy as np
import pytest

import _pchol_cases as pc
import _pchol_ref as pref
from _pchol_ref import U64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def drv():
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    yield driver
    driver.finalize()


@pytest.mark.parametrize("name", list(pc.EXACT_CASES))
def test_rank_deficient_matrix(drv, name):
    A, tol, kmax, _, _ = pc.case(name)
    ref = pc.restatement(name)
    n = A.shape[0]
    p = drv.Cholinv(n)
    try:
        p.set_A(np.where(np.arange(n)[:, None] > np.arange(n)[None, :], np.nan, A))         # the upper triangle alone is read
        with pytest.raises(drv.DriverError):
            p.factor()
        rank, trace, thresh = p.factor_pivoted(rtol=tol)
        L, piv, d = p.L_pivoted(), p.piv(), p.schur_diagonal()
    finally:
        p.close()
    assert rank == ref["rank"] == pc.EXACT_CASES[name] and L.shape == (n, rank)
    assert abs(thresh - ref["thresh"]) <= 1e-12 * ref["thresh"]
    assert sorted(piv.tolist()) == list(range(n)) and np.all(np.diff(piv[rank:]) > 0)
    chosen, rest = piv[:rank], piv[rank:]
    run = pref.running_diagonal(A, L, rank)
    open_ = np.ones(n, dtype=bool)
    for j in range(rank):
        assert np.all(L[chosen[:j], j] == 0.0) and L[chosen[j], j] > 0.0, j
        assert L[chosen[j], j] ** 2 * (1 + 1e-10) >= run[j][open_].max(), ("greedy", j)
        open_[chosen[j]] = False
    assert np.all(d[chosen] == 0.0) and d[rest].max() <= thresh * (1 + 1e-8)
    r1, r2 = pref.residuals(A, L, piv, rank, d)
    print(f"factor_pivoted {name}: rank {rank}, residuals {r1:.3e} {r2:.3e} (restatement {ref['res'][0]:.3e} {ref['res'][1]:.3e}), resid_trace {trace:.6e}")
    assert r1 <= 10.0 * max(ref["res"][0], U64) and r2 <= 10.0 * max(ref["res"][1], U64)
    want = float(np.sum(d[rest]))
    assert abs(trace - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("n", [300, 1100])
def test_the_factors_of_factor_are_left_alone(drv, n):
    B = np.asfortranarray(np.random.default_rng(n).standard_normal((n, 3)))
    p = drv.Cholinv(n)
    try:
        p.generate()
        p.factor()
        A0, R0 = p.A(), p.R()
        X0, res0 = p.solve(B)
        rank, trace, thresh = p.factor_pivoted(max_rank=20)
        assert rank == 20 and trace > 0.0 and p.L_pivoted().shape == (n, 20)
        X1, res1 = p.solve(B)
        assert X1.tobytes() == X0.tobytes() and res1.tobytes() == res0.tobytes()
        assert p.A().tobytes() == A0.tobytes() and p.R().tobytes() == R0.tobytes()
        assert p.rcond() > 0.0
    finally:
        p.close()


def test_rank_zero_and_bad_arguments_raise(drv):
    p = drv.Cholinv(64)
    try:
        p.set_A(np.zeros((64, 64)))
        with pytest.raises(drv.DriverError, match="rank 0"):
            p.factor_pivoted()
        with pytest.raises(drv.DriverError):
            p.L_pivoted()
        with pytest.raises(drv.DriverError):
            p.factor_pivoted(max_rank=65)
        with pytest.raises(drv.DriverError):
            p.factor_pivoted(rtol=-1.0)
    finally:
        p.close()
