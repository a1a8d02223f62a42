"""CPU: the numpy restatement of the pivoted partial Cholesky (tests/_pchol_ref.py), which the device tests take as their reference, agrees with LAPACK's
dpstrf on every case of tests/_pchol_cases.py, and the exact-rank cases are well posed -- the rank is decided with margins that no rounding order
can cross."""
import numpy as np
import pytest
from scipy.linalg import lapack

import _pchol_cases as pc
import _pchol_ref as pref


@pytest.mark.parametrize("name", list(pc.CASES))
def test_restatement_agrees_with_dpstrf(name):
    """the same rank and the same leading pivots.  dpstrf takes the threshold as an absolute number and has no cap: of a capped case its first max_rank
    pivots are compared.  dpstrf updates the diagonal lazily, in another order, and breaks ties by position in the swapped matrix, so pivots at the
    level of the rounding noise -- thresh = n u max a_ii IS that level on the default-tolerance cases -- may come in another order: `leading` are the
    steps whose pivot is at least 1000 thresh"""
    A, tol, kmax, _, _ = pc.case(name)
    r = pc.restatement(name)
    _, lpiv, lrank, info = lapack.dpstrf(np.array(A), tol=r["thresh"], lower=0)
    assert info >= 0
    assert r["rank"] == min(lrank, kmax)
    k = r["rank"]
    assert sorted(r["piv"].tolist()) == list(range(A.shape[0]))
    pivots = np.array([r["L"][r["piv"][j], j] ** 2 for j in range(k)])
    leading = int(np.sum(pivots >= 1e3 * r["thresh"]))
    assert np.all(np.diff(pivots) <= 1e-12 * pivots[0]) if k > 1 else True, "the pivots increase"
    assert leading >= min(k, 33) and np.array_equal(lpiv[:leading] - 1, r["piv"][:leading])
    assert r["res"][0] <= 1e-15 and r["res"][1] <= 1e-16


@pytest.mark.parametrize("name", list(pc.EXACT_CASES))
def test_exact_rank_cases_are_well_posed(name):
    """if a seed fails this, change the seed and not the margins"""
    A, tol, kmax, _, _ = pc.case(name)
    r = pc.restatement(name)
    k = pc.EXACT_CASES[name]
    assert r["rank"] == k
    last = r["L"][r["piv"][k - 1], k - 1] ** 2
    rest = r["piv"][k:]
    print(f"{name}: last pivot {last / r['thresh']:.3e} thresh, largest remaining diagonal {r['d'][rest].max() / r['thresh']:.3e} thresh")
    assert last >= 1e4 * r["thresh"]
    assert r["d"][rest].max() <= 1e-3 * r["thresh"]


def test_first_pivot_of_the_kernel_matrix_is_a_tie():
    A = pc.rbf()
    assert np.all(np.diag(A) == 1.0) and pc.restatement("rbf700")["piv"][0] == 0


def test_running_diagonal_is_the_restatements():
    """d recomputed from L column by column (what the device test's greedy check uses) is the d the restatement carried, bit for bit"""
    A, _, _, _, _ = pc.case("exact300")
    r = pc.restatement("exact300")
    dd = pref.running_diagonal(A, r["L"], r["rank"])
    rest = r["piv"][r["rank"]:]
    assert np.array_equal(dd[-1][rest], r["d"][rest])
