"""CPU: the numpy restatement of the column-pivoted CholeskyQR (tests/_pcqr_ref.py) on the seeded rank-deficient panels of tests/_pcqr_cases.py.

Per case: the restatement finds exactly the planted rank -- a condition on the INPUTS, asserted here so that the rank check of the GPU tests
tests the kernel and not the data; its rank and pivots equal LAPACK's dpstrf on the same Gram matrix with the same absolute tolerance; and its
residual and orthogonality are printed beside those of scipy.linalg.qr(pivoting=True) truncated at the same rank and held to the caps that the GPU
tests use (2e-13 and 5e-14)."""
import numpy as np
import pytest
import scipy.linalg as sla

import _pcqr_cases as pc
import _pcqr_ref as pref
import _scqr_ref as ref


@pytest.mark.parametrize("m,n,k", pc.CASES, ids=pc.IDS)
def test_restatement_finds_the_planted_rank_and_lapacks_pivots(m, n, k):
    G = pc.gram(m, n, k)
    r = pc.restatement(m, n, k)
    assert r["rank"] == k
    assert sorted(r["piv"].tolist()) == list(range(n))
    c, piv, rank, info = sla.lapack.dpstrf(np.triu(G), tol=r["thresh"], lower=0)
    assert rank == k and info == (0 if k == n else 1)
    np.testing.assert_array_equal(piv[:k] - 1, r["piv"][:k])
    s = np.linalg.svd(pc.matrix(m, n, k), compute_uv=False)
    print(f"pcqr {m}x{n} rank {k}: sigma_k / sigma_1 {s[k - 1] / s[0]:.2e}, sigma_k+1 / sigma_1 {(s[k] / s[0] if k < n else 0.0):.2e}, thresh {r['thresh']:.3e}")
    assert s[k - 1] / s[0] >= 1.3e-4 and (k == n or s[k] / s[0] <= 1e-15)


@pytest.mark.parametrize("m,n,k", pc.CASES, ids=pc.IDS)
def test_restatement_beside_truncated_qrcp(m, n, k):
    A, B = pc.matrix(m, n, k), pc.rhs(m, n, k)
    r = pc.restatement(m, n, k)
    res_q, orth_q = pc.qrcp_metrics(m, n, k, k)
    X = pref.basic_solution(r["Q"], r["R"], r["piv"], B)
    ratio = np.linalg.norm(A @ X - B, axis=0) / pc.lstsq_reference(m, n, k)
    print(f"pcqr {m}x{n} rank {k}: residual {r['residual']:.3e} (QRCP {res_q:.3e}), orthogonality {r['orthogonality']:.3e} (QRCP {orth_q:.3e}), "
          f"lstsq residual ratio - 1 <= {ratio.max() - 1.0:.2e}")
    assert r["residual"] <= 2e-13 and r["orthogonality"] <= 5e-14
    assert np.all(ratio <= 1.0 + 1e-8)
    dropped = np.setdiff1d(np.arange(n), r["piv"][:k])
    assert np.all(X[dropped] == 0.0)
    # the trapezoid's invariants that the device test asks of capi_dpstrf hold for the restatement's own factor
    Rf, piv, rank, thresh = pref.pstrf(pc.gram(m, n, k), r["tol"])
    res, schur = pref.pstrf_checks(pc.gram(m, n, k), Rf, piv, rank)
    assert res <= 10 * ref.U64 and schur <= thresh * (1 + 1e-8)


def test_user_tolerance_truncates():
    """panel(8320, 130, 1e6, 5) with rtol = 1e-3: a truncated pivoted QR whose residual is QRCP's at the same rank and within the bound
    sqrt((n - k) tol trace) / ||A||_F"""
    m, n = 8320, 130
    A = ref.panel(m, n, 1e6, 5)
    o = pref.pcqr(A, rtol=1e-3)
    k = o["rank"]
    res, orth = pref.metrics(A, o["Q"], o["R"], o["piv"])
    Q, R, P = sla.qr(A, mode="economic", pivoting=True)
    res_q, _ = pref.metrics(A, Q[:, :k], R[:k], P)
    bound = np.sqrt((n - k) * o["tol"]) * np.sqrt(o["trace"]) / np.linalg.norm(A)
    print(f"pcqr rtol 1e-3: rank {k}, residual {res:.3e}, QRCP at that rank {res_q:.3e}, bound {bound:.3e}, orthogonality {orth:.3e}")
    assert 1 < k < n and o["tol"] == 1e-6
    assert res <= 1.5 * res_q and res <= 1.01 * bound and orth <= 5e-14


def test_stopping_rule_edges():
    """tol = 0 factors a full-rank G to the end; a NaN on the diagonal stops at once with a full permutation; a zero matrix has rank 0"""
    G = pc.gram(2048, 32, 32)
    assert pref.pstrf(G, 0.0)[2] == 32
    Gn = np.array(G)
    Gn[5, 5] = np.nan
    _, piv, rank, _ = pref.pstrf(Gn, 1e-10)
    assert rank == 0 and sorted(piv.tolist()) == list(range(32))
    assert pref.pstrf(np.zeros((4, 4)), 0.0)[2] == 0
