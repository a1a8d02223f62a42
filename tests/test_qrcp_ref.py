"""CPU: tests/_qrcp_ref.py, the numpy restatement of capi_dgeqp3's step rule and of the capi_dgelsy path, against scipy (LAPACK's dgeqp3 and dgelsy) on
the shapes the GPU tests use.  The case builders assert that the references can agree at all: a pivot gap at every step and sigma_{k+1} / sigma_1 <=
1e-15 under the planted rank.  Every comparison prints err/tol before it asserts."""
import numpy as np
import pytest
import scipy.linalg as sla

import _qrcp_ref as ref
from _qrcp_ref import U64

CB = 10.0


def _check(what, err, tol):
    print(f"{what}: err/tol {err:.3e}/{tol:.1e} = {err / tol:.3f}")
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize("mr,n,pad,seed", ref.GEQP3_SHAPES, ids=ref.GEQP3_IDS)
def test_geqp3_against_scipy(mr, n, pad, seed):
    W, (image, tau, jpvt, k, gaps) = ref.geqp3_case(mr, n, seed)
    Qs, Rs, Ps = sla.qr(W, pivoting=True)
    print(f"{mr}x{n}: rank {k}, largest runner-up / pivot {max(gaps) if gaps else 0.0:.9f}")
    assert sorted(jpvt) == list(range(n))
    assert np.array_equal(jpvt[:k], Ps[:k])
    d, ds = np.abs(np.diag(image))[:k], np.abs(np.diag(Rs))[:k]
    _check(f"{mr}x{n} |diag R|", np.abs(d - ds).max() / ds[0], 1e-13)
    e_fac, e_orth = ref.factor_errors(W, image, tau, jpvt, k)
    es = float(np.linalg.norm(W[:, Ps] - Qs @ Rs) / np.linalg.norm(W))
    _check(f"{mr}x{n} ||W P - Q R|| / ||W||", e_fac, CB * max(es, U64))
    _check(f"{mr}x{n} ||Q^T Q - I||", e_orth, CB * max(float(np.linalg.norm(Qs.T @ Qs - np.eye(mr))), U64))
    assert np.all(tau[k:] == 0.0)


@pytest.mark.parametrize("m,n,k,smin,seed", ref.GELSY_SHAPES, ids=ref.GELSY_IDS)
def test_two_stage_rank_pivots_and_minimum_norm(m, n, k, smin, seed):
    """A = Q1 R1, R1 P = Q2 R finds the planted rank at rcond = 1e-13, picks the pivots of scipy's dgeqp3 on A itself, and its minimum-norm X is as close
    to the planted one as scipy's dgelsy"""
    A, B, x_true, _, _ = ref.gelsy_case(m, n, k, smin, seed)
    X, kk, jpvt, F, tauf = ref.gelsy(A, B, ref.RCOND, True)
    assert kk == k
    _, Rs, Ps = sla.qr(A, mode="economic", pivoting=True)
    ds = np.abs(np.diag(Rs))
    assert int(np.sum(ds > ref.RCOND * ds[0])) == k
    assert np.array_equal(jpvt[:k], Ps[:k])
    _check(f"{m}x{n} |diag R| against dgeqp3 on A", np.abs(np.abs(np.diag(F))[:k] - ds[:k]).max() / ds[0], 1e-13)
    Xs, _, ks, _ = sla.lstsq(A, B, cond=ref.RCOND, lapack_driver="gelsy")
    assert ks == k
    e, es = ref.eta(X, x_true), ref.eta(Xs, x_true)
    _check(f"{m}x{n} minimum-norm eta (scipy gelsy {es:.3e})", e, CB * max(es, U64))
    # the basic solution: nonzeros in the pivot columns only
    Xb, kb, jb, _, _ = ref.gelsy(A, B, ref.RCOND, False)
    assert kb == k and np.all(Xb[jb[k:]] == 0.0)


def test_stop_rule_and_edge_cases():
    W = np.zeros((5, 4))
    image, tau, jpvt, k, _ = ref.geqp3(W, 0.0)
    assert k == 0 and list(jpvt) == [0, 1, 2, 3] and np.all(tau == 0.0)
    rng = np.random.default_rng(3)
    W = rng.standard_normal((12, 6))
    W[:, 4] = W[:, 1]                                                     # a duplicated column: the tie goes to the first index
    image, tau, jpvt, k, _ = ref.geqp3(W, 1e-13)
    assert k == 5 and list(jpvt).index(1) < 5 and jpvt[5] == 4
    W = rng.standard_normal((6, 6))
    W[2, 3] = np.nan
    image, tau, jpvt, k, _ = ref.geqp3(W, 0.0)
    assert 0 <= k <= 6 and sorted(jpvt) == list(range(6))
