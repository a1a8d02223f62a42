"""The oracle's extended-precision validators (oracle/capital_oracle.c: orc_ld_*), pinned on inputs whose answer is known:
an exactly representable Cholesky pair, a one-ulp change worked out by hand in rational arithmetic, mpmath at 50 digits,
and the probe form against the full form."""
from fractions import Fraction

import numpy as np
import pytest

from _conditioning import f3_exact


def _int_pair(n, seed):
    rng = np.random.default_rng(seed)
    R = np.asfortranarray(np.triu(rng.integers(-3, 4, (n, n)).astype(float), 1) + np.diag(rng.integers(1, 9, n).astype(float)))
    return np.asfortranarray(R.T @ R), R


@pytest.mark.parametrize("n,seed", [(1, 0), (7, 1), (40, 2), (200, 3)])
def test_cholesky_backward_exact_pair_is_zero(oracle, n, seed):
    A, R = _int_pair(n, seed)
    assert oracle.ld_cholesky_backward(A, R) == 0.0
    A3, R3 = f3_exact(n, seed)
    assert oracle.ld_cholesky_backward(A3, R3) == 0.0


def test_cholesky_backward_reads_upper_triangles_only(oracle):
    A, R = _int_pair(30, 4)
    R2 = R.copy(order="F")
    R2[3, 5] += 1.0
    want = oracle.ld_cholesky_backward(A, R2)
    An, Rn = A.copy(order="F"), R2.copy(order="F")
    low = np.tril(np.ones(A.shape, bool), -1)
    An[low], Rn[low] = np.nan, np.nan
    assert oracle.ld_cholesky_backward(An, Rn) == want > 0


@pytest.mark.parametrize("i,j", [(0, 0), (2, 9), (5, 5), (0, 11), (11, 11)])
def test_cholesky_backward_one_ulp(oracle, i, j):
    """R' = R* + delta e_i e_j^T changes R'^T R' in row / column j only: E_jb = E_bj = -delta R*_ib (b != j), E_jj = -(2 delta R*_ij + delta^2)."""
    n = 12
    A, R = _int_pair(n, 11)
    d = np.spacing(abs(R[i, j])) if R[i, j] != 0 else np.spacing(1.0)
    R2 = R.copy(order="F")
    R2[i, j] += d
    dd = Fraction(float(R2[i, j])) - Fraction(float(R[i, j]))
    err2 = sum(2 * (dd * Fraction(float(R[i, b]))) ** 2 for b in range(n) if b != j)
    err2 += (2 * dd * Fraction(float(R[i, j])) + dd * dd) ** 2
    ctl2 = sum(Fraction(float(x)) ** 2 for x in A.ravel())
    want = float(np.sqrt(float(err2 / ctl2)))
    got = oracle.ld_cholesky_backward(A, R2)
    assert abs(got - want) <= 1e-6 * want, (got, want)


def _mp():
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 50
    return mpmath


def test_ld_validators_agree_with_mpmath(oracle):
    """fp64 inputs with residuals at the u level: the long-double results agree with 50-digit arithmetic to 1e-3 relative (fp64
    arithmetic would not get the first digit right: the residual is the size of its own rounding there)."""
    mp = _mp()
    n, m = 10, 24
    rng = np.random.default_rng(5)
    R = np.asfortranarray(np.triu(rng.random((n, n))) + np.eye(n))
    A = np.asfortranarray(R.T @ R)                                  # rounded: A - R^T R is O(u)
    X = np.asfortranarray(np.triu(np.linalg.inv(R)))
    Q = np.asfortranarray(np.linalg.qr(rng.random((m, n)))[0])
    Rq = np.asfortranarray(np.triu(rng.random((n, n))))
    Aq = np.asfortranarray(Q @ Rq)
    M = lambda a: mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.asarray(a)])
    fro = lambda a: mp.sqrt(sum(a[i, j] ** 2 for i in range(a.rows) for j in range(a.cols)))
    mA, mR, mX, mQ, mRq, mAq = M(A), M(R), M(X), M(Q), M(Rq), M(Aq)
    want = fro(mA - mR.T * mR) / fro(mA)
    assert want > 0
    assert abs(oracle.ld_cholesky_backward(A, R) - float(want)) <= 1e-3 * float(want)
    I = mp.eye(n)
    for side, E, P in ((0, mX * mR - I, (abs(X), abs(R))), (1, mR * mX - I, (abs(R), abs(X)))):
        e, mag = oracle.ld_inverse_residual(X, R, side)
        assert abs(e - float(fro(E))) <= 1e-3 * float(fro(E))
        assert abs(mag - float(fro(M(P[0]) * M(P[1])))) <= 1e-12 * mag
    orth, res = oracle.ld_qr(Aq, Q, Rq)
    wo, wr = fro(mQ.T * mQ - I), fro(mAq - mQ * mRq) / fro(mAq)
    assert abs(orth - float(wo)) <= 1e-3 * float(wo)
    assert abs(res - float(wr)) <= 1e-3 * float(wr)
    B = np.asfortranarray(rng.random((n, 3)))
    Cm = np.asfortranarray(R @ B / 3.0)
    r, mag, cn = oracle.ld_gemm_residual(R, B, 3.0, Cm)
    wg = fro(mR * M(B) - 3 * M(Cm))
    assert abs(r - float(wg)) <= 1e-3 * float(wg)


@pytest.mark.parametrize("seed", range(5))
def test_cholesky_probe_tracks_the_full_form(oracle, seed):
    """||(A - R^T R) V|| / ||A V|| with four random columns against ||A - R^T R|| / ||A||: within a factor of 3 on random
    symmetric perturbations of several sizes."""
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(50, 400))
    R = np.asfortranarray(np.triu(rng.random((n, n))) + np.sqrt(n) * np.eye(n))
    E = rng.standard_normal((n, n)) * 10.0 ** rng.uniform(-14, -8)
    A = np.asfortranarray(R.T @ R + (E + E.T))
    full = oracle.ld_cholesky_backward(A, R)
    probe = oracle.ld_cholesky_probe(A, R, k=4, seed=seed)
    assert full / 3 <= probe <= 3 * full, (n, full, probe)


def test_families_are_what_they_claim(oracle):
    """F3's factor is exact for the oracle's dpotrf up to rounding, F4 fails first at pivot k + 1, F5's inverse is exact."""
    from _conditioning import f4_indefinite, f5_kahan
    A, Rs = f3_exact(300, 7)
    R = A.copy(order="F")
    assert oracle.dpotrf(1, R) == 0
    assert np.abs(np.triu(R) - Rs).max() <= 1e-12 * np.abs(Rs).max()
    for ks in ((0,), (1,), (17,), (128, 200), (299,)):
        B = f4_indefinite(300, ks, seed=3).copy(order="F")
        assert oracle.dpotrf(1, B) == min(ks) + 1
    for uplo in (0, 1):
        T, X = f5_kahan(200, uplo, scale_seed=uplo)
        np.testing.assert_array_equal(T @ X, np.eye(200))
