"""CPU: the step formulas of capi_dchud / capi_dchud_inv, restated in NumPy (tests/_chud_ref.py), meet the factor and inverse criteria of the update
on their own, at the shapes of the GPU tests -- the bounds are reachable before any kernel is blamed -- and report a downdate that leaves the matrix
not positive definite."""
import numpy as np
import pytest

import _chud_ref as ref
import _conditioning as cond


@pytest.mark.parametrize("sign", [1, -1], ids=["update", "downdate"])
@pytest.mark.parametrize("r", [1, 17, 32])
@pytest.mark.parametrize("n", [33, 257, 1000])
def test_reference_meets_the_factor_and_inverse_criteria(n, r, sign):
    A0, V, A1 = ref.problem(n, r, sign)
    R0 = ref.chol_upper(A0)
    R1, log, info = ref.chud(R0, V, sign)
    assert info == 0
    assert np.array_equal(np.tril(R1, -1), np.zeros((n, n))) and (np.diag(R1) > 0).all()
    rho, rho_max = ref.factor_error(R1, A0, A1), ref.factor_bound(A0, A1)
    Ri1 = ref.chud_inv(ref.tri_inv(R0), log, sign)
    eps, eps_max = ref.inverse_error(Ri1, R1), ref.inverse_bound(A0, A1)
    print(f"chud reference n={n} r={r} sign={sign:+d}: rho {rho / ref.U64:.1f} u (bound {rho_max / ref.U64:.1f} u), "
          f"||Rinv' R' - I|| {eps:.2e} (bound {eps_max:.2e})")
    assert rho <= rho_max
    assert eps <= eps_max


@pytest.mark.parametrize("sign", [1, -1], ids=["update", "downdate"])
@pytest.mark.parametrize("n,h1", [(33, 16), (1000, 500)])
def test_reference_updates_a_block_diagonal_inverse(n, h1, sign):
    """the two step ranges [0, h1) and [h1, n) on the inverses of the diagonal blocks; what lies between them is not touched"""
    r = 17
    A0, V, A1 = ref.problem(n, r, sign)
    R0 = ref.chol_upper(A0)
    R1, log, info = ref.chud(R0, V, sign)
    assert info == 0
    Bi = np.zeros((n, n), order="F")
    Bi[:h1, :h1] = ref.tri_inv(R0[:h1, :h1])
    Bi[h1:, h1:] = ref.tri_inv(R0[h1:, h1:])
    Bi[:h1, h1:] = 7.25
    out = ref.chud_inv(ref.chud_inv(Bi, log, sign, 0, h1), log, sign, h1, n)
    assert (out[:h1, h1:] == 7.25).all() and (np.tril(out, -1) == 0).all()
    bound = ref.inverse_bound(A0, A1)
    assert ref.inverse_error(out[:h1, :h1], R1[:h1, :h1]) <= bound
    assert ref.inverse_error(out[h1:, h1:], R1[h1:, h1:]) <= bound


def test_reference_reports_a_downdate_that_is_not_positive_definite():
    T, V = np.eye(64), np.zeros((64, 1))
    V[5, 0] = 2.0
    assert ref.chud(T, V, -1)[2] == 6
    A = cond.f1_spectrum(257, 1e2)
    info = ref.chud(ref.chol_upper(A), ref.failing_v(A), -1)[2]
    assert 1 <= info <= 257
    # the same V as an update is fine
    assert ref.chud(ref.chol_upper(A), ref.failing_v(A), +1)[2] == 0


def test_reference_never_reads_below_the_diagonal():
    n, r = 33, 2
    A0, V, A1 = ref.problem(n, r, 1)
    R0 = ref.chol_upper(A0)
    dirty = R0 + np.tril(np.full((n, n), np.nan), -1)
    R1, log, info = ref.chud(dirty, V, 1)
    assert info == 0 and np.array_equal(np.triu(R1), ref.chud(R0, V, 1)[0])
