"""CPU: the numpy restatement of the equilibration's exponent rule (tests/_equil_ref.py), which the GPU tests hold the kernels against, on the edge
diagonals: exact powers of two of both parities, the largest and the smallest normal number, subnormals down to the smallest -- the scaled diagonal
always lies in [0.5, 2), dscale is always a normal number with -537 <= e <= 512 -- and the round trip of the scaling on the graded inputs of
tests/test_gpu_cholinv_equilibrate.py, bit for bit."""
import numpy as np
import pytest

import _equil_ref as ref

F = np.finfo(np.float64)
EDGES = np.array([1.0, 2.0, 4.0, 0.5, 0.25, 2.0 ** 101, 2.0 ** 100, 2.0 ** -101, 2.0 ** -100, np.nextafter(2.0, 0), np.nextafter(1.0, 0), np.nextafter(1.0, 2), 3.0,
                  F.max, 2.0 ** 1023, F.tiny, np.nextafter(F.tiny, 0), F.tiny / 2, F.tiny / 4, 3 * F.smallest_subnormal, 2 * F.smallest_subnormal, F.smallest_subnormal])


def test_exponents_of_exact_powers_of_two_of_both_parities():
    k = np.arange(-1074, 1024)
    e = ref.exponents(np.ldexp(1.0, k.astype(np.int32)))
    # 2^k = 0.5 2^(k + 1): e = floor((k + 1) / 2), so 2^k / 2^(2 e) is 1 for even k and 0.5 for odd k
    np.testing.assert_array_equal(e, np.floor_divide(k + 1, 2))
    assert e.min() == -537 and e.max() == 512


def test_edge_diagonals_scale_into_half_to_two_with_normal_factors():
    e = ref.exponents(EDGES)
    dscale, rec = ref.poequ2(EDGES)
    assert np.all(dscale >= F.tiny) and np.all(np.isfinite(dscale)), "dscale must be a normal number"
    assert np.all((e >= -537) & (e <= 512))
    np.testing.assert_array_equal(dscale, np.ldexp(1.0, e.astype(np.int32)))
    scaled = np.ldexp(EDGES, (-2 * e).astype(np.int32))
    assert np.all((scaled >= 0.5) & (scaled < 2.0)), scaled
    np.testing.assert_array_equal(np.ldexp(scaled, (2 * e).astype(np.int32)), EDGES)       # and back, subnormals included
    assert rec[0] == 2.0 ** (int(e.min()) - int(e.max())) and rec[1] == F.max and rec[2] == F.smallest_subnormal and rec[3] == 0.0


def test_random_diagonals_over_the_whole_range():
    rng = np.random.default_rng(5)
    d = np.ldexp(rng.uniform(0.5, 1.0, 4000), rng.integers(-1073, 1025, 4000).astype(np.int32))
    d = d[(d > 0) & np.isfinite(d)]
    e = ref.exponents(d)
    scaled = np.ldexp(d, (-2 * e).astype(np.int32))
    assert np.all((scaled >= 0.5) & (scaled < 2.0))


@pytest.mark.parametrize("value", [0.0, -1.0, np.nan, np.inf, -np.inf])
def test_first_bad_entry_wins(value):
    d = np.full(9, 3.0)
    for j in (0, 4, 8):
        x = d.copy()
        x[j] = value
        dscale, rec = ref.poequ2(x)
        assert rec[3] == j + 1 and np.all(dscale == 1.0) and rec[0] == 1.0
    x = d.copy()
    x[[6, 2]] = value
    x[7] = -2.0
    assert ref.poequ2(x)[1][3] == 3


def test_dlaqsy_rule():
    assert ref.scales_by_rule(0.05, 1.0) and not ref.scales_by_rule(0.5, 1.0)
    assert ref.scales_by_rule(1.0, ref.SMALL / 2) and ref.scales_by_rule(1.0, ref.LARGE * 2) and not ref.scales_by_rule(1.0, ref.SMALL)
    assert ref.scales_by_rule(1.0, 1.0, thresh=1.5)
    assert ref.SMALL == 2.0 ** -970


@pytest.mark.parametrize("n,kappa", [(1000, 1e2), (1000, 1e6), (512, 1e2), (1, 1e2)])
def test_round_trip_on_the_graded_inputs_is_exact(n, kappa):
    A, C, D0 = ref.graded(n, kappa)
    e = ref.exponents(np.diag(A))
    As = ref.sym_scale(A, e, 1)
    d = np.diag(As)
    assert np.all((d >= 0.5) & (d < 2.0))
    assert ref.sym_scale(As, e, -1).tobytes() == A.tobytes()
    # the grading spans 16 decades, so dlaqsy's rule scales (order 1 has nothing to grade: it is scaled only when forced)
    scond = ref.poequ2(np.diag(A))[1][0]
    assert ref.scales_by_rule(scond, np.diag(A).max()) == (n > 1)
    X = np.random.default_rng(n).standard_normal((n, 5))
    assert ref.row_scale(ref.row_scale(X, e, 1), e, -1).tobytes() == X.tobytes()
