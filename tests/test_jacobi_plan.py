"""CPU: the pair schedule of capi_dgesvj (capital_amd/csrc/jacobi_plan.h -- round-robin steps of disjoint column pairs) walked by
tests/jacobi_plan/jacobi_plan_sim.cpp, built with ASan + UBSan; and tests/_jacobi_ref.py, the numpy restatement of the kernels, follows the
same schedule."""
import os
import subprocess

import numpy as np
import pytest

import _jacobi_ref as jr

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jacobi_plan")
SIZES = list(range(1, 71)) + [257, 1024, 2047, 2048]


@pytest.fixture(scope="module")
def sim():
    subprocess.check_call(["make", "-C", HERE, "-s"])
    return os.path.join(HERE, "jacobi_plan_sim")


def run(sim, lines):
    res = subprocess.run([sim], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 0, res.stdout + res.stderr
    return [{k: int(v) for k, v in (t.split("=") for t in line.split())} for line in res.stdout.splitlines()]


def test_limits(sim):
    assert run(sim, ["limits"])[0] == {"max_n": 2048, "max_sweeps": jr.MAX_SWEEPS}


def test_every_pair_once_in_disjoint_steps(sim):
    out = run(sim, [f"plan {n}" for n in SIZES])
    assert len(out) == len(SIZES)
    for n, d in zip(SIZES, out):
        N = n + (n & 1)
        assert d["steps"] == (N - 1 if n > 1 else 0) and d["slots"] == (N // 2 if n > 1 else 0), (n, d)
        # every step's pairs are disjoint with p < q < n; every unordered pair exactly once; an odd n rests exactly one column per step
        assert d["bad"] == 0 and d["miss"] == 0 and d["rest_bad"] == 0, (n, d)
        assert d["pairs"] == n * (n - 1) // 2, (n, d)


def test_order_one_has_no_pairs(sim):
    assert run(sim, ["plan 1"])[0] == {"steps": 0, "slots": 0, "pairs": 0, "bad": 0, "miss": 0, "rest_bad": 0}


def test_out_of_range_is_refused(sim):
    res = subprocess.run([sim], input="plan 2049\n", capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 2


@pytest.mark.parametrize("n", [2, 7, 8, 33])
def test_numpy_restatement_follows_the_schedule(n):
    seen = np.zeros((n, n), dtype=int)
    for step in range(n + (n & 1) - 1):
        p, q = jr.step_pairs(n, step)
        assert np.all(p < q) and np.all(q < n) and len(set(p) | set(q)) == 2 * len(p) == n - (n & 1)
        seen[p, q] += 1
    assert np.array_equal(seen, np.triu(np.ones((n, n), dtype=int), 1))
