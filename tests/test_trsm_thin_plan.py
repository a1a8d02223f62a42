"""CPU: the step list of capi_dtrsm_thin (capital_amd/csrc/trsm_thin_plan.h -- leaves of order <= LEAF and rectangular products, in execution order)
walked by tests/trsm_thin_plan/trsm_thin_plan_sim.cpp, built with ASan + UBSan."""
import os
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "trsm_thin_plan")


@pytest.fixture(scope="module")
def sim():
    subprocess.check_call(["make", "-C", HERE, "-s"])
    return os.path.join(HERE, "trsm_thin_plan_sim")


def run(sim, lines):
    res = subprocess.run([sim], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 0, res.stdout + res.stderr
    return [{k: int(v) for k, v in (t.split("=") for t in line.split())} for line in res.stdout.splitlines()]


@pytest.fixture(scope="module")
def leaf(sim):
    return run(sim, ["leaf"])[0]["leaf"]


def test_leaf_is_a_candidate(leaf):
    assert leaf in (256, 512, 1024)


@pytest.mark.parametrize("trans", [0, 1])
def test_steps_cover_once_in_a_valid_order(sim, leaf, trans):
    sizes = [1, 2, 33, leaf - 1, leaf, leaf + 1, 2100, 4097, 65536, 70001]
    out = run(sim, [f"plan {trans} {n}" for n in sizes])
    assert len(out) == len(sizes)
    for n, d in zip(sizes, out):
        nl = -(-n // leaf)
        # every element of the triangle in exactly one leaf or one product: by sums, and element by element where the triangle is small
        assert d["elems"] == d["total"] == n * (n + 1) // 2, (n, d)
        assert d["marked"] == (n * n <= 4000000) and d["miss"] == 0, (n, d)
        # leaves of order <= LEAF; a product reads only finished rows; a leaf's rows have received all their products; every row solved once
        assert d["bad"] == 0 and 1 <= d["max_leaf"] <= leaf, (n, d)
        assert d["leaves"] == nl and d["products"] == nl - 1 and d["steps"] == 2 * nl - 1, (n, d)
        assert d["depth"] == (nl - 1).bit_length(), (n, d)


@pytest.mark.parametrize("trans", [0, 1])
def test_order_2100_recurses_at_least_twice(sim, trans):
    d = run(sim, [f"plan {trans} 2100"])[0]
    assert d["depth"] >= 2 and d["products"] >= 3, d
