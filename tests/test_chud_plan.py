"""CPU: the launch schedule of capi_dchud / capi_dchud_inv (capital_amd/csrc/chud_plan.h -- panels of B steps, apply workgroups of COLS trailing columns,
row groups of the inverse) walked by tests/chud_plan/chud_plan_sim.cpp, built with ASan + UBSan."""
import os
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "chud_plan")


@pytest.fixture(scope="module")
def sim():
    subprocess.check_call(["make", "-C", HERE, "-s"])
    return os.path.join(HERE, "chud_plan_sim")


def run(sim, lines):
    res = subprocess.run([sim], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 0, res.stdout + res.stderr
    return [{k: int(v) for k, v in (t.split("=") for t in line.split())} for line in res.stdout.splitlines()]


@pytest.fixture(scope="module")
def consts(sim):
    return run(sim, ["consts"])[0]


def test_constants(consts):
    assert consts["b"] in (32, 64) and consts["b"] * consts["cols"] == 4096 and consts["rows"] % consts["kchunk"] == 0


def test_every_step_in_one_panel_and_every_trailing_column_in_one_apply(sim, consts):
    b, cols = consts["b"], consts["cols"]
    sizes = [1, 2, b - 1, b, b + 1, 1000, 70001]
    out = run(sim, [f"plan {n}" for n in sizes])
    assert len(out) == len(sizes)
    for n, d in zip(sizes, out):
        panels = -(-n // b)
        assert d["step_miss"] == 0 and d["col_miss"] == 0 and d["bad"] == 0, (n, d)
        assert d["panels"] == panels and d["launches"] == 2 * panels - 1, (n, d)
        assert d["applies"] == sum(-(-(n - min(n, (p + 1) * b)) // cols) for p in range(panels)), (n, d)


def test_rows_of_the_inverse(sim, consts):
    ranges = [(0, 1), (0, 2), (0, 63), (0, 64), (0, 65), (0, 1000), (16, 33), (500, 1000), (37, 70001), (5, 5)]
    out = run(sim, [f"inv {a} {b}" for a, b in ranges])
    for (a, b), d in zip(ranges, out):
        assert d["row_miss"] == 0 and d["bad"] == 0 and d["groups"] == -(-(b - a) // consts["rows"]), (a, b, d)
