"""CPU: the launch schedule of capi_dormqr's thin path (capital_amd/csrc/ormqr_plan.h -- panels of 32 reflectors in either direction, row slices of the
Gram pass, slabs, workspace) walked by tests/ormqr_plan/ormqr_plan_sim.cpp, a stand-alone program built with ASan + UBSan."""
import os
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ormqr_plan")
SHAPES = [(1, 1), (32, 32), (33, 1), (97, 33), (64, 64), (4096, 256), (70001, 130)]
CUS = (256, 7, 1)


@pytest.fixture(scope="module")
def sim():
    subprocess.check_call(["make", "-C", HERE, "-s"])
    return os.path.join(HERE, "ormqr_plan_sim")


def run(sim, lines):
    res = subprocess.run([sim], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 0, res.stdout + res.stderr
    return [{k: int(v) for k, v in (t.split("=") for t in line.split())} for line in res.stdout.splitlines()]


def test_constants(sim):
    c = run(sim, ["consts"])[0]
    assert c["nb"] == 32 and c["tile"] == 32 and c["round"] == c["tile"] * c["waves"]


@pytest.mark.parametrize("trans", [1, 0])
def test_panels_slices_and_workspace(sim, trans):
    cases = [(m, k, cus, rb) for m, k in SHAPES for cus in CUS for rb in (1, 2)]
    out = run(sim, [f"plan {m} {k} {trans} {cus} {rb}" for m, k, cus, rb in cases])
    assert len(out) == len(cases)
    for (m, k, cus, rb), d in zip(cases, out):
        what = (m, k, trans, cus, rb, d)
        assert d["panels"] == -(-k // 32) and d["launches"] == 3 * d["panels"], what
        assert d["refl_miss"] == 0, what                     # every reflector in exactly one panel
        assert d["order_bad"] == 0, what                     # ascending for Q^T, descending for Q
        assert d["row_miss"] == 0, what                      # every live row of every panel in exactly one slice
        assert d["empty"] == 0, what
        assert 1 <= d["slabs"] <= cus, what
        assert d["slabs"] == min(cus, -(-m // 256)), what    # the panel at j0 = 0 has the most rounds
        assert d["touched"] <= d["ws"], what                 # the workspace covers what the walk touches
        assert d["ws"] == 1024 + d["slabs"] * (768 + 512 * rb), what
