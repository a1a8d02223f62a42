"""CPU: the work partition of capi_dresid_sym (capital_amd/csrc/sym_thin_plan.h -- the upper triangle cut into a p x p block triangle, one
workgroup per block, two slots of partial sums per block, p + 1 contributions per line block) run through
tests/sym_thin_plan/sym_thin_plan_sim.cpp, built with ASan + UBSan."""
import os
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sym_thin_plan")
SIZES = [1, 2, 31, 32, 33, 255, 256, 257, 300, 704, 705, 2000, 2100, 4096, 5632, 5633, 6000, 32768, 65536, 70001]
CUS = [1, 2, 3, 7, 32, 64, 255, 256, 304]


@pytest.fixture(scope="module")
def sim():
    subprocess.check_call(["make", "-C", HERE, "-s"])
    return os.path.join(HERE, "sym_thin_plan_sim")


def run(sim, lines):
    res = subprocess.run([sim], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 0, res.stdout + res.stderr
    return [{k: int(v) for k, v in (t.split("=") for t in line.split())} for line in res.stdout.splitlines()]


@pytest.fixture(scope="module")
def plans(sim):
    cases = [(n, cus) for n in SIZES for cus in CUS]
    out = run(sim, [f"plan {n} {cus}" for n, cus in cases])
    assert len(out) == len(cases)
    return list(zip(cases, out))


def test_every_element_belongs_to_one_block(plans):
    for (n, cus), d in plans:
        assert d["bad"] == 0 and d["miss"] == 0, (n, cus, d)
        assert d["elems"] == n * (n + 1) // 2, (n, cus, d)            # the blocks' sizes add up to the triangle ..
        assert d["marked"] == (n * n <= 4000000)                       # .. and, where the matrix is small, element by element
        assert d["blocks"] == d["p"] * (d["p"] + 1) // 2


def test_balance_rule(plans):
    for (n, cus), d in plans:
        q = d["q"]
        assert q * (q + 1) // 2 <= cus < (q + 1) * (q + 2) // 2, (n, cus, d)
        assert 1 <= d["p"] <= q and d["blocks"] <= cus, (n, cus, d)   # one workgroup per block, all of them resident
        assert d["bs"] % 32 == 0 and d["bs"] >= 32 and (d["p"] - 1) * d["bs"] < n <= d["p"] * d["bs"], (n, cus, d)
        assert d["bs"] * q < n + 32 * q, (n, cus, d)                  # bs < n / q + 32
        assert d["max_block"] <= d["bs"] ** 2, (n, cus, d)


def test_slots_written_are_the_slots_read(plans):
    for (n, cus), d in plans:
        p = d["p"]
        assert d["written"] == p * (p + 1) == d["read"], (n, cus, d)  # two per block; p + 1 per line block
        assert d["stray"] == 0 and d["unread"] == 0, (n, cus, d)


def test_the_flagship_plan(plans):
    d = dict(plans)[(32768, 256)]
    assert (d["p"], d["bs"], d["blocks"]) == (22, 1504, 253)
