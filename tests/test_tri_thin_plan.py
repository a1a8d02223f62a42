"""CPU: the work partition of capi_dtrmm_thin (capital_amd/csrc/tri_thin_plan.h -- tiles of 256 output lines x 32 contraction indices dealt to
workgroup slices by equal bytes, the packed column start, the per-column alignment class) run through tests/tri_thin_plan/tri_thin_plan_sim.cpp,
built with ASan + UBSan."""
import os
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tri_thin_plan")
RECT, UPPERTRI = 0, 1
SIZES = [1, 2, 17, 300, 4096, 65536, 70001]


@pytest.fixture(scope="module")
def sim():
    subprocess.check_call(["make", "-C", HERE, "-s"])
    return os.path.join(HERE, "tri_thin_plan_sim")


def run(sim, lines):
    res = subprocess.run([sim], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 0, res.stdout + res.stderr
    return res.stdout.splitlines()


def parse(line):
    return {k: int(v) for k, v in (t.split("=") for t in line.split())}


def check(d, total, slices):
    assert d["bad"] == 0 and d["walked"] == d["tiles"] and d["end_group"] == d["groups"], d
    assert d["elems"] == d["total"] == total, d                     # every element in exactly one tile of exactly one slice ..
    assert d["miss"] == 0, d                                        # .. counted element by element where the block is small
    assert 1 <= d["S"] <= slices and d["max_tile"] <= d["tile_cap"], d
    # the header's rule: no slice exceeds the mean share by more than one tile's worth (256 x 32 elements)
    assert d["max_slice"] * d["S"] <= total + d["tile_cap"] * d["S"], d


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("slices", [256, 7])
def test_triangle_slices_cover_once_and_balance(sim, trans, slices):
    out = run(sim, [f"plan {UPPERTRI} {trans} {n} {n} {slices}" for n in SIZES])
    assert len(out) == len(SIZES)
    for n, line in zip(SIZES, out):
        d = parse(line)
        check(d, n * (n + 1) // 2, slices)
        assert d["marked"] == (n * n <= 4000000)


@pytest.mark.parametrize("trans", [0, 1])
def test_rectangle_slices_cover_once_and_balance(sim, trans):
    shapes = [(n, n) for n in SIZES] + [(5, 300), (300, 5), (1000, 129), (16, 64), (65536, 17), (17, 70001), (32768, 32768)]
    out = run(sim, [f"plan {RECT} {trans} {m} {n} 256" for m, n in shapes])
    for (m, n), line in zip(shapes, out):
        check(parse(line), m * n, 256)


@pytest.mark.parametrize("col0", [0, 1, 65535])
def test_packed_column_start_and_alignment_class(sim, col0):
    """x (x + 1) / 2 in Python integers, beyond 2^32 from column 92682 on; the class is the start's parity; a view's column offsets are relative
    to its first column"""
    starts = sorted({col0 + k for k in range(70)} | {col0 + n - 1 for n in SIZES} | {92681, 92682, 2 ** 31 - 1, 2 ** 31})
    seen = 0
    for x0 in starts:
        for line in run(sim, [f"cols {x0} 3"]):
            t = line.split()
            x = int(t[1])
            d = {k: int(v) for k, v in (u.split("=") for u in t[2:])}
            ref = x * (x + 1) // 2
            assert d["start"] == ref and d["class"] == ref % 2 and d["offset"] == ref - x0 * (x0 + 1) // 2, (x, d)
            seen += ref > 2 ** 32
    assert seen > 0
