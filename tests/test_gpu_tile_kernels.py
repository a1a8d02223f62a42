"""GPU parity of dgemm_tile_kernel<TS, AK, BKC> (capital_amd/csrc/gemm_f64.hip) where its loop structure can go wrong: both tile sizes,
all four operand orientations, ragged edges in m, n and k, K < 16, a FAST loop followed by one generic tail panel, one operand off the
16-byte loads, interior and edge tiles in one launch, split-K with rotation (whole and ragged last slices, a wrap that lands on a
partial panel), triangular outputs (shared diagonal panels, dead sub-tiles, banded tile order, split-K on a triangle) and TRMMs whose
launch holds interior and edge tiles.  The planner sends none of these shapes to the tile kernel by itself, so each group of rows runs
in a child process (tests/_gpu_tile_main.py) whose environment pins the plan -- CAPI_SMALL=0 CAPI_FORCE_TS=64 | 128, or nothing for
the rows a 256-CU device plans onto the tile kernel anyway -- and whose CAPI_DEBUG_GEMM lines prove which kernel ran: a row that ran
on another kernel fails.  Table, operands, reference and checker: tests/_tile_cases.py (exact integer data compared bit for bit; real
data against np.longdouble within a derived componentwise bound)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _tile_cases as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ABNORMAL = []          # a child that ended with a signal, a time-out or an error: nothing more is started on the GPU from here


def _last_row(stderr):
    rows = re.findall(r"^row (\S+)$", stderr or "", re.M)
    return rows[-1] if rows else "(before the first row)"


def _run_group(env, tmp_path):
    """Runs the group's child once; returns (num_cu, {tag: [plan lines as dicts]}, {tag: flat C})."""
    if _ABNORMAL:
        pytest.fail(f"not started: the child of group {_ABNORMAL[0]} ended abnormally")
    rows = tc.rows_of(env)
    rows_json, out_npz = str(tmp_path / "rows.json"), str(tmp_path / "out.npz")
    with open(rows_json, "w") as f:
        json.dump(rows, f)
    child_env = {k: v for k, v in os.environ.items() if k not in ("CAPI_SMALL", "CAPI_FORCE_TS")}
    child_env.update(tc.ENVS[env], CAPI_DEBUG_GEMM="1")
    try:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_gpu_tile_main.py"), rows_json, out_npz],
                             env=child_env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        _ABNORMAL.append(env)
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else e.stderr
        pytest.fail(f"{env}: the child did not finish in 300 s; the last row it announced: {_last_row(err)}")
    if res.returncode != 0 or "cases done" not in res.stdout:
        _ABNORMAL.append(env)
        pytest.fail(f"{env}: the child ended with status {res.returncode}; the last row it announced: {_last_row(res.stderr)}\n"
                    + "\n".join(l for l in res.stderr.splitlines() if not l.startswith(("row ", "[capi gemm]")))[-3000:])
    cus = int(re.search(r"^num_cu (\d+)$", res.stderr, re.M).group(1))
    plans, cur = {}, None
    for line in res.stderr.splitlines():
        if line.startswith("row "):
            cur = plans.setdefault(line[4:].strip(), [])
        elif line.startswith("[capi gemm]") and cur is not None:
            prod, plan = line[len("[capi gemm] "):].split(" -> ")
            cur.append({k: v for k, v in (t.split("=", 1) for t in (prod + " " + plan).split())})
    with np.load(out_npz) as z:
        got = {k: z[k] for k in z.files}
    os.unlink(out_npz)
    assert set(plans) == set(got) == {r["tag"] for r in rows}
    return cus, plans, got


def _check_group(env, tmp_path):
    cus, plans, got = _run_group(env, tmp_path)
    if env == "free" and cus != 256:
        pytest.skip(f"the unforced rows are planned onto the tile kernel by a 256-CU device; this one has {cus}")
    failures, worst, kernels = [], (0.0, None), {}
    for r in tc.rows_of(env):
        tag = r["tag"]
        if len(plans[tag]) != 1:
            failures.append(f"{tag}: {len(plans[tag])} products, expected one")
            continue
        p = plans[tag][0]
        bad = tc.plan_errors(r, p)
        if bad:
            failures.append(f"{tag}: not the intended plan: " + "; ".join(bad))
            continue
        try:
            ratio = tc.check(r, got[tag], int(p["splitk"]))
        except AssertionError as e:
            failures.append(str(e))
            continue
        if r["data"] == "real":
            print(f"[tile] {tag}: splitk {p['splitk']} worst err / bound {ratio:.3e}")
            worst = max(worst, (ratio, tag))
        if r["fn"] == "gemm" and p["path"] == "tile":
            kinds = kernels.setdefault((int(p["ts"]), int(p["ak"]), int(p["bkc"])), set())
            kinds.update(x for x, on in (("ragged", tc.ragged(r)), ("interior", tc.all_interior(r) and int(p["splitk"]) == 1),
                                         ("splitk", int(p["splitk"]) > 1)) if on)
    print(f"[tile] {env}: {len(plans)} rows, {len(failures)} failed; worst err / bound of the real rows {worst[0]:.3e} ({worst[1]})")
    for k in sorted(kernels):
        print(f"[tile] dgemm_tile_kernel<{k[0]}, {bool(k[1])}, {bool(k[2])}>: passing plain rows that are " + ", ".join(sorted(kernels[k])))
    assert not failures, f"{len(failures)} of {len(plans)} rows failed:\n" + "\n".join(failures)
    return kernels


@pytest.mark.parametrize("env,ts", [("ts64", 64), ("ts128", 128)])
def test_forced_tile_size(env, ts, tmp_path):
    """Every row of the group on the forced tile size: the plan, then the numbers.  Each of the four instantiations of the size is named
    by a passing plain-product row with every edge ragged, by one whose tiles are all interior and by one split along k."""
    kernels = _check_group(env, tmp_path)
    for ak in (0, 1):
        for bkc in (0, 1):
            assert kernels.get((ts, ak, bkc), set()) >= {"ragged", "interior", "splitk"}, (ts, ak, bkc, kernels.get((ts, ak, bkc)))


def test_unforced_split_k(tmp_path):
    """Products that a 256-CU device plans onto the tile kernel with split-K by itself, in all four orientations."""
    kernels = _check_group("free", tmp_path)
    assert all("splitk" in kernels.get((64, ak, bkc), set()) for ak in (0, 1) for bkc in (0, 1)), kernels
