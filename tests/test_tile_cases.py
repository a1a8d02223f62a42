"""CPU: the table and the checker of tests/test_gpu_tile_kernels.py (tests/_tile_cases.py).  The checker can fail: a correct result is
accepted, and each of five alterations a wrong tile kernel could produce is rejected, on exact and on real data.  The table means
what it says: every row's product description goes through the planner (tests/gemm_plan/gemm_plan_sim, a 256-CU device, the row's
overrides) and must get the plan the row is named for -- a planner change that moves a row off its kernel shows here, without a GPU."""
import collections
import os
import subprocess

import numpy as np
import pytest

import _tile_cases as tc

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_plan")


# ---- the checker --------------------------------------------------------------------------------------------------------------------------
MUTATION_ROWS = {
    "exact": tc.make_row("ts64", 64, "mutation_exact", "syrk", dict(uplo=tc.UPPER, trans=1), 130, 130, 37, 2.0, -0.5, marks=("share",)),
    "real": tc.make_row("ts64", 64, "mutation_real", "gemmt", dict(uplo=tc.LOWER, ta=0), 130, 130, 37, 1.7, -0.6, data="real"),
}
SPLITK = 4             # the widest bound a row of this depth can get in the table is that of its split-K; 37 deep, nothing splits further


@pytest.fixture(scope="module", params=sorted(MUTATION_ROWS))
def case(request):
    row = MUTATION_ROWS[request.param]
    ops = tc.operands(row)
    ref = tc.reference(row, ops)
    return row, ops, ref, tc.expected_output(row, ops, ref)


def _with_product(row, ops, prod):
    """The flat C that alpha * prod + beta * C leaves in the wanted part (rounded once, from long double)."""
    _, _, C0, wanted = tc.logical(row, ops)
    ld = np.longdouble
    full = ld(row["alpha"]) * prod + ld(row["beta"]) * C0.astype(ld)
    out = ops["C"].copy()
    tc.view(out, ops["ldc"], row["n"])[:row["m"]][wanted] = full[wanted].astype(np.float64)
    return out


def test_the_correct_result_is_accepted(case):
    row, ops, ref, good = case
    assert tc.check(row, good, 1, ops, ref) <= (0.0 if row["data"] == "exact" else 0.05)
    assert tc.check(row, good, SPLITK, ops, ref) <= 0.05
    assert tc.check(row, good, 1) == tc.check(row, good, 1, ops, ref)          # the operands are a function of the tag


def _alterations(row, ops, good):
    opA, opB, C0, wanted = tc.logical(row, ops)
    ld = np.longdouble
    A, B = opA.astype(ld), opB.astype(ld)
    k = row["k"]
    yield "k-index K - 1 left out", _with_product(row, ops, A[:, :k - 1] @ B[:k - 1])
    yield "panel [16, 32) added twice", _with_product(row, ops, A @ B + A[:, 16:32] @ B[16:32])
    twice = ops["C"].copy()
    blk = tc.view(twice, ops["ldc"], row["n"])[:row["m"]]
    blk[wanted] = (ld(row["alpha"]) * (A @ B) + ld(row["beta"]) * (ld(row["beta"]) * C0.astype(ld)))[wanted].astype(np.float64)
    yield "beta applied twice", twice
    i, j = (5, 100) if row["flags"]["uplo"] == tc.LOWER else (100, 5)           # in the other strict triangle
    assert not wanted[i, j]
    tri = good.copy()
    tc.view(tri, ops["ldc"], row["n"])[i, j] = 1.0
    yield "one element of the unwanted triangle written", tri
    pad = good.copy()
    tc.view(pad, ops["ldc"], row["n"])[row["m"], 7] = 0.0
    yield "one padding row written", pad


def test_every_alteration_is_rejected(case):
    row, ops, ref, good = case
    seen = []
    for what, altered in _alterations(row, ops, good):
        assert not np.array_equal(altered.view(np.int64), good.view(np.int64)), what
        for splitk in (1, SPLITK):
            with pytest.raises(AssertionError, match=row["tag"]):
                tc.check(row, altered, splitk, ops, ref)
        seen.append(what)
    assert len(seen) == 5


def test_nan_in_the_wanted_part_is_rejected(case):
    row, ops, ref, good = case
    bad = good.copy()
    tc.view(bad, ops["ldc"], row["n"])[64, 64] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        tc.check(row, bad, 1, ops, ref)


def test_operands_hold_nan_where_nothing_may_be_read():
    for row in tc.ROWS:
        if row["k"] > 600 or row["m"] > 400:
            continue
        ops = tc.operands(row)
        sa, sb, (m, n) = tc.stored_shapes(row)
        A = tc.view(ops["A"], ops["lda"], sa[1], row["offA"])
        assert np.isnan(A[sa[0]:]).all() and np.isnan(ops["A"][:row["offA"]]).all(), row["tag"]
        if sb:
            B = tc.view(ops["B"], ops["ldb"], sb[1], row["offB"])
            assert np.isnan(B[sb[0]:]).all() and np.isnan(ops["B"][:row["offB"]]).all() and np.isfinite(B[:sb[0]]).all() != (row["alpha"] == 0), row["tag"]
        C = tc.view(ops["C"], ops["ldc"], n)
        assert ops["ldc"] == m + 3 and np.isfinite(C[m:]).all() and np.isnan(C[:m]).all() == (row["beta"] == 0.0), row["tag"]
        if row["fn"] == "trmm_oop":
            f = row["flags"]
            dead = np.triu(np.ones(sa, dtype=bool), 1) if f["uplo"] == tc.LOWER else np.tril(np.ones(sa, dtype=bool), -1)
            assert np.isnan(A[:sa[0]][dead]).all() and np.isnan(np.diag(A[:sa[0]])).all() == bool(f["diag"]), row["tag"]
        elif row["alpha"] != 0:
            assert np.isfinite(A[:sa[0]]).all(), row["tag"]
        if row["data"] == "exact":
            for x in (A[:sa[0]], C[m:]):
                x = x[np.isfinite(x)]
                assert (x == np.round(x)).all() and (np.abs(x) <= 4).all(), row["tag"]


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planned():
    """[(row, plan line as a dict of strings)] for every row of the table, on a 256-CU device."""
    subprocess.check_call(["make", "-C", HERE, "-s"])
    lines = [" ".join(f"{k}={v}" for k, v in dict(tc.product_of(r), num_cu=256).items()) for r in tc.ROWS]
    res = subprocess.run([os.path.join(HERE, "gemm_plan_sim")], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 0, res.stdout + res.stderr
    out = []
    for line in res.stdout.splitlines():
        prod, plan = line.split(" -> ")
        out.append({k: v for k, v in (t.split("=", 1) for t in (prod + " " + plan).split())})
    assert len(out) == len(tc.ROWS)
    return list(zip(tc.ROWS, out))


def test_every_row_gets_the_plan_it_is_named_for(planned):
    bad = [f"{r['tag']}: " + "; ".join(tc.plan_errors(r, p)) for r, p in planned if tc.plan_errors(r, p)]
    assert not bad, "\n".join(bad)


def test_without_the_overrides_the_forced_rows_leave_the_tile_kernel_or_its_size(planned):
    """Why the groups need their environment: unforced, nearly every forced row plans onto another kernel or the other tile size."""
    forced = [r for r in tc.ROWS if r["env"] != "free" and "scale" not in r["marks"]]
    lines = [" ".join(f"{k}={v}" for k, v in dict(tc.product_of(r), num_cu=256, force_small=-1, force_ts=0).items()) for r in forced]
    res = subprocess.run([os.path.join(HERE, "gemm_plan_sim")], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 0, res.stdout + res.stderr
    same = sum(f" path=tile ts={r['ts']} " in line for r, line in zip(forced, res.stdout.splitlines()))
    assert same <= len(forced) // 4, (same, len(forced))


def test_every_instantiation_has_its_rows(planned):
    """Each of the eight dgemm_tile_kernel<TS, AK, BKC> is named by plain-product rows with every edge ragged, with all tiles interior
    (FAST loop only, and FAST loop plus a generic tail) and split along k; every (beta == 0, 1, other) epilogue sees each of them."""
    kinds, betas = collections.defaultdict(set), collections.defaultdict(set)
    for r, p in planned:
        if r["fn"] != "gemm" or p["path"] != "tile" or r["env"] == "free":
            continue
        key = (int(p["ts"]), int(p["ak"]), int(p["bkc"]))
        if int(p["splitk"]) > 1:
            kinds[key].add("splitk")
            continue
        betas[key].add(r["beta"] if r["beta"] in (0.0, 1.0) else "other")
        if tc.ragged(r):
            kinds[key].add("ragged")
        if tc.all_interior(r):
            kinds[key].add("interior, K % 16 == 0" if r["k"] % 16 == 0 else ("interior, K < 16" if r["k"] < 16 else "interior, K tail"))
    assert len(kinds) == 8
    for key in kinds:
        assert kinds[key] >= {"splitk", "ragged", "interior, K % 16 == 0", "interior, K tail", "interior, K < 16"}, (key, kinds[key])
        assert betas[key] == {0.0, 1.0, "other"}, (key, betas[key])


def test_real_rows_stay_cheap():
    real = [r for r in tc.ROWS if r["data"] == "real"]
    big = [r["tag"] for r in real if float(r["m"]) * r["n"] * r["k"] > tc.REAL_LIMIT]
    assert big == ["ts128_gemm_tn_256x256x8192_splitk_real"]         # the 128-tile's smallest split-K shape
    assert {r["env"] for r in real} == {"ts64", "ts128"} and all(r["fn"] == "gemm" for r in real)


def test_group_sizes():
    assert {e: len(tc.rows_of(e)) for e in tc.ENVS} == {"ts64": 147, "ts128": 151, "free": 12}
