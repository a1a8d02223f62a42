"""CPU: launch_gemm's planner (capital_amd/csrc/gemm_plan.h -- which kernel, tile size and split-K a product gets and how its launches
are cut) run through tests/gemm_plan/gemm_plan_sim.cpp, built with ASan + UBSan.  The rules the dispatcher is meant to follow, on a
256-CU device unless a case says otherwise, and the exact plans of the products the n = 32768 cholinv step issues on one GPU."""
import math
import os
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_plan")
LEFT, RIGHT, UPPER = 0, 1, 1


@pytest.fixture(scope="module")
def sim():
    subprocess.check_call(["make", "-C", HERE, "-s"])
    return os.path.join(HERE, "gemm_plan_sim")


def _num(v):
    for conv in (int, float):
        try:
            return conv(v)
        except ValueError:
            pass
    return v


def plans(sim, cases):
    """One plan per case: a dict of gemm_plan::Product / Device / Modes / Overrides fields (omitted fields keep their defaults)."""
    lines = [" ".join(f"{k}={int(v) if isinstance(v, bool) else v}" for k, v in c.items()) for c in cases]
    res = subprocess.run([sim], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 0, res.stdout + res.stderr
    out = []
    for line in res.stdout.splitlines():
        d = {k: _num(v) for k, v in (t.split("=", 1) for t in line.split(" -> ")[1].split())}
        d["shares"] = [float(s) for s in str(d.get("shares", "")).split(",") if s]
        out.append(d)
    assert len(out) == len(cases)
    return out


def plan(sim, **case):
    return plans(sim, [case])[0]


def gram(n, k, **kw):               # C = A^T A, upper triangle, A k-contiguous (CholeskyQR2's Gram matrix)
    return dict(M=n, N=n, K=k, out_uplo=UPPER, ak=1, bkc=1, a_is_b=1, same_ld=1, a_vec=1, b_vec=1) | kw


def right_trmm(m, n=256, **kw):     # C = B T, T n x n upper triangular (Q = A R^-1)
    return dict(M=m, N=n, K=n, tri_side=RIGHT, tri_eff_upper=1, bkc=1, a_vec=1, b_vec=1) | kw


def left_trmm(order, n=4096, **kw):  # C = op(T) B, T order x order
    return dict(M=order, N=n, K=order, tri_side=LEFT, tri_eff_upper=1, bkc=1, a_vec=1, b_vec=1) | kw


@pytest.mark.parametrize("m", [64 * 256, 64 * 256 + 32, 100000, 1 << 21, 1 << 23])
@pytest.mark.parametrize("cus", [256, 80])
def test_tall_right_trmm_takes_the_32_row_ts_kernel(sim, m, cus):
    r = plan(sim, **right_trmm(m), num_cu=cus)
    assert r["path"] == "trmm_ts32" and r["launches"] == 1
    assert r["blocks"] == min(math.ceil(m / 32), cus)
    assert plan(sim, **right_trmm(64 * 256 - 32))["path"] != "trmm_ts32"


@pytest.mark.parametrize("n,k,cus", [(256, 1 << 22, 256), (256, 1 << 14, 256), (128, 1 << 13, 256), (64, 4096, 256), (64, 4096, 4),
                                     (256, 1 << 20, 1), (192, 1 << 16, 48)])
def test_full_width_gram(sim, n, k, cus):
    r = plan(sim, **gram(n, k), num_cu=cus)
    S = min(max(math.ceil(k / 16) // 32, 1), cus)
    assert r["path"] == "gram_ts" and r["blocks"] == S and r["splitk"] == S and r["slab_stride"] == n * n
    assert r["reduce"] == ("wide" if S >= 16 else "narrow" if S > 1 else "none")


def test_wide_gram_goes_by_256_blocks(sim):
    r = plan(sim, **gram(1024, 1 << 23))
    assert r["path"] == "gram_blocks" and r["tiles_n"] == 4 and r["ntiles"] == 10
    assert plan(sim, **gram(768, 1 << 23))["path"] == "gram_blocks"
    assert plan(sim, **gram(2304, 1 << 23))["path"] == "tile"
    # the loop's block products: an off-diagonal 256 x 256 block on the tile kernel, a diagonal one on the full-width kernel
    assert plan(sim, **dict(gram(256, 1 << 23), out_uplo=-1, a_is_b=0))["path"] == "tile"
    assert plan(sim, **gram(256, 1 << 23))["path"] == "gram_ts"


def test_small_kernel_up_to_order_512(sim):
    cases = []
    for m in (1, 31, 32, 100, 256, 500, 512):
        for n in (1, 33, 128, 512):
            for k in (1, 64, 500, 2048):
                cases += [dict(M=m, N=n, K=k, a_vec=1, b_vec=1), dict(M=m, N=n, K=k, ak=1, bkc=1, beta=1.0),
                          dict(M=m, N=m, K=k, out_uplo=UPPER, ak=1, bkc=1, a_is_b=1, same_ld=1),
                          dict(M=m, N=n, K=m, tri_side=LEFT, tri_eff_upper=1, bkc=1, batch=4)]
    assert all(r["path"] == "small" for r in plans(sim, cases))
    assert plan(sim, M=513, N=512, K=2048)["path"] != "small" and plan(sim, M=512, N=512, K=2049)["path"] != "small"


@pytest.mark.parametrize("k", [16, 128, 256])
@pytest.mark.parametrize("cus", [256, 64])
def test_thin_products_take_the_small_kernel_when_three_rounds_of_slots_hold_them(sim, k, cus):
    cases = [dict(M=m, N=n, K=k, ak=1, bkc=1, num_cu=cus) for m in (128, 256, 640) for n in range(128, 16384, 384)]
    cases += [dict(M=n, N=n, K=k, out_uplo=UPPER, ak=1, bkc=1, a_is_b=1, same_ld=1, num_cu=cus) for n in range(512, 4096, 128)]
    slots = cus * (2 if k <= 128 else 1)
    for c, r in zip(cases, plans(sim, cases)):
        nt32 = math.ceil(c["M"] / 32) * math.ceil(c["N"] / 32) * (0.5 if c.get("out_uplo", -1) >= 0 else 1.0)
        small = (c["M"] <= 512 and c["N"] <= 512) or nt32 <= 3 * slots
        assert (r["path"] == "small") == small, (c, r)


def test_forced_small_overrides_both_rules(sim):
    assert plan(sim, M=4096, N=4096, K=8192, force_small=1)["path"] == "small"
    assert plan(sim, M=4097, N=4096, K=64, force_small=1)["path"] != "small"
    assert plan(sim, M=128, N=128, K=128, force_small=0)["path"] == "tile"
    assert plan(sim, M=128, N=4096, K=128, ak=1, bkc=1, force_small=0)["path"] == "tile"


@pytest.mark.parametrize("order", [4096, 8192])
@pytest.mark.parametrize("ak", [0, 1])
def test_trmm_pairs_are_whole_resident_rounds(sim, order, ak):
    r = plan(sim, **left_trmm(order, ak=ak))
    assert r["path"] == "pair" and r["ts"] == 128 and r["variant"] == 16 + 2 * ak + 1
    assert r["blocks"] == (order // 256) * (4096 // 128) and r["blocks"] % 512 == 0 and r["launches"] == 1
    r = plan(sim, **left_trmm(order, ak=ak), pair_mode=2, pair_rounds=1)       # capi_set_launch_rounds(1): one launch per round
    assert r["path"] == "pair" and r["per_launch"] == 512 and r["launches"] == r["blocks"] // 512


@pytest.mark.parametrize("case", [left_trmm(6144), left_trmm(4096, n=3072), left_trmm(4096, beta=1.0), left_trmm(4096, b_vec=0),
                                  left_trmm(4096, tri_dense=1), left_trmm(4096, pair_mode=0)])
def test_no_trmm_pairs_off_whole_rounds_or_their_preconditions(sim, case):
    assert plan(sim, **case)["path"] == "tile"


def test_tail_of_64_tiles(sim):
    cases = [dict(M=128 * a, N=128 * b, K=8192, a_vec=1, b_vec=1) for a in range(8, 96, 3) for b in (8, 16, 32, 40)]
    cases += [dict(M=128 * a, N=128 * a, K=8192, out_uplo=UPPER, ak=1, bkc=1, a_is_b=1, same_ld=1) for a in range(30, 130, 7)]
    cases += [dict(c, stream_cu=192) for c in cases[:40]]
    seen = set()
    for c, r in zip(cases, plans(sim, cases)):
        per_round = 2 * c.get("stream_cu", 256)
        ntiles_all = r["ntiles"] + r["tail128"]
        rem = ntiles_all % per_round
        want = rem if r["ts"] == 128 and r["splitk"] == 1 and ntiles_all >= 2 * per_round and 0 < rem <= 3 * per_round // 4 else 0
        assert r["tail128"] == want, (c, r)
        seen.add(want > 0)
    assert seen == {True, False}


def test_resident_rounds(sim):
    cube = dict(M=16384, N=16384, K=16384, a_vec=1, b_vec=1)
    r = plan(sim, **cube, rounds_mode=1)
    assert r["ntiles"] == 16384 and r["per_launch"] == 512 and r["launches"] == 32 and r["tail128"] == 0
    assert plan(sim, **cube)["launches"] == 1
    r = plan(sim, **cube, rounds_mode=1, stream_cu=192)
    assert r["per_launch"] == 384 and r["launches"] == math.ceil(r["ntiles"] / 384)
    assert r["tail128"] == 16384 % 384 and r["ntiles"] == 16384 - r["tail128"]
    # triangular outputs only with bit 1 (in the banded order)
    assert plan(sim, **gram(16384, 16384), rounds_mode=1)["launches"] == 1
    r = plan(sim, **gram(16384, 16384), rounds_mode=2)
    assert r["order"] == 1 and r["per_launch"] == 512 and r["launches"] == math.ceil(r["ntiles"] / 512)


def test_split_k(sim):
    cases = [dict(M=m, N=n, K=k, out_uplo=up, ak=1, bkc=1, a_vec=1, b_vec=1) for m in (64, 128, 256, 512, 1024, 2048) for n in (64, 256, 1024)
             for k in (256, 1000, 4096, 10000, 65536, 1 << 20) for up in (-1, UPPER) if up < 0 or m == n]
    on, off = plans(sim, cases), plans(sim, [dict(c, ws_for_slab=0) for c in cases])
    assert sum(r["splitk"] > 1 for r in on) > len(cases) // 2
    assert all(r["splitk"] == 1 for r in off)
    for c, r in zip(cases, on):
        if r["splitk"] > 1:
            # every slice is k_per_split >= 256 deep (a multiple of the 16-deep panel) but the last, which takes what remains
            assert r["k_per_split"] >= 256 and c["K"] // r["splitk"] >= 256 and r["k_per_split"] % 16 == 0
            assert (r["splitk"] - 1) * r["k_per_split"] < c["K"] <= r["splitk"] * r["k_per_split"]
            assert r["slab_stride"] == c["M"] * c["N"] and r["reduce"] == "narrow" and r["tail128"] == 0


def test_recorded_flop_shares(sim):
    whole = [plan(sim, M=16384, N=16384, K=16384, a_vec=1, b_vec=1, rounds_mode=1),
             plan(sim, **left_trmm(8192, n=8192), pair_mode=2, pair_rounds=1), plan(sim, **left_trmm(4096)),
             plan(sim, M=1000, N=1000, K=1 << 20, a_vec=1, b_vec=1), plan(sim, M=2048, N=2048, K=2048)]
    assert whole[0]["launches"] == 32 and whole[1]["launches"] == 4 and whole[3]["splitk"] > 1
    for r in whole:
        assert len(r["shares"]) == r["launches"] and sum(r["shares"]) == pytest.approx(1.0, rel=1e-12)
    for rounds in (0, 1):
        r = plan(sim, M=128 * 65, N=128 * 16, K=4096, a_vec=1, b_vec=1, rounds_mode=rounds)   # 1040 tiles: two rounds + 16
        assert r["tail128"] == 16 and r["ntiles"] == 1024 and r["blocks"] == 1024
        assert len(r["shares"]) == r["launches"] == (2 if rounds else 1)        # the tail launch has no record
        assert sum(r["shares"]) == pytest.approx(1 - 16 / 1040, rel=1e-12)
        assert r["shares"] == [c / 1040 for c in ([512, 512] if rounds else [1024])]


def test_panel32_images_reach_only_the_kernels_that_read_them(sim):
    cases = [dict(gram(256, 1 << 20), a_tiled=1), dict(right_trmm(1 << 20), a_tiled=1), dict(right_trmm(1 << 20), c_tiled=1),
             dict(right_trmm(1 << 20), a_tiled=1, c_tiled=1), dict(gram(256, 1 << 13), a_tiled=1), dict(right_trmm(8192), a_tiled=1),
             dict(right_trmm(1 << 20, n=512), c_tiled=1), dict(gram(128, 1 << 20), a_tiled=1, num_cu=4),
             dict(M=4096, N=256, K=256, a_tiled=1), dict(M=256, N=256, K=4096, ak=1, bkc=1, a_tiled=1, force_small=1)]
    got = [r["path"] for r in plans(sim, cases)]
    assert got[:4] == ["gram_ts", "trmm_ts32", "trmm_ts32", "trmm_ts32"]
    assert all(p in ("gram_ts", "trmm_ts32", "refused") for p in got), got


# The products of one n = 32768 cholinv step on one GPU (launches in resident rounds: capi_set_launch_rounds(1)) as CAPI_DEBUG_GEMM
# printed them, and their plans -- the same as the dispatcher's before it was split into planner and launcher (the kernel trace of a
# whole bench run, kernel by kernel with grids and LDS sizes, did not change).
#   M N K out_uplo tri_side tri_eff_upper beta batch ak a_is_b same_ld   path ts splitk launches tail128
CHOLINV_32768 = [
    "128 128 128 1 -1 0 1 0 1 1 1             small 128 1 1 0",
    "128 128 128 -1 1 1 0 8 0 0 0             small 128 1 1 0",
    "128 128 128 -1 0 1 0 8 0 0 1             small 128 1 1 0",
    "128 128 128 -1 0 0 0 0 1 0 0             small 128 1 1 0",
    "128 256 128 -1 0 0 0 0 1 0 0             small 128 1 1 0",
    "128 384 128 -1 0 0 0 0 1 0 0             small 128 1 1 0",
    "128 512 128 -1 0 0 0 0 1 0 0             small 128 1 1 0",
    "128 640 128 -1 0 0 0 0 1 0 0             small 128 1 1 0",
    "128 768 128 -1 0 0 0 0 1 0 0             small 128 1 1 0",
    "128 896 128 -1 0 0 0 0 1 0 0             small 128 1 1 0",
    "128 1024 128 -1 0 0 0 0 1 0 0            small 128 1 1 0",
    "128 1152 128 -1 0 0 0 0 1 0 0            small 128 1 1 0",
    "128 1280 128 -1 0 0 0 0 1 0 0            small 128 1 1 0",
    "128 1408 128 -1 0 0 0 0 1 0 0            small 128 1 1 0",
    "128 1536 128 -1 0 0 0 0 1 0 0            small 128 1 1 0",
    "128 1664 128 -1 0 0 0 0 1 0 0            small 128 1 1 0",
    "128 1792 128 -1 0 0 0 0 1 0 0            small 128 1 1 0",
    "128 1920 128 -1 0 0 0 0 1 0 0            small 128 1 1 0",
    "256 256 128 1 -1 0 1 0 1 1 1             small 128 1 1 0",
    "256 256 256 -1 1 1 0 4 0 0 0             small 256 1 1 0",
    "256 256 256 -1 0 1 0 4 0 0 1             small 256 1 1 0",
    "384 384 128 1 -1 0 1 0 1 1 1             small 128 1 1 0",
    "512 512 128 1 -1 0 1 0 1 1 1             small 128 1 1 0",
    "512 512 512 -1 1 1 0 2 0 0 0             small 256 1 1 0",
    "512 512 512 -1 0 1 0 2 0 0 1             small 256 1 1 0",
    "640 640 128 1 -1 0 1 0 1 1 1             small 128 1 1 0",
    "768 768 128 1 -1 0 1 0 1 1 1             small 128 1 1 0",
    "896 896 128 1 -1 0 1 0 1 1 1             small 128 1 1 0",
    "1024 1024 128 1 -1 0 1 0 1 1 1           small 128 1 1 0",
    "1024 1024 1024 -1 1 1 0 0 0 0 0          tile 64 1 1 0",
    "1024 1024 1024 -1 0 1 0 0 0 0 1          tile 64 1 1 0",
    "1152 1152 128 1 -1 0 1 0 1 1 1           small 128 1 1 0",
    "1280 1280 128 1 -1 0 1 0 1 1 1           small 128 1 1 0",
    "1408 1408 128 1 -1 0 1 0 1 1 1           small 128 1 1 0",
    "1536 1536 128 1 -1 0 1 0 1 1 1           small 128 1 1 0",
    "1664 1664 128 1 -1 0 1 0 1 1 1           small 128 1 1 0",
    "1792 1792 128 1 -1 0 1 0 1 1 1           tile 64 1 1 0",
    "1920 1920 128 1 -1 0 1 0 1 1 1           tile 64 1 1 0",
    "2048 2048 2048 1 -1 0 1 0 1 1 1          tile 128 3 1 0",
    "2048 2048 2048 -1 1 1 0 0 0 0 0          tile 64 1 1 0",
    "2048 2048 2048 -1 0 1 0 0 0 0 1          tile 64 1 1 0",
    "2048 2048 2048 -1 0 0 0 0 1 0 1          tile 64 1 1 0",
    "4096 4096 4096 1 -1 0 1 0 1 1 1          tile 64 1 1 0",
    "4096 4096 4096 -1 1 1 0 0 0 0 0          pair 128 1 1 0",
    "4096 4096 4096 -1 0 1 0 0 0 0 1          pair 128 1 1 0",
    "4096 4096 4096 -1 0 0 0 0 1 0 1          pair 128 1 1 0",
    "8192 8192 8192 1 -1 0 1 0 1 1 1          tile 128 1 4 32",
    "8192 8192 8192 -1 1 1 0 0 0 0 0          pair 128 1 4 0",
    "8192 8192 8192 -1 0 1 0 0 0 0 1          pair 128 1 4 0",
    "8192 8192 8192 -1 0 0 0 0 1 0 1          pair 128 1 4 0",
    "16384 16384 16384 1 -1 0 1 0 1 1 1       tile 128 1 16 64",
    "16384 16384 16384 -1 0 0 0 0 1 0 1       pair 128 1 16 0",
]


def test_plans_of_the_n32768_cholinv_step(sim):
    keys = "M N K out_uplo tri_side tri_eff_upper beta batch ak a_is_b same_ld".split()
    cases, want = [], []
    for row in CHOLINV_32768:
        f = row.split()
        cases.append(dict(zip(keys, f[:11]), bkc=1, a_vec=1, b_vec=1, rounds_mode=3, pair_mode=2, pair_rounds=1))
        want.append((f[11], *map(int, f[12:])))
    assert [(r["path"], r["ts"], r["splitk"], r["launches"], r["tail128"]) for r in plans(sim, cases)] == want
