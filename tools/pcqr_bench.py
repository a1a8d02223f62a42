"""Times of the column-pivoted CholeskyQR (qr::cacqr::factor_pivoted) on one GPU beside the plain path it stands next to, measured alternately in
the same process:

  kernel  capi_dpstrf (Cholesky with complete pivoting, one workgroup per 32-column panel plus one capi_dsyrk per panel) beside
          capi_dpotrf_trtri (what a plain sweep runs in its place: R and R^-1) on the same full-rank Gram matrix, n = 256, 1024, 2048.
          Both work in place, so every call starts from a fresh device copy of G; the copy is outside the timed interval
  driver  driver.Cacqr at 2^22 x 256: factor() (CholeskyQR2) and factor_pivoted() on a full-rank panel, then both calls on a panel of rank 200
          (factor() refuses it: the time to the refusal is printed for what it is worth)

The full-rank panel is a seeded 65536-row Gaussian block repeated down the panel with varying scales, the rank-200 one a 65536 x 200 block times a
200 x 256 Gaussian, repeated likewise: timing inputs, not accuracy tests (those are tests/test_gpu_cacqr_pivoted.py).  Every call is timed on the wall clock
between two synchronisations (capi_dpstrf reads 4 bytes back, so device events alone would miss its host share): warm-up, then `--reps` alternating
rounds, median and min .. max.  The parent process makes no GPU call: every part runs in a child of its own under a time limit, and a failed child
ends the run.  The lines go to stdout and to --out.

    python tools/pcqr_bench.py [--reps 7] [--orders 256,1024,2048] [--shape 4194304x256] [--rank 200] [--limit 300] [--out profiles/cacqr_pivoted.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fmt(ts):
    return f"{statistics.median(ts):9.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]"


def wall(sync, fn):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return 1e3 * (time.perf_counter() - t0), out


def kernel_child(orders, reps, warmup):
    import ctypes as C
    import numpy as np
    import torch
    from capital_amd import capi
    h = capi.Handle(0)
    p = capi.ptr
    print(f"== capi_dpstrf beside capi_dpotrf_trtri; {reps} alternating rounds after {warmup} warm-up rounds; capi version {h.L.capi_version()}", flush=True)
    for n in orders:
        A = np.random.default_rng(n).standard_normal((4 * n, n))
        G0 = capi.to_device(A.T @ A)
        G, Ri = capi.empty(n, n), capi.empty(n, n)
        piv = torch.zeros(n, dtype=torch.int32, device="cuda")
        rank = C.c_int()
        tol = 11.0 * (4.0 * n * n + n * (n + 1.0)) * 2.0 ** -53
        steps = {
            "capi_dpstrf": lambda: h.call("capi_dpstrf", n, p(G), n, tol, piv.data_ptr(), C.byref(rank)),
            "capi_dpotrf_trtri": lambda: h.call("capi_dpotrf_trtri", n, p(G), n, p(Ri), n),
        }
        times = {k: [] for k in steps}
        for i in range(warmup + reps):
            for k, fn in steps.items():
                G.copy_(G0)
                t, _ = wall(h.sync, fn)
                if i >= warmup:
                    times[k].append(t)
        assert rank.value == n and h.info() == 0, (rank.value, n)
        panels = (n + 31) // 32
        print(f"-- n = {n}: rank {rank.value}; capi_dpstrf is {panels} panel launches and {panels - 1} capi_dsyrk calls")
        for k in steps:
            print(f"   {k:18s} {fmt(times[k])}")
        med = {k: statistics.median(v) for k, v in times.items()}
        print(f"   capi_dpstrf / capi_dpotrf_trtri = {med['capi_dpstrf'] / med['capi_dpotrf_trtri']:.2f};  per pivot step: {1e3 * med['capi_dpstrf'] / n:.2f} us", flush=True)
    h.close()


def tall(m, n, rank):
    """an m x n timing panel of the given rank: a 65536-row seeded block repeated down the panel with scales 1 .. 2 (a repeated block keeps its rank)"""
    import numpy as np
    rng = np.random.default_rng(rank)
    rows = min(m, 1 << 16)
    base = rng.standard_normal((rows, rank))
    if rank < n:
        base = base @ rng.standard_normal((rank, n))
    A = np.empty((m, n), order="F")
    for t, r0 in enumerate(range(0, m, rows)):
        r1 = min(m, r0 + rows)
        A[r0:r1] = base[:r1 - r0] * (1.0 + (t % 17) / 16.0)
    return A


def driver_child(m, n, rank, reps, warmup):
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    q = driver.Cacqr(m, n, c=1, variant=2)
    print(f"== driver.Cacqr {m} x {n} (A is {8 * m * n / 1e9:.2f} GB); factor() is CholeskyQR2; {reps} alternating rounds after {warmup} warm-up rounds", flush=True)
    for label, k in (("full rank", n), (f"rank {rank}", rank)):
        q.set_A(tall(m, n, k))
        got = {}

        def plain():
            try:
                q.factor()
                got["factor"] = "ok"
            except driver.DriverError as e:
                got["factor"] = "refused: " + str(e)[:90]

        def pivoted():
            got["rank"] = q.factor_pivoted()

        steps = {"factor()": plain, "factor_pivoted()": pivoted}
        times = {s: [] for s in steps}
        for i in range(warmup + reps):
            for s, fn in steps.items():
                t, _ = wall(driver.sync, fn)
                if i >= warmup:
                    times[s].append(t)
        print(f"-- {label}: factor_pivoted found rank {got['rank']}; factor(): {got['factor']}")
        for s in steps:
            print(f"   {s:18s} {fmt(times[s])}")
        med = {s: statistics.median(v) for s, v in times.items()}
        print(f"   factor_pivoted() / factor() = {med['factor_pivoted()'] / med['factor()']:.2f}", flush=True)
    q.close()
    driver.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--orders", default="256,1024,2048")
    ap.add_argument("--shape", default=f"{1 << 22}x256")
    ap.add_argument("--rank", type=int, default=200)
    ap.add_argument("--limit", type=int, default=300, help="seconds per part")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cacqr_pivoted.txt"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child == "kernel":
        kernel_child([int(v) for v in a.orders.split(",")], a.reps, a.warmup)
        return 0
    if a.child == "driver":
        m, n = (int(v) for v in a.shape.split("x"))
        driver_child(m, n, a.rank, a.reps, a.warmup)
        return 0
    lines = []
    rc = 0
    for part in ("kernel", "driver"):
        cmd = [sys.executable, "-u", os.path.abspath(__file__), "--child", part, "--reps", str(a.reps), "--warmup", str(a.warmup), "--orders", a.orders,
               "--shape", a.shape, "--rank", str(a.rank)]
        try:
            res = subprocess.run(cmd, timeout=a.limit, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            text, rc = res.stdout, res.returncode
        except subprocess.TimeoutExpired as e:
            text, rc = (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or ""), 124
            text += f"\n{part}: no result within {a.limit} s; stopping\n"
        print(text, end="", flush=True)
        lines.append(text)
        if rc != 0:
            print(f"{part}: the child ended with status {rc}; stopping", flush=True)
            break
    if rc == 0:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("".join(lines))
    return rc


if __name__ == "__main__":
    sys.exit(main())
