"""The operations on the cholinv factors themselves (cholesky::cholinv::apply / quadratic_forms / log_determinant / inverse_diagonal) on one GPU, each
beside what it stands next to, in one run:

  kernel   capi_dtri_rownorm2 on a packed triangle of order n, beside capi_dtrmm_thin (CAPI_UPPERTRI, NOTRANS, r = 1) on the same triangle -- the same
           bytes through the same partition -- and beside a device copy of the same bytes (b.copy_(a): it moves twice the triangle); the three alternate
           inside every round
  ops      Cholinv on the generator's SPD matrix, complete_inv = 0 (the block form) and 1 (the complete form), and complete_inv = 0 with substitution:
           apply() of each operator at r = 1 / 8 / 32 beside solve(refine=0, residual=False) of the same block, quadratic_forms, logdet and
           inverse_diagonal beside factor().  Wall clock of the Python call: host copies of B and of the result included (n x r doubles each way)

warm-up, then `--reps` rounds, median and min..max.  The parent process makes no GPU call: every leg runs in a child of its own under a time limit,
and a failed child ends the run.

    python tools/apply_bench.py [--n 32768] [--reps 5] [--warmup 1] [--legs kernel,ops] [--limit 500]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RS = (1, 8, 32)


def fmt(ts):
    return f"{statistics.median(ts):9.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]"


def kernel_child(n, reps, warmup):
    import torch
    from capital_amd import capi
    h = capi.Handle(0)
    dev = "cuda:0"
    p = capi.ptr
    count = n * (n + 1) // 2
    T = torch.empty(count, dtype=torch.float64, device=dev).normal_()
    T2 = torch.empty_like(T)
    b = torch.empty(n, dtype=torch.float64, device=dev).normal_()
    c = torch.empty(n, dtype=torch.float64, device=dev)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    legs = {
        "capi_dtri_rownorm2": lambda: h.call("capi_dtri_rownorm2", capi.UPPERTRI, n, n, p(T), 0, 0, 0.0, p(out)),
        "capi_dtrmm_thin r=1": lambda: h.call("capi_dtrmm_thin", capi.UPPERTRI, capi.NOTRANS, n, n, 1, 1.0, p(T), 0, 0, p(b), n, 0.0, p(c), n),
        "copy of the triangle": lambda: T2.copy_(T),
    }
    ts = {k: [] for k in legs}
    for i in range(warmup + reps):
        for k, f in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if i >= warmup:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    gb = 8.0 * count / 1e9
    print(f"== packed triangle of order {n}: {gb:.2f} GB; {reps} rounds after {warmup} warm-up, the three legs alternate; capi version {h.L.capi_version()}")
    for k in legs:
        moved = 2 * gb if k.startswith("copy") else gb
        print(f"   {k:22s} {fmt(ts[k])}   {moved / statistics.median(ts[k]):6.2f} TB/s of {moved:.2f} GB")
    m = {k: statistics.median(v) for k, v in ts.items()}
    print(f"   rownorm2 / dtrmm_thin(r = 1) = {m['capi_dtri_rownorm2'] / m['capi_dtrmm_thin r=1']:.3f}", flush=True)
    h.close()


def timed(f, reps, warmup, sync):
    ts = []
    for i in range(warmup + reps):
        sync()
        t0 = time.perf_counter()
        f()
        sync()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def ops_child(n, reps, warmup):
    import numpy as np
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    try:
        bc = 0 if n <= 2048 else -(max(n // 2048, 2).bit_length() - 1)
        rng = np.random.default_rng(1)
        B = np.asfortranarray(rng.standard_normal((n, max(RS))))
        for complete_inv in (0, 1):
            pr = driver.Cholinv(n, c=1, complete_inv=complete_inv, split=1, bc_mult=bc)
            pr.generate()
            tf = timed(pr.factor, reps, warmup, driver.sync)
            h1 = n >> 1
            print(f"== Cholinv n = {n}, complete_inv = {complete_inv}, split = 1, Serialize + SaveIntermediates; {reps} rounds after {warmup} warm-up; wall clock of the "
                  f"Python calls, host copies included")
            print(f"   factor()                      {fmt(tf)}")
            for subst in ((False, True) if complete_inv == 0 else (False,)):
                pr.set_solve_substitution(subst)
                print(f"-- the inverses by {'substitution on R' if subst else ('the block form' if complete_inv == 0 else 'products with the complete R^-1')}")
                for r in RS:
                    b = np.asfortranarray(B[:, :r])
                    ts = timed(lambda: pr.solve(b, refine=0, residual=False), reps, warmup, driver.sync)
                    line = f"   r = {r:2d}  solve(refine=0) {statistics.median(ts):8.3f}"
                    for op in ("R", "RT", "Rinv", "RinvT"):
                        if subst and op in ("R", "RT"):
                            continue
                        ta = timed(lambda: pr.apply(b, op), reps, warmup, driver.sync)
                        line += f"   {op} {statistics.median(ta):8.3f} [{min(ta):.3f} .. {max(ta):.3f}]"
                    tq = timed(lambda: pr.quadratic_forms(b), reps, warmup, driver.sync)
                    print(line + f"   quadratic_forms {statistics.median(tq):8.3f}  (ms)", flush=True)
            pr.set_solve_substitution(False)
            print(f"   logdet()                      {fmt(timed(pr.logdet, reps, warmup, driver.sync))}")
            td = timed(pr.inverse_diagonal, reps, warmup, driver.sync)
            extra = f"; extra memory of the block form: {8.0 * h1 * (n - h1) / 1e9:.2f} GB for the formed R^-1_12" if complete_inv == 0 else ""
            print(f"   inverse_diagonal()            {fmt(td)}   = {statistics.median(td) / statistics.median(tf):.3f} of factor(){extra}", flush=True)
            pr.close()
    finally:
        driver.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", default="kernel,ops")
    ap.add_argument("--limit", type=int, default=500, help="seconds per child")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        {"kernel": kernel_child, "ops": ops_child}[a.child](a.n, a.reps, a.warmup)
        return 0
    for leg in [x for x in a.legs.split(",") if x]:
        try:
            rc = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), "--child", leg, "--n", str(a.n), "--reps", str(a.reps), "--warmup", str(a.warmup)],
                                timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"{leg}: no result within {a.limit} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"{leg}: the child ended with status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
