"""capi_dpchol (the pivoted partial Cholesky under cholesky::cholinv::factor_pivoted) on one GPU beside what it stands next to, in one run:

  pchol    capi_dpchol on an RBF kernel matrix of random points of the unit square (every diagonal entry 1), max_rank = 64, 512, 2048 with LAPACK's default
           threshold: wall clock of the whole call (it ends with its own synchronisation, and reads the stop flag once per round of 64 steps), the rank
           reached, microseconds per step and the effective rate of the reads of L's earlier columns, 4 n k^2 bytes in all; beside a device copy of
           n x k doubles (b.copy_(a): it moves 16 n k bytes), which is what writing L once costs
  factor   Cholinv.factor() (config 2's policies: complete_inv = 0, split = 1, Serialize) on the generator's SPD matrix of the same order

warm-up, then `--reps` rounds, median and min..max.  The parent process makes no GPU call: every leg runs in a child of its own under a time limit,
and a failed child ends the run.

    python tools/pchol_bench.py [--n 32768] [--scale 0.01] [--reps 5] [--warmup 1] [--legs pchol,factor] [--limit 500]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RANKS = (64, 512, 2048)


def fmt(ts):
    return f"{statistics.median(ts):9.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]"


def pchol_child(n, scale, reps, warmup):
    import ctypes as C
    import torch
    from capital_amd import capi
    h = capi.Handle(0)
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(5)
    p = capi.ptr
    X = torch.rand((n, 2), dtype=torch.float64, device=dev, generator=g)
    A = torch.empty((n, n), dtype=torch.float64, device=dev)
    for j0 in range(0, n, 1024):
        D2 = ((X[j0:j0 + 1024, None, :] - X[None, :, :]) ** 2).sum(-1)
        A[j0:j0 + 1024] = torch.exp(D2 * (-0.5 / (scale * scale)))
    del D2
    piv = torch.empty(n, dtype=torch.int32, device=dev)
    d = torch.empty(n, dtype=torch.float64, device=dev)
    rank, trace = C.c_int(0), C.c_double(0.0)
    h.sync()
    print(f"== capi_dpchol, n = {n}, RBF kernel of random points of the unit square, length scale {scale}, LAPACK's default threshold; {reps} rounds after "
          f"{warmup} warm-up; capi version {h.L.capi_version()}, library {os.path.basename(capi.LIB_PATH)}", flush=True)
    for k in [r for r in RANKS if r <= n]:
        L = torch.empty((k, n), dtype=torch.float64, device=dev)
        csrc = torch.empty((k, n), dtype=torch.float64, device=dev).normal_()
        tp, tc = [], []
        for i in range(warmup + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h.call("capi_dpchol", n, p(A), n, -1.0, k, p(L), n, p(piv), p(d), C.byref(rank), C.byref(trace))
            t1 = time.perf_counter()
            L.copy_(csrc)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if i >= warmup:
                tp.append((t1 - t0) * 1e3)
                tc.append((t2 - t1) * 1e3)
        kk = rank.value
        m, mc = statistics.median(tp), statistics.median(tc)
        print(f"-- max_rank = {k}: rank {kk}, trace left out {trace.value:.3e} of {n}")
        print(f"   capi_dpchol        {fmt(tp)}   {m * 1e3 / max(kk, 1):8.2f} us per step   reads of L: {4.0 * n * kk * kk / 1e9:8.2f} GB, "
              f"{4.0 * n * kk * kk / (m * 1e-3) / 1e12:.3f} TB/s effective")
        print(f"   copy of n x k      {fmt(tc)}   moves {16.0 * n * k / 1e9:.3f} GB: {16.0 * n * k / (mc * 1e-3) / 1e12:.2f} TB/s   capi_dpchol / copy = {m / mc:.0f}",
              flush=True)
        del L, csrc
    h.close()


def factor_child(n, scale, reps, warmup):
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    try:
        pr = driver.Cholinv(n, c=1, complete_inv=0, split=1, bc_mult=0 if n <= 2048 else -(max(n // 2048, 2).bit_length() - 1))
        pr.generate()
        ts = []
        for i in range(warmup + reps):
            driver.sync()
            t0 = time.perf_counter()
            pr.factor()
            driver.sync()
            if i >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        print(f"== Cholinv.factor(), n = {n}, the generator's SPD matrix, complete_inv = 0, split = 1, Serialize + SaveIntermediates: R and R^-1")
        print(f"   factor()           {fmt(ts)}", flush=True)
        pr.close()
    finally:
        driver.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--scale", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", default="pchol,factor")
    ap.add_argument("--limit", type=int, default=500, help="seconds per child")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        {"pchol": pchol_child, "factor": factor_child}[a.child](a.n, a.scale, a.reps, a.warmup)
        return 0
    for leg in [x for x in a.legs.split(",") if x]:
        try:
            rc = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), "--child", leg, "--n", str(a.n), "--scale", str(a.scale), "--reps", str(a.reps),
                                 "--warmup", str(a.warmup)], timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"{leg}: no result within {a.limit} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"{leg}: the child ended with status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
