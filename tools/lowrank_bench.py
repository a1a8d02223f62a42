"""The low-rank solve (cholesky::cholinv::lowrank_prepare / lowrank_solve / lowrank_quadratic_forms: M = L L^T + D on factor_pivoted()'s L) on one GPU
beside what it stands next to, in one run:

  kernels  through the C-ABI, on an n x k block of random numbers (no timing here depends on the values), k = 64, 512, 2048:
           capi_dsyrk alone, G = L^T L (upper, k x k) -- the floor of any prepare;
           capi_drow_pow(power -1/2, out of place: L_s = D^-1/2 L) against a device copy of the same bytes (b.copy_(a): 16 n k bytes moved);
           capi_drow_pow(power -1, in place) on an n x 32 block against a copy of that
  lowrank  driver.Cholinv on the RBF kernel matrix of tools/pchol_bench.py (random points of the unit square, every diagonal entry 1), per k after
           factor_pivoted(max_rank = k): lowrank_prepare with a general D (a user diagonal), with a uniform shift for the first time (G = L^T L formed),
           with another uniform shift (G cached); lowrank_solve at r = 1, 8, 32 with and without the residual norms; lowrank_quadratic_forms at
           r = 1, 32.  Wall clock of the Python call, which includes the host copies of B and X
  factor   Cholinv.factor() (config 2's policies) on the generator's SPD matrix of the same order

warm-up, then `--reps` rounds, median and min..max.  The parent process makes no GPU call: every leg runs in a child of its own under a time limit,
and a failed child ends the run.

    python tools/lowrank_bench.py [--n 32768] [--scale 0.01] [--reps 5] [--warmup 1] [--legs kernels,lowrank,factor] [--limit 500]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
RANKS = (64, 512, 2048)


def fmt(ts):
    return f"{statistics.median(ts):9.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]"


def kernels_child(n, scale, reps, warmup):
    import torch
    from capital_amd import capi
    h = capi.Handle(0)
    dev = "cuda:0"
    p = capi.ptr

    def timed(fn):
        ts = []
        for i in range(warmup + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    print(f"== the kernels of the low-rank solve through the C-ABI, n = {n}; {reps} rounds after {warmup} warm-up; capi version {h.L.capi_version()}, "
          f"library {os.path.basename(capi.LIB_PATH)}", flush=True)
    d = torch.rand(n, dtype=torch.float64, device=dev) + 0.5
    for k in [r for r in RANKS if r <= n]:
        L = torch.empty((k, n), dtype=torch.float64, device=dev).normal_()
        Ls = torch.empty((k, n), dtype=torch.float64, device=dev)
        G = torch.empty((k, k), dtype=torch.float64, device=dev)
        ts = timed(lambda: h.call("capi_dsyrk", capi.UPPER, capi.TRANS, k, n, 1.0, p(L), n, 0.0, p(G), k))
        tr = timed(lambda: h.call("capi_drow_pow", n, k, -0.5, p(d), 1.0, p(L), n, 0.0, p(Ls), n, None))
        tc = timed(lambda: Ls.copy_(L))
        ms, mr, mc = statistics.median(ts), statistics.median(tr), statistics.median(tc)
        print(f"-- k = {k}")
        print(f"   capi_dsyrk G = L^T L       {fmt(ts)}   {n * k * (k + 1.0) / (ms * 1e-3) / 1e12:7.2f} TFLOP/s (n k (k + 1) flop)")
        print(f"   capi_drow_pow(-1/2) n x k  {fmt(tr)}   moves {16.0 * n * k / 1e9:.3f} GB: {16.0 * n * k / (mr * 1e-3) / 1e12:.2f} TB/s")
        print(f"   copy of n x k              {fmt(tc)}   {16.0 * n * k / (mc * 1e-3) / 1e12:.2f} TB/s   capi_drow_pow / copy = {mr / mc:.2f}", flush=True)
        del L, Ls, G
    B = torch.empty((32, n), dtype=torch.float64, device=dev).normal_()
    B2 = torch.empty((32, n), dtype=torch.float64, device=dev)
    nrm = torch.empty(32, dtype=torch.float64, device=dev)
    tr = timed(lambda: h.call("capi_drow_pow", n, 32, -1.0, p(d), 1.0, p(B), n, 0.0, p(B), n, None))
    tn = timed(lambda: h.call("capi_drow_pow", n, 32, 1.0, p(d), -1.0, p(B), n, 1.0, p(B2.zero_()), n, p(nrm)))
    tc = timed(lambda: B2.copy_(B))
    print(f"-- the thin block, n x 32")
    print(f"   capi_drow_pow(-1) in place {fmt(tr)}")
    print(f"   capi_drow_pow(+1), beta = 1, with the column norms (and a memset)  {fmt(tn)}")
    print(f"   copy of n x 32             {fmt(tc)}   capi_drow_pow(-1) / copy = {statistics.median(tr) / statistics.median(tc):.2f}", flush=True)
    h.close()


def lowrank_child(n, scale, reps, warmup):
    import numpy as np
    import torch
    from capital_amd import driver
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(5)
    X = torch.rand((n, 2), dtype=torch.float64, device=dev, generator=g)
    A = torch.empty((n, n), dtype=torch.float64, device=dev)
    for j0 in range(0, n, 1024):
        D2 = ((X[j0:j0 + 1024, None, :] - X[None, :, :]) ** 2).sum(-1)
        A[j0:j0 + 1024] = torch.exp(D2 * (-0.5 / (scale * scale)))
    del D2
    Ah = A.cpu().numpy()
    del A, X
    torch.cuda.empty_cache()
    driver.init(0, 0, 1, None, use_torch_stream=False)
    try:
        pr = driver.Cholinv(n, c=1, complete_inv=0, split=1)
        pr.set_A(Ah.T)                                                        # (symmetric: the transposed view is the column-major image)
        del Ah
        rng = np.random.default_rng(5)
        diag = 10.0 ** rng.uniform(-4, -2, n)
        Bs = {r: np.asfortranarray(rng.standard_normal((n, r))) for r in (1, 8, 32)}

        def timed(fn, before=None):
            ts = []
            for i in range(warmup + reps):
                if before:
                    before()
                driver.sync()
                t0 = time.perf_counter()
                fn()
                driver.sync()
                if i >= warmup:
                    ts.append((time.perf_counter() - t0) * 1e3)
            return ts

        print(f"== Cholinv.lowrank_*, n = {n}, RBF kernel of random points of the unit square, length scale {scale}; wall clock of the Python calls (host copies "
              f"of B and X included); {reps} rounds after {warmup} warm-up", flush=True)
        for k in [r for r in RANKS if r <= n]:
            rank, trace, _ = pr.factor_pivoted(max_rank=k)
            out = {}
            tg = timed(lambda: out.update(pr.lowrank_prepare(diag=diag)))
            cg = out["cnorm1"]
            tf = timed(lambda: out.update(pr.lowrank_prepare(shift=1e-3)), before=lambda: pr.factor_pivoted(max_rank=k))
            tcch = timed(lambda: out.update(pr.lowrank_prepare(shift=1e-2)))
            print(f"-- max_rank = {k}: rank {rank}, trace left out {trace:.3e} of {n}")
            print(f"   lowrank_prepare, a general D             {fmt(tg)}   ||C||_1 = {cg:.3e}")
            print(f"   lowrank_prepare, a uniform shift, first  {fmt(tf)}   (G = L^T L formed)")
            print(f"   lowrank_prepare, a uniform shift, cached {fmt(tcch)}   ||C||_1 = {out['cnorm1']:.3e}, log det M = {out['logdet']:.6e}")
            for r in (1, 8, 32):
                t0 = timed(lambda: pr.lowrank_solve(Bs[r], residual=False))
                t1 = timed(lambda: pr.lowrank_solve(Bs[r], residual=True))
                Xs, res = pr.lowrank_solve(Bs[r])
                rel = float(np.max(res / np.linalg.norm(Bs[r], axis=0)))
                print(f"   lowrank_solve r = {r:2d}                     {fmt(t0)}   with the residual norms {fmt(t1)}   max ||b - M x|| / ||b|| = {rel:.1e}")
            for r in (1, 32):
                tq = timed(lambda: pr.lowrank_quadratic_forms(Bs[r]))
                print(f"   lowrank_quadratic_forms r = {r:2d}           {fmt(tq)}", flush=True)
        pr.close()
    finally:
        driver.finalize()


def factor_child(n, scale, reps, warmup):
    import pchol_bench
    pchol_bench.factor_child(n, scale, reps, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--scale", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", default="kernels,lowrank,factor")
    ap.add_argument("--limit", type=int, default=500, help="seconds per child")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        {"kernels": kernels_child, "lowrank": lowrank_child, "factor": factor_child}[a.child](a.n, a.scale, a.reps, a.warmup)
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
