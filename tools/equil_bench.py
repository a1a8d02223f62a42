"""The power-of-two equilibration of cholesky::cholinv::equilibrate on one GPU, measured alternately in the same process (tools/solve_bench.py's method:
warm-up, then `--reps` alternating rounds, median, min .. max and spread):

  (a) capi_dsym_scale2 on a column-major n x n matrix with lda = n, sign = +1 and sign = -1 in turn (every round ends on the matrix it began with):
      the upper triangle is read and written once, in place
  (b) the device copy of tools/hbm_copy_bench.py (b.copy_(a)) of the triangle's bytes: it reads and writes as many bytes as (a) does
  (c) capi_dpoequ2 (the n diagonal entries, one workgroup) and capi_drow_scale2 on n x 32 with its norms

then, on driver.Cholinv with config 2's policies (complete_inv = 0, split = 1, Serialize + SaveIntermediates), equilibrate(thresh = 2: forced on
generate()'s matrix) as a whole -- the diagonal pass, its 32-byte record read back, the scaling pass, the n scale factors fetched; wall clock up to a
device synchronise -- beside factor() of the scaled matrix and unequilibrate(), alternating.  The gate of the design: equilibrate() / factor() < 0.05,
so that cost is never a reason to skip it.  The parent process makes no GPU call: the order runs in a child under a time limit.

    python tools/equil_bench.py [--n 32768] [--reps 9] [--warmup 2] [--limit 600]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def line(name, ts, extra=""):
    med = statistics.median(ts)
    return f"   {name:26s} {med:9.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]   spread {(max(ts) - min(ts)) / med * 100:4.1f} %{extra}"


def child(n, reps, warmup):
    import ctypes as C
    import numpy as np
    import torch
    from capital_amd import capi, driver
    h = capi.Handle(0)
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(5)
    p = capi.ptr
    # a symmetric matrix graded over 16 decades (row j of the tensor is column j of the matrix: the same thing)
    A = torch.empty((n, n), dtype=torch.float64, device=dev)
    for j0 in range(0, n, 4096):
        A[j0:j0 + 4096] = torch.randn((min(4096, n - j0), n), dtype=torch.float64, device=dev, generator=g) * (1.0 / n ** 0.5)
    A = torch.triu(A)
    A += torch.triu(A, 1).T
    torch.diagonal(A).add_(2.0)
    d0 = 10.0 ** (torch.rand(n, dtype=torch.float64, device=dev, generator=g) * 16.0 - 8.0)
    A *= d0[:, None]
    A *= d0[None, :]
    np_ = n * (n + 1) // 2
    dscale = torch.empty(n, dtype=torch.float64, device=dev)
    rec = torch.zeros(4, dtype=torch.float64, device=dev)
    X = torch.randn((32, n), dtype=torch.float64, device=dev, generator=g)
    Y = torch.empty_like(X)
    nrm = torch.zeros(32, dtype=torch.float64, device=dev)
    csrc = torch.empty(np_, dtype=torch.float64, device=dev).normal_()
    cdst = torch.empty_like(csrc)
    before = A.clone() if n <= 16384 else A[:2048].clone()
    h.sync()
    ms = C.c_float()

    def timed(fn):
        h.call("capi_timer_start")
        fn()
        h.call("capi_timer_stop_ms", C.byref(ms))
        return ms.value

    print(f"== n = {n}, lda = n: the upper triangle is {8 * np_ / 1e9:.2f} GB; {reps} alternating rounds after {warmup} warm-up rounds; "
          f"capi version {h.L.capi_version()}", flush=True)
    h.call("capi_dpoequ2", n, p(A), n, p(dscale), p(rec))
    h.sync()
    r4 = rec.cpu().numpy()
    print(f"   capi_dpoequ2: scond = {r4[0]:.3e}, amax = {r4[1]:.3e}, amin = {r4[2]:.3e}, info = {int(r4[3])}")
    steps = {
        "a.dsym_scale2(+1)": lambda: h.call("capi_dsym_scale2", n, p(A), n, p(dscale), 1),
        "b.copy": lambda: cdst.copy_(csrc),
        "a.dsym_scale2(-1)": lambda: h.call("capi_dsym_scale2", n, p(A), n, p(dscale), -1),
        "c.dpoequ2": lambda: h.call("capi_dpoequ2", n, p(A), n, p(dscale), p(rec)),
        "c.drow_scale2 r=32 +norms": lambda: h.call("capi_drow_scale2", n, 32, p(dscale), -1, p(X), n, p(Y), n, p(nrm)),
    }
    times = {k: [] for k in steps}
    for i in range(warmup + reps):
        for k, fn in steps.items():
            tm = timed(fn)
            if i >= warmup:
                times[k].append(tm)
    h.sync()
    same = torch.equal(A if n <= 16384 else A[:2048], before)
    print(f"   after the rounds the matrix holds the bits it began with: {same}")
    both = times["a.dsym_scale2(+1)"] + times["a.dsym_scale2(-1)"]
    med = {k: statistics.median(v) for k, v in times.items()}
    mscale, mcopy = statistics.median(both), med["b.copy"]
    for k in steps:
        extra = ""
        if k.startswith("a."):
            extra = f"   this / copy = {med[k] / mcopy:.3f}   {2 * 8 * np_ / med[k] / 1e9:.2f} TB/s of {2 * 8 * np_ / 1e9:.2f} GB moved"
        elif k == "b.copy":
            extra = f"   {2 * 8 * np_ / med[k] / 1e9:.2f} TB/s of {2 * 8 * np_ / 1e9:.2f} GB moved"
        print(line(k, times[k], extra))
    ratio = mscale / mcopy
    print(f"   capi_dsym_scale2 (both signs) / copy = {ratio:.3f}: {'within 1.25 x the copy' if ratio <= 1.25 else 'LOSES: more than 1.25 x the copy'}", flush=True)
    assert same, "the scaling did not restore the matrix"
    del A, csrc, cdst, before, X, Y
    h.close()
    torch.cuda.empty_cache()

    driver.init(0, 0, 1, None, use_torch_stream=False)
    try:
        pr = driver.Cholinv(n, c=1, complete_inv=0, split=1, bc_mult=0 if n <= 2048 else -(max(n // 2048, 2).bit_length() - 1))
        pr.generate()
        te, tf, tu, out = [], [], [], None
        for i in range(warmup + reps):
            t0 = time.perf_counter()
            out = pr.equilibrate(2.0)
            driver.sync()
            t1 = time.perf_counter()
            pr.factor()
            driver.sync()
            t2 = time.perf_counter()
            pr.unequilibrate()
            driver.sync()
            t3 = time.perf_counter()
            if i >= warmup:
                te.append((t1 - t0) * 1e3)
                tf.append((t2 - t1) * 1e3)
                tu.append((t3 - t2) * 1e3)
        print(f"== Cholinv n = {n}, complete_inv = 0, split = 1, Serialize + SaveIntermediates, {pr.stats()}; {reps} alternating rounds after {warmup}; "
              f"wall clock of the Python calls up to a device synchronise; equilibrate(2.0) -> scaled = {out[0]}, scond = {out[1]:.3f}, amax = {out[2]:.3e}")
        print(line("equilibrate()", te))
        print(line("factor()", tf))
        print(line("unequilibrate()", tu))
        ratio = statistics.median(te) / statistics.median(tf)
        worst = max(te) / min(tf)
        print(f"   equilibrate() / factor() = {ratio:.4f} at the medians, {worst:.4f} at max / min: the gate is 0.05: {'PASS' if worst < 0.05 else 'LOSES'}", flush=True)
        pr.close()
        assert np.isfinite(ratio)
    finally:
        driver.finalize()
    return 0 if worst < 0.05 else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=600, help="seconds for the child")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.n, a.reps, a.warmup)
    try:
        rc = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), "--child", "--n", str(a.n), "--reps", str(a.reps), "--warmup", str(a.warmup)],
                            timeout=a.limit).returncode
    except subprocess.TimeoutExpired:
        print(f"no result within {a.limit} s; stopping", flush=True)
        return 124
    if rc != 0:
        print(f"the child ended with status {rc}", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
