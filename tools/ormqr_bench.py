"""capi_dormqr(CAPI_TRANS) and capi_dgels on one GPU at 2^22 x 256, r = 1, 8, 32, on a well-conditioned panel (capi_dgeqrf reconstructs from
CholeskyQR2) and at kappa 1e12 (the Householder panels run), beside

  copy          a device copy (b.copy_(a), tools/hbm_copy_bench.py) sized to MOVE the bytes capi_dormqr moves: per panel 2 x the panel's bytes and
                3 x the live rows of C (a copy of N bytes moves 2 N);
  dorgqr route  what the C-ABI offered before capi_dormqr: capi_dorgqr forms the m x n Q, capi_dgemtn_ts gives Q^T B -- its first n rows only, which
                is what a least-squares solve needs; capi_dormqr also delivers the tail;
  cacqr         driver.Cacqr factor() + lstsq() on its own generated panel of the same shape (well-conditioned case only).  lstsq takes B from the
                host, so its figure includes that transfer; it is a wall-clock time.

Warm-up, then `--reps` alternating rounds; median and min .. max, everything that is compared measured in the same session.  The parent process
makes no GPU call: each conditioning runs in a child of its own under a time limit, and a failed child ends the run.

    python tools/ormqr_bench.py [--reps 7] [--shape 4194304x256] [--limit 500]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(m, n, kind, reps, warmup):
    import ctypes as C
    import numpy as np
    import torch
    from capital_amd import capi
    h = capi.Handle(0)
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(1)
    p = capi.ptr
    ms = C.c_float()

    def timed(fn):
        h.call("capi_timer_start")
        fn()
        h.call("capi_timer_stop_ms", C.byref(ms))
        return ms.value

    def fmt(ts):
        return f"{statistics.median(ts):9.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]"

    # column-major m x n as an (n, m) tensor.  kappa 1e12: a near-orthonormal Gaussian panel times an n x n matrix with log-spaced singular values
    A = torch.randn((n, m), dtype=torch.float64, device=dev, generator=g) * (1.0 / m ** 0.5)
    if kind == "kappa1e12":
        rng = np.random.default_rng(1)
        V1, _ = np.linalg.qr(rng.standard_normal((n, n)))
        V2, _ = np.linalg.qr(rng.standard_normal((n, n)))
        M = (V1 * np.logspace(0, -12, n)[None, :]) @ V2.T
        A = torch.from_numpy(np.ascontiguousarray(M.T)).to(dev) @ A
    print(f"== {kind}: m = {m}, n = {n}: A is {8 * m * n / 1e9:.2f} GB; {reps} alternating rounds after {warmup} warm-up rounds; capi version "
          f"{h.L.capi_version()}", flush=True)
    F = A.clone()
    tau = torch.zeros(n, dtype=torch.float64, device=dev)
    work = torch.empty_like(A)
    tg = []
    for i in range(3):
        F.copy_(A)
        tg.append(timed(lambda: h.call("capi_dgeqrf", m, n, p(F), m, p(tau))))
    print(f"   capi_dgeqrf            {fmt(tg[1:])}   (first call, with its allocations: {tg[0]:.1f} ms)", flush=True)
    tq = []
    for i in range(3):
        work.copy_(F)
        tq.append(timed(lambda: h.call("capi_dorgqr", m, n, n, p(work), m, p(tau))))
    print(f"   capi_dorgqr            {fmt(tq[1:])}   (first call: {tq[0]:.1f} ms)", flush=True)
    Q = work.clone()
    for r in (1, 8, 32):
        B0 = torch.randn((r, m), dtype=torch.float64, device=dev, generator=g)
        Bw, Bg = B0.clone(), B0.clone()
        Cq = capi.zeros(n, r)
        nrm = torch.zeros(r, dtype=torch.float64, device=dev)
        tau2 = torch.zeros(n, dtype=torch.float64, device=dev)
        info = C.c_int(0)
        moved = sum(8 * (m - j0) * (2 * min(32, n - j0) + 3 * r) for j0 in range(0, n, 32))
        csrc = torch.empty(moved // 16, dtype=torch.float64, device=dev).normal_()
        cdst = torch.empty_like(csrc)
        steps = {
            "dormqr_T": (lambda: Bw.copy_(B0), lambda: h.call("capi_dormqr", capi.LEFT, capi.TRANS, m, r, n, p(F), m, p(tau), p(Bw), m)),
            "gemtn(Q^T B)": (None, lambda: h.call("capi_dgemtn_ts", m, n, r, 1.0, p(Q), m, p(B0), m, 0.0, p(Cq), n)),
            "copy": (None, lambda: cdst.copy_(csrc)),
            "dgels": (lambda: (work.copy_(A), Bg.copy_(B0)),
                      lambda: h.call("capi_dgels", m, n, r, p(work), m, p(tau2), p(Bg), m, p(nrm), C.byref(info))),
        }
        times = {k: [] for k in steps}
        for i in range(warmup + reps):
            for k, (prep, fn) in steps.items():
                if k == "dgels" and kind == "kappa1e12" and i >= 3:      # 0.1 s and more a call: three rounds
                    continue
                if prep:
                    prep()
                t = timed(fn)
                if i >= warmup or (k == "dgels" and kind == "kappa1e12" and i >= 1):
                    times[k].append(t)
        h.sync()
        same = (Bw[:, :n] - Cq).abs().max().item() / max(Cq.abs().max().item(), 1e-300)
        print(f"-- r = {r}: info {info.value}; max |dormqr's first n rows - gemtn(Q^T B)| / max = {same:.2e}")
        for k in steps:
            print(f"   {k:22s} {fmt(times[k])}")
        med = {k: statistics.median(v) for k, v in times.items()}
        route = statistics.median(tq[1:]) + med["gemtn(Q^T B)"]
        print(f"   dorgqr route (capi_dorgqr + capi_dgemtn_ts) {route:.3f} ms;  route / dormqr = {route / med['dormqr_T']:.2f}")
        print(f"   dormqr moves {moved / 1e9:.2f} GB: {moved / med['dormqr_T'] / 1e9:.2f} TB/s; the copy of the same bytes {moved / med['copy'] / 1e9:.2f} TB/s; "
              f"copy / dormqr = {med['copy'] / med['dormqr_T']:.2f} ({min(times['copy']) / med['dormqr_T']:.2f} .. {max(times['copy']) / med['dormqr_T']:.2f})",
              flush=True)
        del B0, Bw, Bg, Cq, csrc, cdst
    h.close()


def child_cacqr(m, n, reps):
    import numpy as np
    from capital_amd import driver
    import torch
    driver.init(0, 0, 1, None, use_torch_stream=False)
    try:
        q = driver.Cacqr(m, n, c=1, variant=2)
        q.generate()
        tf = []
        for i in range(reps + 1):
            q.generate()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            q.factor()
            torch.cuda.synchronize()
            tf.append(1e3 * (time.perf_counter() - t0))
        print(f"== cacqr (CholeskyQR2, its own generated panel) m = {m}, n = {n}: wall-clock times")
        print(f"   factor()               {statistics.median(tf[1:]):9.3f} ms [{min(tf[1:]):.3f} .. {max(tf[1:]):.3f}]")
        for r in (1, 8, 32):
            B = np.asfortranarray(np.random.default_rng(r).standard_normal((m, r)))
            tl = []
            for i in range(4):
                t0 = time.perf_counter()
                q.lstsq(B)
                tl.append(1e3 * (time.perf_counter() - t0))
            print(f"   lstsq() r = {r:2d}         {statistics.median(tl[1:]):9.3f} ms [{min(tl[1:]):.3f} .. {max(tl[1:]):.3f}]   (B comes from the host: "
                  f"{8 * m * r / 1e9:.2f} GB)", flush=True)
        q.close()
    finally:
        driver.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shape", default=f"{1 << 22}x256")
    ap.add_argument("--limit", type=int, default=500, help="seconds per child")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    m, n = (int(v) for v in a.shape.split("x"))
    if a.child == "cacqr":
        child_cacqr(m, n, a.reps)
        return 0
    if a.child:
        child(m, n, a.child, a.reps, a.warmup)
        return 0
    for kind in ("well", "kappa1e12", "cacqr"):
        try:
            rc = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), "--child", kind, "--shape", a.shape, "--reps", str(a.reps),
                                 "--warmup", str(a.warmup)], timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"{kind}: no result within {a.limit} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"{kind}: the child ended with status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
