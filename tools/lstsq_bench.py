"""Phase times of the least-squares solve on the CholeskyQR factors (qr::cacqr::least_squares) on one GPU, new kernels against the route the
public C-ABI offered before them, measured alternately in the same process:

  (a) capi_dgemtn_ts (C = Q^T B)  +  capi_dtrsm (X = R^-1 C)  +  capi_dresid_ts (norms of B - A X, nothing written)
  (b) capi_dgemm(T, N)            +  capi_dtrsm               +  copy of B and capi_dgemm(N, N) into it (W = B - A X; no norms)

for (m, n) = (2^22, 256) and (2^21, 1024) and r = 1, 8, 32: warm-up, then `--reps` alternating rounds, median and min..max per phase, and
in the same rounds the device copy of tools/hbm_copy_bench.py (b.copy_(a)) sized to move the bytes of a streaming phase (a copy of N bytes moves 2 N).  The parent
process makes no GPU call: every shape runs in a child of its own under a time limit, and a failed child ends the run.

    python tools/lstsq_bench.py [--reps 9] [--shapes 4194304x256,2097152x1024] [--limit 240]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(m, n, reps, warmup):
    import ctypes as C
    import torch
    from capital_amd import capi
    h = capi.Handle(0)
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(1)
    A = torch.randn((n, m), dtype=torch.float64, device=dev, generator=g) * (1.0 / m ** 0.5)      # column-major m x n: stands for both Q and A
    R = (torch.triu(torch.randn((n, n), dtype=torch.float64, device=dev, generator=g)) + n * torch.eye(n, dtype=torch.float64, device=dev)).T.contiguous()
    ms = C.c_float()

    def timed(fn):
        h.call("capi_timer_start")
        fn()
        h.call("capi_timer_stop_ms", C.byref(ms))
        return ms.value

    def fmt(ts):
        return f"{statistics.median(ts):8.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]"

    print(f"== m = {m}, n = {n}: A is {8 * m * n / 1e9:.2f} GB; {reps} alternating rounds after {warmup} warm-up rounds; capi version {h.L.capi_version()}", flush=True)
    for r in (1, 8, 32):
        B = torch.randn((r, m), dtype=torch.float64, device=dev, generator=g)
        W = torch.empty_like(B)
        Ca, Cb = capi.zeros(n, r), capi.zeros(n, r)
        nrm = torch.zeros(r, dtype=torch.float64, device=dev)
        p = capi.ptr
        # the copy of tools/hbm_copy_bench.py (b.copy_(a) on the same stream), sized to MOVE the bytes of one streaming phase:
        # 8 m (n + r) in all, half of them read and half written
        by1 = 8 * m * (n + r)
        csrc = torch.empty(by1 // 16, dtype=torch.float64, device=dev).normal_()
        cdst = torch.empty_like(csrc)
        steps = {
            "a.gemtn": lambda: h.call("capi_dgemtn_ts", m, n, r, 1.0, p(A), m, p(B), m, 0.0, p(Ca), n),
            "b.gemm_TN": lambda: h.call("capi_dgemm", capi.TRANS, capi.NOTRANS, n, r, m, 1.0, p(A), m, p(B), m, 0.0, p(Cb), n),
            "a.trsm": lambda: h.call("capi_dtrsm", capi.LEFT, capi.UPPER, capi.NOTRANS, capi.NONUNIT, n, r, 1.0, p(R), n, p(Ca), n),
            "b.trsm": lambda: h.call("capi_dtrsm", capi.LEFT, capi.UPPER, capi.NOTRANS, capi.NONUNIT, n, r, 1.0, p(R), n, p(Cb), n),
            "a.resid": lambda: h.call("capi_dresid_ts", m, n, r, p(A), m, p(Ca), n, p(B), m, None, 0, p(nrm)),
            "b.copy+gemm_NN": lambda: (h.call("capi_memcpy_d2d_async", p(W), p(B), 8 * m * r),
                                       h.call("capi_dgemm", capi.NOTRANS, capi.NOTRANS, m, r, n, -1.0, p(A), m, p(Cb), n, 1.0, p(W), m)),
            "copy": lambda: cdst.copy_(csrc),
        }
        times = {k: [] for k in steps}
        for i in range(warmup + reps):
            for k, fn in steps.items():                       # (a) and (b) of each phase alternate
                t = timed(fn)
                if i >= warmup:
                    times[k].append(t)
        h.sync()
        # the two routes computed the same thing
        dC = (Ca - Cb).abs().max().item() / max(Cb.abs().max().item(), 1e-300)
        dn = ((W * W).sum(dim=1).sqrt() - nrm.sqrt()).abs().max().item() / max(nrm.sqrt().max().item(), 1e-300)
        print(f"-- r = {r}:  max |X_a - X_b| / max |X_b| = {dC:.2e}, max rel. difference of the residual norms = {dn:.2e}")
        for k in steps:
            print(f"   {k:16s} {fmt(times[k])}")
        med = {k: statistics.median(v) for k, v in times.items()}
        ta, tb = med["a.gemtn"] + med["a.trsm"] + med["a.resid"], med["b.gemm_TN"] + med["b.trsm"] + med["b.copy+gemm_NN"]
        print(f"   total (a) {ta:.3f} ms   total (b) {tb:.3f} ms   (b) / (a) = {tb / ta:.2f}")
        c1 = med["copy"]
        print(f"   the copy moves {by1 / 1e9:.2f} GB, the bytes of gemtn and of resid: {by1 / c1 / 1e9:.2f} TB/s at its median;  "
              f"copy / gemtn = {c1 / med['a.gemtn']:.2f} (with the copy's min .. max: {min(times['copy']) / med['a.gemtn']:.2f} .. {max(times['copy']) / med['a.gemtn']:.2f}), "
              f"copy / resid = {c1 / med['a.resid']:.2f} ({min(times['copy']) / med['a.resid']:.2f} .. {max(times['copy']) / med['a.resid']:.2f})", flush=True)
        del B, W, Ca, Cb, nrm, csrc, cdst
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default=f"{1 << 22}x256,{1 << 21}x1024")
    ap.add_argument("--limit", type=int, default=240, help="seconds per shape")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        m, n = (int(v) for v in a.child.split("x"))
        child(m, n, a.reps, a.warmup)
        return 0
    for shape in a.shapes.split(","):
        try:
            rc = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), "--child", shape, "--reps", str(a.reps), "--warmup", str(a.warmup)],
                                timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"{shape}: no result within {a.limit} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"{shape}: the child ended with status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
