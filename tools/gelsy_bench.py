"""capi_dgeqp3 and capi_dgelsy on one GPU, everything that is compared measured in the same session:

  geqp3   capi_dgeqp3 at n = 256, 1024, 2048 on triu of a Gaussian block (rtol = 0: all n steps run) beside
            capi_dpstrf on the Gram matrix R^T R of the same block (tol = 0), and
            the host route: R to the host, scipy.linalg.qr(pivoting=True, mode="raw") -- LAPACK's dgeqp3 on the threads the environment grants
            (OMP_NUM_THREADS; 16 on the machines this was written for) --, the image back to the device.  A wall-clock time with both transfers.
  gelsy   capi_dgelsy at 2^22 x 256, r = 1, 8, 32, in both solution modes beside capi_dgels, on a full-rank well-conditioned panel, and capi_dgelsy
          alone at rank 200 with sigma_k / sigma_1 = 1e-8 (capi_dgels does not solve that one).

Warm-up, then `--reps` alternating rounds; median and min .. max.  The parent process makes no GPU call: each part runs in a child of its own under
a time limit, and a failed child ends the run.

    python tools/gelsy_bench.py [--reps 7] [--shape 4194304x256] [--limit 500] > profiles/gelsy.txt"""
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


def child_geqp3(reps, warmup):
    import ctypes as C
    import numpy as np
    import scipy.linalg as sla
    import torch
    from capital_amd import capi
    h = capi.Handle(0)
    dev = "cuda:0"
    p = capi.ptr
    ms = C.c_float()

    def timed(fn):
        h.call("capi_timer_start")
        fn()
        h.call("capi_timer_stop_ms", C.byref(ms))
        return ms.value

    print(f"== geqp3: {reps} alternating rounds after {warmup} warm-up rounds; capi version {h.L.capi_version()}; host threads "
          f"{os.environ.get('OMP_NUM_THREADS', 'unset')}", flush=True)
    for n in (256, 1024, 2048):
        R = np.asfortranarray(np.triu(np.random.default_rng(n).standard_normal((n, n))))
        dR = capi.to_device(R)
        dG = dR @ dR.T                                        # (R^T R) as an (n, n) tensor of a symmetric matrix
        W, G = dR.clone(), dG.clone()
        tau = torch.zeros(n, dtype=torch.float64, device=dev)
        jp = torch.zeros(n, dtype=torch.int32, device=dev)
        piv = torch.zeros(n, dtype=torch.int32, device=dev)
        k, kp = C.c_int(0), C.c_int(0)
        host = {}

        def host_route():
            t0 = time.perf_counter()
            Rh = capi.to_host(dR)
            out = sla.qr(Rh, pivoting=True, mode="raw")       # ((qr, tau), R, jpvt)
            qr, jh = out[0][0], out[-1]
            host["img"] = capi.to_device(qr)
            torch.cuda.synchronize()
            host["jpvt"] = jh
            return 1e3 * (time.perf_counter() - t0)

        steps = {
            "capi_dgeqp3": (lambda: W.copy_(dR), lambda: timed(lambda: h.call("capi_dgeqp3", n, n, p(W), n, p(jp), p(tau), 0.0, C.byref(k)))),
            "capi_dpstrf (Gram)": (lambda: G.copy_(dG), lambda: timed(lambda: h.call("capi_dpstrf", n, p(G), n, 0.0, p(piv), C.byref(kp)))),
            "host route (wall)": (None, host_route),
        }
        times = {s: [] for s in steps}
        for i in range(warmup + reps):
            for s, (prep, fn) in steps.items():
                if prep:
                    prep()
                    torch.cuda.synchronize()
                t = fn()
                if i >= warmup:
                    times[s].append(t)
        same = int(np.sum(jp.cpu().numpy()[:k.value] == host["jpvt"][:k.value]))
        d = np.abs(np.diag(capi.to_host(W)))
        dh = np.abs(np.diag(capi.to_host(host["img"])))
        print(f"-- n = {n}: rank {k.value} (dpstrf {kp.value}); pivots equal to the host's: {same} of {k.value}; max | |r_jj| - host's | / r_00 = "
              f"{np.abs(d - dh).max() / dh[0]:.2e}")
        for s in steps:
            print(f"   {s:22s} {fmt(times[s])}")
        med = {s: statistics.median(v) for s, v in times.items()}
        print(f"   per step: {1e3 * med['capi_dgeqp3'] / n:.2f} us;  geqp3 / dpstrf = {med['capi_dgeqp3'] / med['capi_dpstrf (Gram)']:.2f};  "
              f"geqp3 / host route = {med['capi_dgeqp3'] / med['host route (wall)']:.2f}", flush=True)
    h.close()


def child_gelsy(m, n, kind, reps, warmup):
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

    A = torch.randn((n, m), dtype=torch.float64, device=dev, generator=g) * (1.0 / m ** 0.5)
    rank = n
    if kind == "rank200":                                      # A <- A[:, :200] diag(s) V^T: rank 200, sigma_k / sigma_1 = 1e-8
        rank = 200
        V, _ = np.linalg.qr(np.random.default_rng(1).standard_normal((n, rank)))
        M = np.logspace(0, -8, rank)[:, None] * V.T            # rank x n
        A = torch.from_numpy(np.ascontiguousarray(M.T)).to(dev) @ A[:rank]
    print(f"== gelsy, {kind}: m = {m}, n = {n}, planted rank {rank}: A is {8 * m * n / 1e9:.2f} GB; {reps} alternating rounds after {warmup} warm-up "
          f"rounds; capi version {h.L.capi_version()}", flush=True)
    work = torch.empty_like(A)
    tau, tauf, tauz = (torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(3))
    F, Z = capi.zeros(n, n), capi.zeros(n, n)
    jp = torch.zeros(n, dtype=torch.int32, device=dev)
    for r in (1, 8, 32):
        B0 = torch.randn((r, m), dtype=torch.float64, device=dev, generator=g)
        Bw = B0.clone()
        nrm = torch.zeros(r, dtype=torch.float64, device=dev)
        info, k = C.c_int(0), C.c_int(0)

        def prep():
            work.copy_(A)
            Bw.copy_(B0)

        def gelsy(mn):
            return lambda: h.call("capi_dgelsy", m, n, r, p(work), m, p(tau), p(F), n, p(tauf), p(jp), p(Z), n, p(tauz), p(Bw), m, 1e-13, mn, p(nrm),
                                  C.byref(k))

        steps = {"dgelsy minimum norm": gelsy(1), "dgelsy basic": gelsy(0)}
        if kind == "well":
            steps["dgels"] = lambda: h.call("capi_dgels", m, n, r, p(work), m, p(tau), p(Bw), m, p(nrm), C.byref(info))
        times = {s: [] for s in steps}
        for i in range(warmup + reps):
            for s, fn in steps.items():
                prep()
                t = timed(fn)
                if i >= warmup:
                    times[s].append(t)
        h.sync()
        print(f"-- r = {r}: rank found {k.value}" + (f"; dgels info {info.value}" if kind == "well" else ""))
        for s in steps:
            print(f"   {s:22s} {fmt(times[s])}")
        if kind == "well":
            med = {s: statistics.median(v) for s, v in times.items()}
            print(f"   dgelsy minimum norm / dgels = {med['dgelsy minimum norm'] / med['dgels']:.3f};  dgelsy basic / dgels = "
                  f"{med['dgelsy basic'] / med['dgels']:.3f}", flush=True)
        del B0, Bw
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shape", default=f"{1 << 22}x256")
    ap.add_argument("--limit", type=int, default=500, help="seconds per child")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    m, n = (int(v) for v in a.shape.split("x"))
    if a.child == "geqp3":
        child_geqp3(a.reps, a.warmup)
        return 0
    if a.child:
        child_gelsy(m, n, a.child, 3 if a.child == "rank200" else a.reps, 1 if a.child == "rank200" else a.warmup)
        return 0
    for kind in ("geqp3", "well", "rank200"):
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
