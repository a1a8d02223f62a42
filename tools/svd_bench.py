"""Times of the tall-skinny SVD on the CholeskyQR factors (qr::cacqr::svd) on one GPU, against the route a caller had before it, measured alternately
in the same process:

  kernel  capi_dgesvj on R (n = 256, 1024) in its three forms -- values only, V only, U and V -- with the sweep counts, against
          R to the host, numpy.linalg.svd there (the BLAS threads the environment gives: 16 on the measuring machine), U_R back to the device
  driver  driver.Cacqr at 2^22 x 256: factor(), svd(left=False) and svd(left=True) through the driver (the latter returns U to the host, 8.6 GB:
          the fetch is part of that figure), and in the same session the device part of left=True alone, capi_dgesvj with U + capi_dgemm (Q U_R)

R is the triangle of numpy's QR of a 4 n x n panel with log-spaced singular values 1 .. 1e-7.  Every call is timed on the wall clock between two
synchronisations (capi_dgesvj reads 4 bytes back per sweep, so device events alone would miss its host share): warm-up, then `--reps` alternating
rounds, median and min .. max.  The parent process makes no GPU call: every part runs in a child of its own under a time limit, and a failed child
ends the run.  The lines go to stdout and to --out.

    python tools/svd_bench.py [--reps 7] [--orders 256,1024] [--shape 4194304x256] [--limit 300] [--out profiles/cacqr_svd.txt]"""
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


def triangle(n, kappa=1e7, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    Uq, _ = np.linalg.qr(rng.standard_normal((4 * n, n)))
    Vq, _ = np.linalg.qr(rng.standard_normal((n, n)))
    R = np.linalg.qr((Uq * np.logspace(0, -np.log10(kappa), n)[None, :]) @ Vq.T, mode="r")
    return np.asfortranarray(np.triu(R * np.where(np.diag(R) < 0.0, -1.0, 1.0)[:, None]))


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
    print(f"== capi_dgesvj against the host route; {reps} alternating rounds after {warmup} warm-up rounds; capi version {h.L.capi_version()}; "
          f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}, torch threads {torch.get_num_threads()}", flush=True)
    for n in orders:
        Rh = triangle(n)
        dR = capi.to_device(Rh)
        dU, dV, ds = capi.empty(n, n), capi.empty(n, n), capi.empty(n, 1)
        sweeps = C.c_int()
        counts = {}

        def gesvj(form, U, V):
            h.call("capi_dgesvj", n, p(dR), n, p(U), n, p(ds), p(V), n, C.byref(sweeps))
            counts[form] = sweeps.value

        def host_route():
            R = capi.to_host(dR)                               # R to the host
            U, s, Vt = np.linalg.svd(R)
            return capi.to_device(U), s                        # U_R back to the device (sigma and V stay with the host's caller)

        steps = {
            "values only": lambda: gesvj("values only", None, None),
            "V only": lambda: gesvj("V only", None, dV),
            "U and V": lambda: gesvj("U and V", dU, dV),
            "host route": host_route,
        }
        times = {k: [] for k in steps}
        for i in range(warmup + reps):
            for k, fn in steps.items():
                t, out = wall(h.sync, fn)
                if i >= warmup:
                    times[k].append(t)
        s_dev = ds.cpu().numpy().ravel()
        ds_rel = np.max(np.abs(s_dev - out[1])) / out[1][0]
        N = n + (n & 1)
        print(f"-- n = {n}: {N - 1} launches of {N // 2} workgroups per sweep; max |sigma - sigma_host| / sigma_1 = {ds_rel:.2e}")
        for k in steps:
            extra = f"   {counts[k]} sweeps, {counts[k] * (N - 1)} step launches" if k in counts else ""
            print(f"   {k:12s} {fmt(times[k])}{extra}")
        med = {k: statistics.median(v) for k, v in times.items()}
        print(f"   host route / (U and V) = {med['host route'] / med['U and V']:.2f};  per step launch (U and V): "
              f"{1e3 * med['U and V'] / (counts['U and V'] * (N - 1)):.2f} us", flush=True)
    h.close()


def driver_child(m, n, reps, warmup):
    import ctypes as C
    import numpy as np
    import torch
    from capital_amd import capi, driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    q = driver.Cacqr(m, n, c=1, variant=2)
    q.generate()
    q.factor()
    L, hh = capi.load(), driver.handle_ptr()

    def call(name, *a):
        rc = getattr(L, name)(hh, *a)
        assert rc == 0, (name, rc)

    # the device part of svd(left=True) on blocks of the same shapes: capi_dgesvj with U, then U = Q U_R
    p = capi.ptr
    dR = capi.to_device(np.triu(q.R()))
    dQ = capi.empty(m, n)
    dQ.normal_()
    dUR, dV, ds, dU = capi.empty(n, n), capi.empty(n, n), capi.empty(n, 1), capi.empty(m, n)
    sweeps = C.c_int()
    torch.cuda.synchronize()

    def device_part():
        call("capi_dgesvj", n, p(dR), n, p(dUR), n, p(ds), p(dV), n, C.byref(sweeps))
        call("capi_dgemm", capi.NOTRANS, capi.NOTRANS, m, n, n, 1.0, p(dQ), m, p(dUR), n, 0.0, p(dU), m)

    steps = {
        "factor()": q.factor,
        "svd(left=False)": lambda: q.svd(left=False),
        "device part of left=True": device_part,
        "Q U_R alone": lambda: call("capi_dgemm", capi.NOTRANS, capi.NOTRANS, m, n, n, 1.0, p(dQ), m, p(dUR), n, 0.0, p(dU), m),
    }
    print(f"== driver.Cacqr {m} x {n} (A is {8 * m * n / 1e9:.2f} GB), CholeskyQR2; {reps} alternating rounds after {warmup} warm-up rounds", flush=True)
    times = {k: [] for k in steps}
    for i in range(warmup + reps):
        for k, fn in steps.items():
            t, _ = wall(driver.sync, fn)
            if i >= warmup:
                times[k].append(t)
    for k in steps:
        print(f"   {k:26s} {fmt(times[k])}")
    print(f"   Jacobi sweeps on R: {q.svd_sweeps} (driver), {sweeps.value} (device part)")
    t, (U, s, V) = wall(driver.sync, lambda: q.svd(left=True))
    print(f"   svd(left=True), once, U fetched to the host ({8 * m * n / 1e9:.2f} GB): {t:9.3f} ms;  cond2 = {s[0] / s[-1]:.3e}", flush=True)
    q.close()
    driver.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--orders", default="256,1024")
    ap.add_argument("--shape", default=f"{1 << 22}x256")
    ap.add_argument("--limit", type=int, default=300, help="seconds per part")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cacqr_svd.txt"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child == "kernel":
        kernel_child([int(v) for v in a.orders.split(",")], a.reps, a.warmup)
        return 0
    if a.child == "driver":
        m, n = (int(v) for v in a.shape.split("x"))
        driver_child(m, n, a.reps, a.warmup)
        return 0
    lines = []
    rc = 0
    for part in ("kernel", "driver"):
        cmd = [sys.executable, "-u", os.path.abspath(__file__), "--child", part, "--reps", str(a.reps), "--warmup", str(a.warmup), "--orders", a.orders,
               "--shape", a.shape]
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
