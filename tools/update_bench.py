"""cholesky::cholinv::update on one GPU beside what it replaces, measured alternately in the same process:

  capi   capi_dchud and capi_dchud_inv alone, on a synthetic well-conditioned triangle in packed and in full storage, beside the device copy of
         tools/hbm_copy_bench.py (b.copy_(a)) sized to MOVE the triangle's bytes (a copy of N bytes moves 2 N).  An update is followed by the
         downdate with the same V, so that the triangle stays what it was over the rounds; both directions are timed.
  e2e    Cholinv.update (config 2's policies: complete_inv = 0, split = 1, Serialize) in inverse and in TRSM mode, wall clock incl. the host copy of V,
         beside set_A + factor() and factor() alone on the same matrix.  Update and downdate alternate here too.

for r = 1, 8, 32: warm-up, then `--reps` alternating rounds, median and min..max.  The parent process makes no GPU call: every leg runs in a child of
its own under a time limit, and a failed child ends the run.

    python tools/update_bench.py [--n 32768] [--reps 7] [--warmup 2] [--legs capi,e2e] [--limit 500]"""
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


def capi_child(n, reps, warmup):
    import ctypes as C
    import torch
    from capital_amd import capi
    h = capi.Handle(0)
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(5)
    p = capi.ptr
    # a well-conditioned upper triangle: unit diagonal, entries of size 1 / n above it (row j of the tensor is column j of the matrix)
    Tf = torch.empty((n, n), dtype=torch.float64, device=dev)
    for j0 in range(0, n, 4096):
        blk = torch.randn((min(4096, n - j0), n), dtype=torch.float64, device=dev, generator=g) * (1.0 / n)
        Tf[j0:j0 + blk.shape[0]] = torch.tril(blk, diagonal=j0 - 1)
    torch.diagonal(Tf).fill_(1.0)
    np_ = n * (n + 1) // 2
    Tp = torch.empty(np_, dtype=torch.float64, device=dev)
    h.call("capi_serialize", capi.RECT, capi.UPPERTRI, p(Tf), n, n, p(Tp), n, n, 0, n, 0, n, 0, n, 0, n)
    # the inverse's stand-in: the same triangle (the kernel's work does not depend on the values)
    Ip = Tp.clone()
    h.sync()
    ms = C.c_float()
    info = C.c_int(0)

    def timed(fn):
        h.call("capi_timer_start")
        fn()
        h.call("capi_timer_stop_ms", C.byref(ms))
        return ms.value

    print(f"== capi_dchud / capi_dchud_inv, n = {n}: the triangle is {8 * np_ / 1e9:.2f} GB packed; {reps} alternating rounds after {warmup} warm-up rounds; "
          f"capi version {h.L.capi_version()}, library {os.path.basename(capi.LIB_PATH)}", flush=True)
    for r in (1, 8, 32):
        V0 = torch.randn((r, n), dtype=torch.float64, device=dev, generator=g) * (0.5 / r ** 0.5)
        V = torch.empty_like(V0)
        log = torch.empty(h.L.capi_dchud_log_bytes(n, r) // 8, dtype=torch.float64, device=dev)
        csrc = torch.empty(np_ // 2, dtype=torch.float64, device=dev).normal_()
        cdst = torch.empty_like(csrc)

        def chud(sign, T, ldt):
            h.call("capi_dchud", sign, n, r, T, ldt, 0, p(V), n, p(log), C.byref(info))
            assert info.value == 0, info.value

        steps = {
            "dchud +1 packed": lambda: chud(1, p(Tp), 0),
            "dchud_inv +1 packed": lambda: h.call("capi_dchud_inv", 1, n, r, p(Ip), 0, 0, p(log), 0, n),
            "dchud -1 packed": lambda: chud(-1, p(Tp), 0),
            "dchud_inv -1 packed": lambda: h.call("capi_dchud_inv", -1, n, r, p(Ip), 0, 0, p(log), 0, n),
            "dchud +1 full": lambda: chud(1, p(Tf), n),
            "dchud -1 full": lambda: chud(-1, p(Tf), n),
            "copy": lambda: cdst.copy_(csrc),
        }
        times = {k: [] for k in steps}
        for i in range(warmup + reps):
            for k, fn in steps.items():
                V.copy_(V0)                                               # V is destroyed by every call
                tm = timed(fn)
                if i >= warmup:
                    times[k].append(tm)
        h.sync()
        med = {k: statistics.median(v) for k, v in times.items()}
        print(f"-- r = {r}:")
        for k in steps:
            ts = times[k]
            extra = "" if k == "copy" else f"   this / copy = {med[k] / med['copy']:.1f}   {med[k] * 1e6 / n:.0f} ns per step"
            print(f"   {k:22s} {fmt(ts)}   spread {(max(ts) - min(ts)) / med[k] * 100:4.1f} %{extra}")
        print(f"   the copy moves {8 * np_ / 1e9:.2f} GB: {8 * np_ / med['copy'] / 1e9:.2f} TB/s at its median; a panel of 32 steps is 2 launches: "
              f"{2 * ((n + 31) // 32) - 1} launches per capi_dchud", flush=True)
        del V0, V, log, csrc, cdst
    h.close()


def e2e_child(n, reps, warmup):
    import numpy as np
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    try:
        rng = np.random.default_rng(0)
        print(f"== Cholinv.update beside set_A + factor(), n = {n}, complete_inv = 0, split = 1, Serialize + SaveIntermediates: medians of {reps} alternating "
              f"rounds after {warmup}, wall clock (update: incl. the host copy of V)")
        for trsm in (False, True):
            pr = driver.Cholinv(n, c=1, complete_inv=0, split=1, bc_mult=0 if n <= 2048 else -(max(n // 2048, 2).bit_length() - 1), trsm_mode=trsm)
            pr.generate()
            A = pr.A()
            scale = 0.5 * np.sqrt(np.trace(A) / n)
            pr.factor()
            driver.sync()
            mode = "TRSM" if trsm else "inverse"
            B = np.asfortranarray(rng.standard_normal((n, 2)))
            Vs = {r: np.asfortranarray(rng.standard_normal((n, r)) * (scale / np.sqrt(r))) for r in (1, 8, 32)}
            t = {("factor",): [], ("set_A+factor",): []}
            t.update({(r, s): [] for r in Vs for s in ("up", "down")})
            for i in range(warmup + reps):
                for r, V in Vs.items():
                    for s in ("up", "down"):
                        t0 = time.perf_counter()
                        pr.update(V, downdate=(s == "down"))
                        driver.sync()
                        if i >= warmup:
                            t[(r, s)].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                pr.set_A(A)
                t1 = time.perf_counter()
                pr.factor()
                driver.sync()
                t2 = time.perf_counter()
                if i >= warmup:
                    t[("factor",)].append((t2 - t1) * 1e3)
                    t[("set_A+factor",)].append((t2 - t0) * 1e3)
            X, res = pr.solve(B)
            mf, ms_ = statistics.median(t[("factor",)]), statistics.median(t[("set_A+factor",)])
            print(f"   {mode} mode factor():          {fmt(t[('factor',)])}")
            print(f"   {mode} mode set_A + factor():  {fmt(t[('set_A+factor',)])}")
            for r in Vs:
                for s in ("up", "down"):
                    m = statistics.median(t[(r, s)])
                    verdict = "wins" if m < mf else "LOSES"
                    print(f"   {mode} mode update r = {r:2d} {s:4s}: {fmt(t[(r, s)])}   factor() / update = {mf / m:.2f} ({verdict}), set_A + factor() / update = {ms_ / m:.2f}",
                          flush=True)
            print(f"   {mode} mode: a solve on the last factors: max ||b - A x|| = {res.max():.2e}", flush=True)
            pr.close()
    finally:
        driver.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="capi,e2e")
    ap.add_argument("--limit", type=int, default=500, help="seconds per child")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        {"capi": capi_child, "e2e": e2e_child}[a.child](a.n, a.reps, a.warmup)
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
