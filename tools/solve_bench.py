"""The thin triangular product behind cholesky::cholinv::solve on one GPU, on synthetic triangles (no factorization), measured alternately in
the same process:

  (a) capi_dtrmm_thin on the operand as it lies: packed or full storage, NOTRANS and TRANS, the CAPI_UPPERTRI form on the whole triangle and
      the CAPI_RECT form on its top right quarter (the R12 block of a split at n / 2)
  (b) the device copy of tools/hbm_copy_bench.py (b.copy_(a)) sized to MOVE the triangle's bytes (a copy of N bytes moves 2 N)
  (c) the route through the earlier entry points: capi_serialize to full storage where the operand is packed, plus capi_dtrmm_oop on r columns

for n = 16384 and 32768 and r = 1, 8, 32: warm-up, then `--reps` alternating rounds, median and min..max.  With --resid ORDERS the residual
pass of solve, Rout <- B - S X with its norms on a symmetric S, by three routes and the copy, alternating in the same way:

  (a) capi_dresid_sym on the upper triangle
  (b) capi_dresid_ts over all of A (what solve ran before capi_dresid_sym existed)
  (c) two capi_dtrmm_thin(CAPI_UPPERTRI) calls on full storage, NOTRANS and TRANS, and a diagonal correction (two elementwise device kernels;
      no norms): the triangle read twice, with no kernel of its own

With --subst ORDERS the solve by SUBSTITUTION
on the factor itself (a synthetic, well-conditioned triangle), alternating:

  (a) capi_dtrsm_thin, NOTRANS and TRANS, packed and full storage (run once per LEAF candidate of trsm_thin_plan.h: CAPITAL_HIP_LIB names the build)
  (b) capi_dtrsm on full storage for the same r columns: what the TRSM-mode solve runs without info::solve_by_substitution
  (c) capi_dtrmm_thin(CAPI_UPPERTRI) on a packed triangle (the inverse mode's product with R^-1) and the copy of the triangle's bytes

and with --subst-e2e N Cholinv.solve with refine = 0 and 1, substitution off and on, in both factor modes (Serialize + SaveIntermediates: the only
packed configuration in which the TRSM mode solves with the flag off).  With --bounds N the condition estimate and the error bounds: capi_dsym_abs
beside capi_dresid_sym and the copy at r = 1, 8, 32, then Cholinv.rcond() and solve_expert beside solve in both factor modes (--orders "" runs it
alone).  With --e2e N one Cholinv.solve
(config 2's policies: complete_inv = 0, split = 1, Serialize) beside its factor().  The parent process makes no GPU call: every order runs in a
child of its own under a time limit, and a failed child ends the run.

    python tools/solve_bench.py [--reps 9] [--orders 16384,32768] [--resid 16384,32768] [--subst 32768] [--subst-e2e 32768] [--e2e 32768] [--bounds 32768] [--limit 300]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(n, reps, warmup):
    import ctypes as C
    import torch
    from capital_amd import capi
    h = capi.Handle(0)
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(1)
    p = capi.ptr
    # column-major n x n upper triangle (zeros below), its packed image, and the scratch that route (c) unpacks into
    Tf = torch.empty((n, n), dtype=torch.float64, device=dev)
    for j0 in range(0, n, 4096):                                          # (row j of the tensor is column j of the matrix)
        blk = torch.randn((min(4096, n - j0), n), dtype=torch.float64, device=dev, generator=g) * (1.0 / n ** 0.5)
        Tf[j0:j0 + blk.shape[0]] = torch.tril(blk, diagonal=j0)
    np_ = n * (n + 1) // 2
    Tp = torch.empty(np_, dtype=torch.float64, device=dev)
    h.call("capi_serialize", capi.RECT, capi.UPPERTRI, p(Tf), n, n, p(Tp), n, n, 0, n, 0, n, 0, n, 0, n)
    scratch = torch.zeros((n, n), dtype=torch.float64, device=dev)
    h.sync()
    ms = C.c_float()
    h2 = n // 2

    def timed(fn):
        h.call("capi_timer_start")
        fn()
        h.call("capi_timer_stop_ms", C.byref(ms))
        return ms.value

    def fmt(ts):
        return f"{statistics.median(ts):8.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]"

    def thin(shape, trans, m, k, r, T, ldt, col0, B, C_):
        h.call("capi_dtrmm_thin", shape, trans, m, k, r, 1.0, T, ldt, col0, p(B), n, 0.0, p(C_), n)

    def unpack():
        h.call("capi_serialize", capi.UPPERTRI, capi.RECT, p(Tp), n, n, p(scratch), n, n, 0, n, 0, n, 0, n, 0, n)

    def oop(trans, T, B, C_, r):
        h.call("capi_dtrmm_oop", capi.LEFT, capi.UPPER, trans, capi.NONUNIT, n, r, 1.0, T, n, p(B), n, p(C_), n)

    print(f"== n = {n}: the triangle is {8 * np_ / 1e9:.2f} GB packed, its quarter rectangle {8 * h2 * h2 / 1e9:.2f} GB; {reps} alternating rounds "
          f"after {warmup} warm-up rounds; capi version {h.L.capi_version()}", flush=True)
    for r in (1, 8, 32):
        B = torch.randn((r, n), dtype=torch.float64, device=dev, generator=g)
        Ca, Cc = capi.zeros(n, r), capi.zeros(n, r)
        csrc = torch.empty(np_ // 2, dtype=torch.float64, device=dev).normal_()
        cdst = torch.empty_like(csrc)
        rect_p = p(Tp) + 8 * (h2 * (h2 + 1) // 2)                         # element (0, h2) of the packed triangle
        rect_f = p(Tf) + 8 * h2 * n
        steps = {}
        for tn, t in (("N", capi.NOTRANS), ("T", capi.TRANS)):
            steps[f"a.tri_{tn}.packed"] = lambda t=t: thin(capi.UPPERTRI, t, n, n, r, p(Tp), 0, 0, B, Ca)
            steps[f"c.tri_{tn}.packed"] = lambda t=t: (unpack(), oop(t, p(scratch), B, Cc, r))
            steps[f"a.tri_{tn}.full"] = lambda t=t: thin(capi.UPPERTRI, t, n, n, r, p(Tf), n, 0, B, Ca)
            steps[f"c.tri_{tn}.full"] = lambda t=t: oop(t, p(Tf), B, Cc, r)
            steps[f"a.rect_{tn}.packed"] = lambda t=t: thin(capi.RECT, t, h2, h2, r, rect_p, 0, h2, B, Ca)
            steps[f"a.rect_{tn}.full"] = lambda t=t: thin(capi.RECT, t, h2, h2, r, rect_f, n, 0, B, Ca)
        steps["copy"] = lambda: cdst.copy_(csrc)
        times = {k: [] for k in steps}
        for i in range(warmup + reps):
            for k, fn in steps.items():
                tm = timed(fn)
                if i >= warmup:
                    times[k].append(tm)
        # the two routes computed the same thing (the last tri pair that ran into Ca and Cc: TRANS, full storage)
        thin(capi.UPPERTRI, capi.TRANS, n, n, r, p(Tp), 0, 0, B, Ca)
        oop(capi.TRANS, p(Tf), B, Cc, r)
        h.sync()
        d = (Ca - Cc).abs().max().item() / max(Cc.abs().max().item(), 1e-300)
        print(f"-- r = {r}:  max |C_a - C_c| / max |C_c| = {d:.2e}")
        med = {k: statistics.median(v) for k, v in times.items()}
        for k in steps:
            extra = ""
            if k.startswith("a.tri"):
                c = "c" + k[1:]
                extra = f"   copy / (a) = {med['copy'] / med[k]:.2f}   (c) / (a) = {med[c] / med[k]:.2f}   min (c) / max (a) = {min(times[c]) / max(times[k]):.2f}"
            elif k.startswith("a.rect"):
                extra = f"   {8 * h2 * h2 / med[k] / 1e9:.2f} TB/s"
            print(f"   {k:20s} {fmt(times[k])}{extra}")
        print(f"   the copy moves {8 * np_ / 1e9:.2f} GB: {8 * np_ / med['copy'] / 1e9:.2f} TB/s at its median", flush=True)
        del B, Ca, Cc, csrc, cdst
    h.close()


def resid_child(n, reps, warmup):
    import ctypes as C
    import torch
    from capital_amd import capi
    h = capi.Handle(0)
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(2)
    p = capi.ptr
    # a symmetric n x n matrix in full storage (row j of the tensor is column j of the matrix: the same thing)
    A = torch.empty((n, n), dtype=torch.float64, device=dev)
    for j0 in range(0, n, 4096):
        A[j0:j0 + 4096] = torch.randn((min(4096, n - j0), n), dtype=torch.float64, device=dev, generator=g) * (1.0 / n ** 0.5)
    A = torch.triu(A)
    A += torch.triu(A, 1).T
    diag = torch.diagonal(A).clone()
    np_ = n * (n + 1) // 2
    h.sync()
    ms = C.c_float()

    def timed(fn):
        h.call("capi_timer_start")
        fn()
        h.call("capi_timer_stop_ms", C.byref(ms))
        return ms.value

    print(f"== residual pass, n = {n}: the upper triangle is {8 * np_ / 1e9:.2f} GB, all of A {8 * n * n / 1e9:.2f} GB; {reps} alternating rounds after "
          f"{warmup} warm-up rounds; capi version {h.L.capi_version()}", flush=True)
    for r in (1, 8, 32):
        X = torch.randn((r, n), dtype=torch.float64, device=dev, generator=g)
        B = torch.randn((r, n), dtype=torch.float64, device=dev, generator=g)
        Ra, Rb, Rc = capi.zeros(n, r), capi.zeros(n, r), capi.zeros(n, r)
        na, nb = torch.zeros(r, dtype=torch.float64, device=dev), torch.zeros(r, dtype=torch.float64, device=dev)
        csrc = torch.empty(np_ // 2, dtype=torch.float64, device=dev).normal_()
        cdst = torch.empty_like(csrc)

        def route_c():
            h.call("capi_dtrmm_thin", capi.UPPERTRI, capi.NOTRANS, n, n, r, -1.0, p(A), n, 0, p(X), n, 0.0, p(Rc), n)
            h.call("capi_dtrmm_thin", capi.UPPERTRI, capi.TRANS, n, n, r, -1.0, p(A), n, 0, p(X), n, 1.0, p(Rc), n)
            Rc.add_(B).addcmul_(X, diag)                                  # both products counted the diagonal

        steps = {
            "a.dresid_sym": lambda: h.call("capi_dresid_sym", n, r, p(A), n, p(X), n, p(B), n, p(Ra), n, p(na)),
            "b.dresid_ts.full": lambda: h.call("capi_dresid_ts", n, n, r, p(A), n, p(X), n, p(B), n, p(Rb), n, p(nb)),
            "c.thin_N+T.full": route_c,
            "copy": lambda: cdst.copy_(csrc),
        }
        times = {k: [] for k in steps}
        for i in range(warmup + reps):
            for k, fn in steps.items():
                tm = timed(fn)
                if i >= warmup:
                    times[k].append(tm)
        h.sync()
        scale = max(Rb.abs().max().item(), 1e-300)
        print(f"-- r = {r}:  max |R_a - R_b| / max |R_b| = {(Ra - Rb).abs().max().item() / scale:.2e}, max |R_c - R_b| / max |R_b| = "
              f"{(Rc - Rb).abs().max().item() / scale:.2e}, max |norm_a - norm_b| / norm_b = {((na - nb).abs() / nb).max().item():.2e}")
        med = {k: statistics.median(v) for k, v in times.items()}
        for k in steps:
            ts = times[k]
            print(f"   {k:20s} {statistics.median(ts):8.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]   spread {(max(ts) - min(ts)) / med[k] * 100:4.1f} %"
                  f"   (b) / this = {med['b.dresid_ts.full'] / med[k]:.2f}")
        print(f"   the copy moves {8 * np_ / 1e9:.2f} GB: {8 * np_ / med['copy'] / 1e9:.2f} TB/s at its median", flush=True)
        del X, B, Ra, Rb, Rc, csrc, cdst
    h.close()


def subst_child(n, reps, warmup):
    import ctypes as C
    import torch
    from capital_amd import capi
    h = capi.Handle(0)
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(3)
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
    h.sync()
    ms = C.c_float()

    def timed(fn):
        h.call("capi_timer_start")
        fn()
        h.call("capi_timer_stop_ms", C.byref(ms))
        return ms.value

    print(f"== solve by substitution, n = {n}: the triangle is {8 * np_ / 1e9:.2f} GB packed; {reps} alternating rounds after {warmup} warm-up rounds; "
          f"capi version {h.L.capi_version()}, library {os.path.basename(capi.LIB_PATH)}", flush=True)
    for r in (1, 8, 32):
        B0 = torch.randn((r, n), dtype=torch.float64, device=dev, generator=g)
        X, Xb, Cm = torch.empty_like(B0), torch.empty_like(B0), capi.zeros(n, r)
        csrc = torch.empty(np_ // 2, dtype=torch.float64, device=dev).normal_()
        cdst = torch.empty_like(csrc)
        steps = {}
        for tn, t in (("N", capi.NOTRANS), ("T", capi.TRANS)):
            steps[f"a.dtrsm_thin_{tn}.packed"] = lambda t=t: h.call("capi_dtrsm_thin", t, n, r, p(Tp), 0, 0, p(X), n)
            steps[f"a.dtrsm_thin_{tn}.full"] = lambda t=t: h.call("capi_dtrsm_thin", t, n, r, p(Tf), n, 0, p(X), n)
            steps[f"b.dtrsm_{tn}.full"] = lambda t=t: h.call("capi_dtrsm", capi.LEFT, capi.UPPER, t, capi.NONUNIT, n, r, 1.0, p(Tf), n, p(Xb), n)
            steps[f"c.dtrmm_thin_{tn}.packed"] = lambda t=t: h.call("capi_dtrmm_thin", capi.UPPERTRI, t, n, n, r, 1.0, p(Tp), 0, 0, p(B0), n, 0.0, p(Cm), n)
        steps["copy"] = lambda: cdst.copy_(csrc)
        times = {k: [] for k in steps}
        for i in range(warmup + reps):
            for k, fn in steps.items():
                X.copy_(B0)                                               # the solves are in place: every one starts from the same right-hand side
                Xb.copy_(B0)
                tm = timed(fn)
                if i >= warmup:
                    times[k].append(tm)
        # the two routes compute the same thing: once more, TRANS, the thin solve on the packed and the block TRSM on the full operand
        X.copy_(B0)
        h.call("capi_dtrsm_thin", capi.TRANS, n, r, p(Tp), 0, 0, p(X), n)
        Xb.copy_(B0)
        h.call("capi_dtrsm", capi.LEFT, capi.UPPER, capi.TRANS, capi.NONUNIT, n, r, 1.0, p(Tf), n, p(Xb), n)
        h.sync()
        d = (X - Xb).abs().max().item() / max(Xb.abs().max().item(), 1e-300)
        print(f"-- r = {r}:  max |X_a - X_b| / max |X_b| = {d:.2e}")
        med = {k: statistics.median(v) for k, v in times.items()}
        for k in steps:
            extra = ""
            if k.startswith("a."):
                b = "b.dtrsm_" + k.split("_")[2].split(".")[0] + ".full"
                extra = f"   (b) / (a) = {med[b] / med[k]:.2f}   min (b) / max (a) = {min(times[b]) / max(times[k]):.2f}   (a) / copy = {med[k] / med['copy']:.2f}"
            print(f"   {k:26s} {statistics.median(times[k]):8.3f} ms [{min(times[k]):.3f} .. {max(times[k]):.3f}]{extra}")
        print(f"   the copy moves {8 * np_ / 1e9:.2f} GB: {8 * np_ / med['copy'] / 1e9:.2f} TB/s at its median; the chain of {n} rows costs "
              f"{min(med[k] for k in med if k.startswith('a.')) * 1e6 / n:.0f} ns per row at the fastest (a)", flush=True)
        del B0, X, Xb, Cm, csrc, cdst
    h.close()


def subst_e2e(n):
    import numpy as np
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    try:
        rng = np.random.default_rng(0)
        print(f"== Cholinv.solve, n = {n}, Serialize + SaveIntermediates, complete_inv = 0: best of 3, wall clock incl. the host copies of B and X")
        for trsm in (False, True):
            pr = driver.Cholinv(n, c=1, complete_inv=0, split=1, bc_mult=0 if n <= 2048 else -(max(n // 2048, 2).bit_length() - 1), trsm_mode=trsm)
            pr.generate()
            pr.factor()
            for r in (1, 8, 32):
                B = np.asfortranarray(rng.standard_normal((n, r)))
                for refine in (0, 1):
                    row = []
                    for on in (False, True):
                        pr.set_solve_substitution(on)
                        v = []
                        for _ in range(3):
                            t0 = time.perf_counter()
                            X, res = pr.solve(B, refine=refine, residual=True)
                            v.append((time.perf_counter() - t0) * 1e3)
                        row.append((min(v), float(res.max())))
                    print(f"   {'TRSM' if trsm else 'inverse'} mode r = {r:2d} refine = {refine}: substitution off {row[0][0]:8.1f} ms (max ||b - A x|| = {row[0][1]:.2e}), "
                          f"on {row[1][0]:8.1f} ms ({row[1][1]:.2e})", flush=True)
            pr.close()
    finally:
        driver.finalize()


def bounds_child(n, reps, warmup):
    """condition estimate and error bounds: the |.| pass beside the residual pass and the copy, then Cholinv.rcond() and solve_expert beside solve"""
    import ctypes as C
    import numpy as np
    import torch
    from capital_amd import capi, driver
    h = capi.Handle(0)
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(4)
    p = capi.ptr
    A = torch.empty((n, n), dtype=torch.float64, device=dev)
    for j0 in range(0, n, 4096):
        A[j0:j0 + 4096] = torch.randn((min(4096, n - j0), n), dtype=torch.float64, device=dev, generator=g) * (1.0 / n ** 0.5)
    A = torch.triu(A)
    A += torch.triu(A, 1).T
    np_ = n * (n + 1) // 2
    h.sync()
    ms = C.c_float()

    def timed(fn):
        h.call("capi_timer_start")
        fn()
        h.call("capi_timer_stop_ms", C.byref(ms))
        return ms.value

    print(f"== |A| |X| + |B| pass, n = {n}: the upper triangle is {8 * np_ / 1e9:.2f} GB; {reps} alternating rounds after {warmup} warm-up rounds; "
          f"capi version {h.L.capi_version()}", flush=True)
    for r in (1, 8, 32):
        X = torch.randn((r, n), dtype=torch.float64, device=dev, generator=g)
        B = torch.randn((r, n), dtype=torch.float64, device=dev, generator=g)
        Wa, Rb = capi.zeros(n, r), capi.zeros(n, r)
        ma, nb = torch.zeros(r, dtype=torch.float64, device=dev), torch.zeros(r, dtype=torch.float64, device=dev)
        csrc = torch.empty(np_ // 2, dtype=torch.float64, device=dev).normal_()
        cdst = torch.empty_like(csrc)
        steps = {
            "a.dsym_abs": lambda: h.call("capi_dsym_abs", n, r, p(A), n, p(X), n, p(B), n, p(Wa), n, p(ma)),
            "b.dresid_sym": lambda: h.call("capi_dresid_sym", n, r, p(A), n, p(X), n, p(B), n, p(Rb), n, p(nb)),
            "copy": lambda: cdst.copy_(csrc),
        }
        times = {k: [] for k in steps}
        for i in range(warmup + reps):
            for k, fn in steps.items():
                tm = timed(fn)
                if i >= warmup:
                    times[k].append(tm)
        h.sync()
        ref = (A.abs() @ X.abs().T).T + B.abs() if n <= 32768 else None
        if ref is not None:
            print(f"-- r = {r}:  max |W - torch| / max W = {(Wa - ref).abs().max().item() / ref.max().item():.2e}, "
                  f"max |colmax - max W| = {(ma - Wa.max(dim=1).values).abs().max().item():.1e}")
        med = {k: statistics.median(v) for k, v in times.items()}
        for k in steps:
            ts = times[k]
            print(f"   {k:16s} {statistics.median(ts):8.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]   this / (b) = {med[k] / med['b.dresid_sym']:.2f}"
                  f"   this / copy = {med[k] / med['copy']:.2f}")
        print(f"   the copy moves {8 * np_ / 1e9:.2f} GB: {8 * np_ / med['copy'] / 1e9:.2f} TB/s at its median", flush=True)
        del X, B, Wa, Rb, csrc, cdst, ref
    del A
    h.close()
    torch.cuda.empty_cache()

    driver.init(0, 0, 1, None, use_torch_stream=False)
    try:
        rng = np.random.default_rng(0)
        print(f"== Cholinv.rcond() and solve_expert beside solve, n = {n}, Serialize + SaveIntermediates, complete_inv = 0, refine = 1: medians of {reps} "
              f"alternating rounds after {warmup}, wall clock incl. the host copies of B and X")
        for trsm in (False, True):
            pr = driver.Cholinv(n, c=1, complete_inv=0, split=1, bc_mult=0 if n <= 2048 else -(max(n // 2048, 2).bit_length() - 1), trsm_mode=trsm)
            pr.generate()
            pr.factor()
            mode = "TRSM" if trsm else "inverse"
            v, out = [], None
            for i in range(warmup + reps):
                t0 = time.perf_counter()
                out = pr.rcond(details=True)
                if i >= warmup:
                    v.append((time.perf_counter() - t0) * 1e3)
            print(f"   {mode} mode rcond(): {statistics.median(v):8.2f} ms [{min(v):.2f} .. {max(v):.2f}]   rcond = {out[0]:.3e}, ||A||_1 = {out[1]:.3e}, "
                  f"{out[2]} products with A^-1", flush=True)
            for r in (1, 8, 32):
                B = np.asfortranarray(rng.standard_normal((n, r)))
                ts, te, res = [], [], None
                for i in range(warmup + reps):
                    t0 = time.perf_counter()
                    pr.solve(B, refine=1, residual=True)
                    t1 = time.perf_counter()
                    res = pr.solve_expert(B, refine=1, residual=True)
                    t2 = time.perf_counter()
                    if i >= warmup:
                        ts.append((t1 - t0) * 1e3)
                        te.append((t2 - t1) * 1e3)
                print(f"   {mode} mode r = {r:2d}: solve {statistics.median(ts):8.2f} ms [{min(ts):.2f} .. {max(ts):.2f}], solve_expert {statistics.median(te):8.2f} ms "
                      f"[{min(te):.2f} .. {max(te):.2f}]: the bounds add {statistics.median(te) - statistics.median(ts):.2f} ms   "
                      f"(max berr {res[3].max():.2e}, max ferr {res[2].max():.2e})", flush=True)
            pr.close()
    finally:
        driver.finalize()


def e2e(n):
    import numpy as np
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    try:
        pr = driver.Cholinv(n, c=1, complete_inv=0, split=1, bc_mult=0 if n <= 2048 else -(max(n // 2048, 2).bit_length() - 1))
        pr.generate()
        tf, ts = [], {}
        for _ in range(3):
            t0 = time.perf_counter()
            pr.factor()
            driver.sync()
            tf.append((time.perf_counter() - t0) * 1e3)
        rng = np.random.default_rng(0)
        for r in (1, 32):
            B = np.asfortranarray(rng.standard_normal((n, r)))
            for refine, residual in ((0, False), (1, True)):
                v = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    X, res = pr.solve(B, refine=refine, residual=residual)
                    v.append((time.perf_counter() - t0) * 1e3)
                ts[(r, refine)] = (min(v), None if res is None else float(res.max()))
        print(f"== end to end, n = {n}, {pr.stats()}: factor() {min(tf):.1f} ms (best of 3, wall clock)")
        for (r, refine), (t, res) in ts.items():
            print(f"   Cholinv.solve r = {r:2d} refine = {refine}: {t:8.1f} ms wall clock incl. the host copies of B and X"
                  + (f", max ||b - A x|| = {res:.2e}" if res is not None else ""), flush=True)
        pr.close()
    finally:
        driver.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--orders", default="16384,32768")
    ap.add_argument("--resid", default="", help="orders of the residual pass: capi_dresid_sym against capi_dresid_ts and two capi_dtrmm_thin calls")
    ap.add_argument("--subst", default="", help="orders of the solve by substitution: capi_dtrsm_thin against capi_dtrsm, capi_dtrmm_thin and the copy")
    ap.add_argument("--subst-e2e", type=int, default=0, help="order of Cholinv.solve with substitution off and on, in both factor modes (0: none)")
    ap.add_argument("--e2e", type=int, default=0, help="order of one end-to-end factor() + solve (0: none)")
    ap.add_argument("--bounds", type=int, default=0, help="order of the condition estimate and error bounds: capi_dsym_abs, Cholinv.rcond(), solve_expert (0: none)")
    ap.add_argument("--limit", type=int, default=300, help="seconds per child")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        if a.child.startswith("subst_e2e:"):
            subst_e2e(int(a.child[10:]))
        elif a.child.startswith("subst:"):
            subst_child(int(a.child[6:]), a.reps, a.warmup)
        elif a.child.startswith("e2e:"):
            e2e(int(a.child[4:]))
        elif a.child.startswith("bounds:"):
            bounds_child(int(a.child[7:]), a.reps, a.warmup)
        elif a.child.startswith("resid:"):
            resid_child(int(a.child[6:]), a.reps, a.warmup)
        else:
            child(int(a.child), a.reps, a.warmup)
        return 0
    jobs = [o for o in a.orders.split(",") if o] + [f"resid:{o}" for o in a.resid.split(",") if o] + [f"subst:{o}" for o in a.subst.split(",") if o]
    jobs += ([f"subst_e2e:{a.subst_e2e}"] if a.subst_e2e else []) + ([f"e2e:{a.e2e}"] if a.e2e else []) + ([f"bounds:{a.bounds}"] if a.bounds else [])
    for job in jobs:
        try:
            rc = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), "--child", job, "--reps", str(a.reps), "--warmup", str(a.warmup)],
                                timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"{job}: no result within {a.limit} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"{job}: the child ended with status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
