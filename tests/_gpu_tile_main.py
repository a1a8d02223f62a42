"""Child of tests/test_gpu_tile_kernels.py: the rows of one environment group of tests/_tile_cases.py (argv[1]: a JSON file), once each,
in a fresh process whose environment pins the plan (CAPI_SMALL, CAPI_FORCE_TS: read once per process) and turns the plan trace on
(CAPI_DEBUG_GEMM).  Every row is announced on stderr before its call, so the plan lines -- and a fault -- belong to a row; the C each
call leaves behind goes into the .npz argv[2] under the row's tag.  The parent does all the checking."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    with open(sys.argv[1]) as f:
        rows = json.load(f)
    import torch
    import _tile_cases as tc
    from capital_amd import capi
    print(f"num_cu {torch.cuda.get_device_properties(0).multi_processor_count}", file=sys.stderr, flush=True)
    h = capi.Handle(0)
    out = {}
    for r in rows:
        ops = tc.operands(r)
        dA = torch.from_numpy(ops["A"]).cuda()
        dB = None if ops["B"] is None else torch.from_numpy(ops["B"]).cuda()
        dC = torch.from_numpy(ops["C"]).cuda()
        torch.cuda.synchronize()
        pA = dA.data_ptr() + 8 * r["offA"]
        pB = None if dB is None else dB.data_ptr() + 8 * r["offB"]
        f, m, n, k = r["flags"], r["m"], r["n"], r["k"]
        print(f"row {r['tag']}", file=sys.stderr, flush=True)
        if r["fn"] == "gemm":
            h.call("capi_dgemm", f["ta"], f["tb"], m, n, k, r["alpha"], pA, ops["lda"], pB, ops["ldb"], r["beta"], capi.ptr(dC), ops["ldc"])
        elif r["fn"] == "syrk":
            h.call("capi_dsyrk", f["uplo"], f["trans"], n, k, r["alpha"], pA, ops["lda"], r["beta"], capi.ptr(dC), ops["ldc"])
        elif r["fn"] == "gemmt":
            h.call("capi_dgemmt", f["uplo"], f["ta"], 1 - f["ta"], n, k, r["alpha"], pA, ops["lda"], pB, ops["ldb"], r["beta"], capi.ptr(dC),
                   ops["ldc"])
        elif r["fn"] == "trmm_oop":
            h.call("capi_dtrmm_oop", f["side"], f["uplo"], f["trans"], f["diag"], m, n, r["alpha"], pA, ops["lda"], pB, ops["ldb"],
                   capi.ptr(dC), ops["ldc"])
        else:
            raise SystemExit(f"unknown fn {r['fn']}")
        h.sync()
        out[r["tag"]] = dC.cpu().numpy()
    h.close()
    np.savez(sys.argv[2], **out)
    print("cases done", flush=True)


if __name__ == "__main__":
    main()
