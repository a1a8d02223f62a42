"""Child of tests/test_gpu_trmm_acc.py::test_the_plans_are_the_intended_ones: one triangular product per row of the parent's case table
(sizes only -- the operands are zeros), each announced on stderr, where CAPI_DEBUG_GEMM (read once per process, hence this process)
makes launch_gemm print the plan it chose.  Prints the device's CU count first: the expected plans are those of 256 CUs."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    rows = json.loads(sys.argv[1])
    import torch
    from capital_amd import capi
    print(f"num_cu {torch.cuda.get_device_properties(0).multi_processor_count}", file=sys.stderr, flush=True)
    h = capi.Handle(0)
    for r in rows:
        m, n = r["m"], r["n"]
        nt = m if r["side"] == 0 else n
        T = torch.zeros((nt, nt), dtype=torch.float64, device="cuda")
        B = torch.zeros((n, m), dtype=torch.float64, device="cuda")
        C = torch.zeros((n, m), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        print(f"row {r['tag']}", file=sys.stderr, flush=True)
        form = (r["side"], r["uplo"], r["trans"], r["diag"], m, n)
        if r["fn"] == "acc":
            h.call("capi_dtrmm_acc", *form, 1.0, capi.ptr(T), nt, capi.ptr(B), m, r["beta"], capi.ptr(C), m)
        elif r["fn"] == "oop":
            h.call("capi_dtrmm_oop", *form, 1.0, capi.ptr(T), nt, capi.ptr(B), m, capi.ptr(C), m)
        else:
            h.call("capi_dtrmm", *form, 1.0, capi.ptr(T), nt, capi.ptr(B), m)
        h.sync()
    h.close()
    print("plans ok", flush=True)


if __name__ == "__main__":
    main()
