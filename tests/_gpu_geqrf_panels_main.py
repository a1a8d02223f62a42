"""Child process of tests/test_gpu_householder_qr.py::test_panels_at_tall_shapes.  Started with CAPI_GEQRF_NO_RECONSTRUCT=1, which
csrc/qr_f64.hip reads once per process: capi_dgeqrf + capi_dorgqr take the column-by-column Householder panels at tall shapes.
Prints, per shape, the errors of R (relative to max |R|), the reflectors and tau against the oracle's dgeqr2, and of Q against its dorg2r."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    assert os.environ.get("CAPI_GEQRF_NO_RECONSTRUCT"), "run with CAPI_GEQRF_NO_RECONSTRUCT=1"
    import torch
    import oracle
    from capital_amd import capi
    oracle.build()
    h = capi.Handle(0)
    for m, n in ((20011, 96), (16384, 256)):
        A = np.asfortranarray(np.random.default_rng(m * 1000 + n).random((m, n)) - 0.5)
        ref = A.copy(order="F")
        tau_ref = oracle.dgeqrf(ref)
        dA = capi.to_device(A)
        dtau = torch.zeros(n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        h.call("capi_dgeqrf", m, n, capi.ptr(dA), m, capi.ptr(dtau))
        h.sync()
        out, tau = capi.to_host(dA), dtau.cpu().numpy()
        h.call("capi_dorgqr", m, n, n, capi.ptr(dA), m, capi.ptr(dtau))
        h.sync()
        Q = capi.to_host(dA)
        Qref = out.copy(order="F")
        oracle.dorgqr(Qref, tau, n)
        Rref = np.triu(ref[:n])
        eR = np.abs(np.triu(out[:n]) - Rref).max() / np.abs(Rref).max()
        eV = np.abs(np.tril(out, -1) - np.tril(ref, -1)).max()
        print(f"panels {m}x{n}: R {eR:.3e} reflectors {eV:.3e} tau {np.abs(tau - tau_ref).max():.3e} Q {np.abs(Q - Qref).max():.3e}", flush=True)
    h.close()


if __name__ == "__main__":
    main()
