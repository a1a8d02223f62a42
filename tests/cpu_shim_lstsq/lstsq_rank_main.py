"""One rank of the CPU rehearsal of qr::cacqr::least_squares (tests/test_lstsq_host.py): scqr_rank_main.py's set-up (the driver linked
against a CPU stand-in of the C-ABI, collectives over gloo) on the build of this directory, which adds the two streaming kernels in plain
C++ -- or, with CAPITAL_SHIM_LIB, on a stand-in that lacks them.  Every rank builds the same seeded problem (tests/_lstsq_cases.py) and keeps
its rows r, r + P, .. of A and B."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.join(TESTS, "cpu_shim"))

from rank_main import make_callback  # noqa: E402
import _lstsq_cases as lc  # noqa: E402


def main():
    cfg = json.loads(sys.argv[1])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from capital_amd import driver
    lib = C.CDLL(os.environ.get("CAPITAL_SHIM_LIB", os.path.join(HERE, "libcapital_driver_cpu_lstsq.so")), mode=C.RTLD_GLOBAL)
    driver.bind(lib)
    driver._drv = lib
    keep = make_callback()
    lib.capi_shim_set_collective(keep)
    assert lib.capital_drv_init(0, rank, world, None, None) == 0, lib.capital_drv_last_error()
    c = cfg.get("c", 1)
    q = driver.Cacqr(cfg["m"], cfg["n"], c=c, variant=cfg["sweeps"], serialize=cfg["serialize"], shifted=cfg["shifted"], complete_inv=1, bc_mult=-1)
    raised, factor_raised, out = "", "", {}
    if c == 1:
        A, B, _ = lc.problem(cfg["m"], cfg["n"], cfg["r"], cfg["kappa"], cfg["rho"])
        q.set_A(np.asfortranarray(A[rank::world]))
        B_loc = np.asfortranarray(B[rank::world])
    else:
        q.generate()
        B_loc = np.ones((q.m_loc, cfg["r"]), order="F")
    try:
        if cfg.get("factor", True):
            q.factor()
            out = {"R": q.R()}
    except driver.DriverError as e:
        factor_raised = str(e)
    try:
        X, res = q.lstsq(B_loc, residual=cfg.get("residual", True))
        out.update(X=X, res=res if res is not None else np.zeros(0), R_after=q.R() if c == 1 else np.zeros(0))
    except driver.DriverError as e:
        raised = str(e)
    dist.barrier()                         # every rank came back: nobody is left inside a collective
    np.savez(os.path.join(cfg["dir"], f"rank{rank}.npz"), raised=np.array(raised), factor_raised=np.array(factor_raised), **out)
    q.close()
    lib.capital_drv_finalize()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
