"""One rank of the CPU rehearsal of SHIFTED CholeskyQR (tests/test_shifted_cqr_host.py): rank_main.py's set-up (the driver linked
against the oracle-backed shim -- the build of tests/cpu_shim_scqr, which adds the shifted sweep's two entry points -- collectives over gloo) with the `shifted` option of driver.Cacqr and an ill-conditioned input: every
rank builds the same seeded panel (tests/_scqr_ref.py) and keeps its rows r, r + P, .. of it."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from rank_main import make_callback  # noqa: E402
import _scqr_ref as ref  # noqa: E402


def main():
    cfg = json.loads(sys.argv[1])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from capital_amd import driver
    lib = C.CDLL(os.environ.get("CAPITAL_SHIM_LIB", os.path.join(os.path.dirname(HERE), "cpu_shim_scqr", "libcapital_driver_cpu_scqr.so")), mode=C.RTLD_GLOBAL)
    driver.bind(lib)
    driver._drv = lib
    keep = make_callback()
    lib.capi_shim_set_collective(keep)
    assert lib.capital_drv_init(0, rank, world, None, None) == 0, lib.capital_drv_last_error()
    c = cfg.get("c", 1)
    q = driver.Cacqr(cfg["m"], cfg["n"], c=c, variant=cfg["variant"], serialize=cfg["serialize"], shifted=cfg["shifted"], complete_inv=1, bc_mult=-1)
    raised, out = "", {}
    if c == 1:
        A = ref.panel(cfg["m"], cfg["n"], cfg["kappa"], seed=cfg["seed"], graded=cfg["graded"])
        q.set_A(np.asfortranarray(A[rank::world]))
    else:
        q.generate()
    try:
        q.factor()
        out = {"Q": q.Q(), "R": q.R(), "stats": np.array([[s["shift"], s["trace"], s["cond_bound"]] for s in q.sweep_stats()])}
    except driver.DriverError as e:
        raised = str(e)
    dist.barrier()                         # every rank came back: nobody is left inside a collective
    np.savez(os.path.join(cfg["dir"], f"rank{rank}.npz"), raised=np.array(raised), **out)
    q.close()
    lib.capital_drv_finalize()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
