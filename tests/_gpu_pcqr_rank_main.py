"""One rank of a column-pivoted CholeskyQR on several ranks (tests/test_gpu_cacqr_pivoted.py), in the style of tests/_gpu_svd_rank_main.py: a fresh
process, torch.distributed (gloo) only to ship the communicator's unique id, everything else through the product's driver.  Every rank builds the
same seeded panel (tests/_pcqr_cases.py), keeps its rows r, r + P, .. of A and of the right-hand sides, factors with pivoting, solves, and saves its
rows of Q with the rank, piv, R and X."""
import datetime
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _pcqr_cases as pc  # noqa: E402


def main():
    cfg = json.loads(sys.argv[1])
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ["LOCAL_RANK"])
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(local)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=int(os.environ.get("CAPITAL_TEST_GLOO_TIMEOUT_S", "300"))))
    from capital_amd import driver
    driver.init_distributed(local)
    for case in cfg["cases"]:
        print(f"rank {rank}: case {case['tag']} starts", flush=True)
        m, n, k = case["m"], case["n"], case["k"]
        A, B = pc.matrix(m, n, k), pc.rhs(m, n, k)
        q = driver.Cacqr(m, n, c=1, variant=2)
        q.set_A(np.asfortranarray(A[rank::world]))
        got = q.factor_pivoted()
        X, res = q.lstsq(np.asfortranarray(B[rank::world]))
        np.savez(os.path.join(cfg["dir"], f"{case['tag']}_rank{rank}.npz"), rank=got, piv=q.piv, R=q.R_pivoted(), Q=q.Q_pivoted(), X=X, res=res)
        q.close()
        dist.barrier()
    driver.finalize()
    dist.barrier()
    dist.destroy_process_group()
    print(f"rank {rank} ok", flush=True)


if __name__ == "__main__":
    main()
