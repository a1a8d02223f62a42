"""bench.py on the GPU at a small order: a plain run prints the headline line and nothing it does not need, and
--dump-outputs writes the factors of its last timed step, equal to the oracle's on the same generated input."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_plain_run_dumps_the_factors_of_its_last_step(oracle, tmp_path):
    import bench
    n = 4096                      # two recursion levels above the one-GPU base case (order 2048); R and R^-1 are sampled by rows
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--n", str(n), "--steps", "2", "--warmup", "1",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["dtype"] == "f64" and line["config"]["n"] == n
    assert not {"config2", "cholesky_trsm_mode", "cacqr2", "cacqr2_config5", "mfma_f64_loop_tflops", "cpu_baseline"} & set(line)
    k = bench.DUMP_BYTES // (2 * 8 * n)
    rows = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(n, k, replace=False))
    R, Ri = np.load(tmp_path / "R.npy"), np.load(tmp_path / "Rinv.npy")
    assert R.dtype == Ri.dtype == np.float64 and R.shape == Ri.shape == (k, n)
    assert sorted(os.listdir(tmp_path)) == ["R.npy", "Rinv.npy"]
    A = oracle.distribute_symmetric(n, n, 0, 0, 1, 1)
    Rref, Riref, info = oracle.cholinv_factor(A, 0, 1, bench.bc_mult_for(n, 1, 1, bench.BASE_CASE_ORDER_ONE_GPU), 1, 1)
    assert info == 0
    assert np.abs(R - Rref[rows]).max() <= 1e-12 * np.abs(Rref).max()
    assert np.abs(Ri - Riref[rows]).max() <= 1e-12 * np.abs(Riref).max()
