"""On the device: the GPU twin of tests/test_summa_gloo.py.  matmult::summa's gemm, trmm and syrk in every form (tests/_summa_cases.py: the table,
the longdouble reference of the global product, the bound 2 (Kg + 4) u S, bit-identical depth replicas, untouched pad rows and triangles, no
NaN) on one rank and on the loopback grids 1x1x2 and 2x2x1 over the host-staged and the asynchronous transport -- the launcher of
tests/test_gpu_multirank.py.  All cases of a grid go into ONE launch: a test costs the start-up of its ranks and a few hundred tiny multiplies.

The 2x2x2 grid, eight ranks as threads, is test_summa_eight_ranks_as_threads_2x2x2 in tests/test_gpu_multirank.py: the session runs that file
first (tests/conftest.py), while the pytest process holds nothing on the card.  Measured on an MI355X, the same launch takes 9 s there, 22 s
beside a parent that holds one handle, and 109 s at this file's place in the session -- sixteen hardware queues of ranks beside the parent's."""
import os
import subprocess
import tempfile

import pytest

import _summa_cases as SC
from test_gpu_multirank import LOOPBACK, _launch

pytestmark = pytest.mark.gpu
ENV = {"CAPITAL_MIN_CHUNK_COLS": SC.MIN_CHUNK_COLS}
CASES = [{"tag": "summa", "kind": "summa"}]


def _check(world, d):
    from capital_amd import driver
    SC.check_launch(world, d, "summa_rank{}.npz", driver.SUMMA_FILL)


def test_summa_one_rank():
    """1x1x1: every form is one direct call of the tile kernels (and the one-rank communicator goes through RCCL)"""
    with tempfile.TemporaryDirectory() as d:
        _launch(1, {"dir": d, "cases": CASES}, extra_env=ENV)
        _check(1, d)


@pytest.mark.parametrize("world,mode", [(2, "host"), (4, "host"), (2, "async"), (4, "async")],
                         ids=["loopback2", "loopback4", "loopback2_async", "loopback4_async"])
def test_summa_on_loopback_grids(world, mode):
    """1x1x2 (column split, K slices, depth sums) and 2x2x1 (two K-class steps per layer, packed triangles on the wire), all ranks on GPU 0"""
    subprocess.check_call(["make", "-C", os.path.dirname(LOOPBACK), "-s"])
    with tempfile.TemporaryDirectory() as d:
        _launch(world, {"dir": d, "cases": CASES}, loopback=mode, extra_env=ENV)
        _check(world, d)
