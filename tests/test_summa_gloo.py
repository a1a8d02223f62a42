"""CPU, over gloo and the oracle-backed shim (tests/cpu_shim): matmult::summa's gemm, trmm and syrk on the grids 1x1x2, 2x2x1 and 2x2x2 in EVERY
form -- both sides, both triangles, transposed or not, unit diagonals, general alpha and beta, beta = 0 over NaN -- through each of their paths
(column split, K slices, K-class steps, the chunk pipeline with packed triangles, staged strided blocks, pair / multi-path transfers and
triangular depth sums), by the public overloads and by the view-level engine on padded blocks.  cholinv and cacqr reach this code with three forms
of trmm, one of syrk and two of gemm; tests/_summa_cases.py has the table, the operands, the longdouble reference of the GLOBAL product and the
check: the any-order dot-product bound 2 (Kg + 4) u S elementwise, bit-identical depth replicas, untouched pad rows and other triangles, no NaN.
All cases of a grid run in one launch."""
import tempfile

import pytest

import _summa_cases as SC
from test_multirank_gloo import _launch, shim_lib  # noqa: F401  (the launcher and the fixture that builds the shim)


def run_grid(world, launch, only=None):
    """launch(world, cfg) runs the ranks; every case of every rank is then checked."""
    from capital_amd import driver
    with tempfile.TemporaryDirectory() as d:
        launch(world, {"kind": "summa", "dir": d, "only": only})
        SC.check_launch(world, d, "rank{}.npz", driver.SUMMA_FILL, only)


@pytest.mark.parametrize("world", [2, 4, 8], ids=["1x1x2", "2x2x1", "2x2x2"])
def test_summa_every_form_on_grids(shim_lib, world):
    run_grid(world, lambda w, cfg: _launch(w, cfg, timeout=600, extra_env={"CAPITAL_MIN_CHUNK_COLS": SC.MIN_CHUNK_COLS}))
