"""CPU: the numpy restatement of shifted CholeskyQR (tests/_scqr_ref.py) against Householder QR, and the host layer's shifted sweeps
(qr::cacqr with num_shifted > 0) on 1, 2 and 4 gloo ranks over the oracle-backed shim of the C-ABI (tests/cpu_shim, extended in tests/cpu_shim_scqr)."""
import json
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _scqr_ref as ref
from _scqr_ref import U64

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "cpu_shim")
SHIM_SCQR = os.path.join(HERE, "cpu_shim_scqr")      # the shim plus the shifted sweep's two entry points


@pytest.mark.parametrize("m,n,kappa,num_iter,num_shifted,graded", [(2048, 32, 1e10, 3, 1, False), (2048, 32, 1e10, 3, 1, True),
                                                                   (4096, 48, 1e12, 4, 2, False), (4096, 48, 1e12, 4, 2, True),
                                                                   (1024, 24, 1e4, 2, 0, False), (1024, 24, 1e4, 3, 1, True), (300, 1, 1.0, 3, 1, True)])
def test_reference_against_householder(m, n, kappa, num_iter, num_shifted, graded):
    """R is unique up to the signs of its rows; its forward error in either algorithm is bounded by the condition number of the
    problem times the rounding, column by column (the columns of a graded panel differ by 2^80):
    ||r_j - r_j^H|| <= 50 n u kappa ||r_j||.  Q^T Q = I to 50 n u.  And the diagnostic: the last (plain) sweep sees an orthonormal panel."""
    A = ref.panel(m, n, kappa, seed=n + num_iter, graded=graded)
    Q, R, stats = ref.scqr(A, num_iter, num_shifted)
    Rh = np.linalg.qr(A, mode="r")
    Rh = Rh * np.sign(np.diag(Rh))[:, None]
    assert np.all(np.tril(R, -1) == 0) and np.all(np.diag(R) > 0)
    err = np.linalg.norm(R - Rh, axis=0) / np.linalg.norm(Rh, axis=0)
    assert err.max() <= 50 * n * U64 * kappa, err.max()
    assert np.linalg.norm(Q.T @ Q - np.eye(n)) <= 50 * n * U64
    assert (np.linalg.norm(A - Q @ R, axis=0) / np.linalg.norm(A, axis=0)).max() <= 50 * n * U64
    assert len(stats) == num_iter and stats[-1]["cond_bound"] <= 4.0
    assert all(s["shift"] > 0 for s in stats[:num_shifted]) and all(s["shift"] == 0 for s in stats[num_shifted:])


def test_reference_equivariance_and_breakdown():
    """the restatement itself is exactly equivariant under power-of-two column scalings, and its plain CholeskyQR2 breaks down at 1e10"""
    A = ref.panel(2048, 40, 1e10, seed=3)
    e = ref.grading_exponents(40, seed=9, lo=-100, hi=100)
    Q0, R0, st0 = ref.scqr(A, 3, 1)
    Q1, R1, st1 = ref.scqr(np.ldexp(A, e[None, :]), 3, 1)
    np.testing.assert_array_equal(R1, np.ldexp(R0, e[None, :]))
    np.testing.assert_array_equal(Q1, Q0)
    assert st0 == st1
    with pytest.raises(np.linalg.LinAlgError):
        ref.scqr(A, 2, 0)
    G = np.diag([4.0, 0.0, 1.0, -1.0])
    assert ref.equilibrate_shift(G, 100)[4] == 2


# ---------------------------------------------------------------------------------------------------------------------------------
# the host layer on gloo ranks over the CPU shim
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim_lib():
    subprocess.check_call(["make", "-C", SHIM_SCQR, "-s"])
    return os.path.join(SHIM_SCQR, "libcapital_driver_cpu_scqr.so")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(world, cfg, timeout=600, extra_env=None):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1",
                   GLOO_SOCKET_IFNAME="lo", CAPITAL_MIN_CHUNK_COLS="8", CAPITAL_MULTIPATH="2", CAPITAL_MULTIPATH_MIN="8")
        env.update(extra_env or {})
        procs.append(subprocess.Popen([sys.executable, os.path.join(SHIM, "scqr_rank_main.py"), json.dumps(cfg)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=timeout)
            outs.append(o)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    return [np.load(os.path.join(cfg["dir"], f"rank{r}.npz")) for r in range(world)]


@pytest.mark.parametrize("m,n,kappa,variant,shifted,graded,serialize", [(4096, 32, 1e10, 3, 1, True, True), (4096, 48, 1e12, 4, 2, False, False)])
def test_shifted_1d_sharded_rows(shim_lib, m, n, kappa, variant, shifted, graded, serialize):
    """2 and 4 ranks, rows dealt cyclically: R is bit-identical on every rank (the shift is computed from the reduced Gram matrix,
    the same bits everywhere).  Against the 1-rank run only the all-reduce's summation order differs, a relative perturbation of the
    Gram matrix of order u: R moves by at most its condition number times that, ||r_j - r_j'|| <= 50 n u kappa ||r_j|| per column.  The
    assembled Q is orthonormal to 50 n u and Q R reproduces A, and the host layer agrees with the numpy restatement to the same bound."""
    cfg = {"m": m, "n": n, "kappa": kappa, "variant": variant, "shifted": shifted, "graded": graded, "serialize": serialize, "seed": 7}
    A = ref.panel(m, n, kappa, seed=7, graded=graded)
    Rs = {}
    for world in (1, 2, 4):
        with tempfile.TemporaryDirectory() as d:
            z = _launch(world, dict(cfg, dir=d))
            assert all(str(zz["raised"]) == "" for zz in z), [str(zz["raised"]) for zz in z]
            for zz in z[1:]:
                np.testing.assert_array_equal(zz["R"], z[0]["R"])
                np.testing.assert_array_equal(zz["stats"], z[0]["stats"])
            Q = np.zeros((m, n))
            for r, zz in enumerate(z):
                Q[r::world] = zz["Q"]
            R = Rs[world] = z[0]["R"]
            st = z[0]["stats"]
        assert np.all(np.tril(R, -1) == 0) and np.all(np.diag(R) > 0)
        assert np.linalg.norm(Q.T @ Q - np.eye(n)) <= 50 * n * U64
        assert (np.linalg.norm(A - Q @ R, axis=0) / np.linalg.norm(A, axis=0)).max() <= 50 * n * U64
        assert st.shape == (variant, 3) and np.all(st[:shifted, 0] > 0) and np.all(st[shifted:, :2] == 0) and st[-1, 2] <= 4.0
    _, Rref, st_ref = ref.scqr(A, variant, shifted)
    for R in (Rs[2], Rs[4], Rref):
        err = np.linalg.norm(R - Rs[1], axis=0) / np.linalg.norm(Rs[1], axis=0)
        assert err.max() <= 50 * n * U64 * kappa, err.max()


def test_shifted_on_a_cube_raises_on_every_rank(shim_lib):
    """c = 2 on 8 ranks: the Gram block is element-cyclic there; shifted sweeps are refused on every rank, before any collective"""
    with tempfile.TemporaryDirectory() as d:
        z = _launch(8, {"m": 512, "n": 32, "c": 2, "variant": 3, "shifted": 1, "serialize": False, "dir": d})
        raised = [str(zz["raised"]) for zz in z]
    for msg in raised:
        assert "1-D variant (c == 1) only" in msg, raised


def test_c_abi_without_the_entry_points_refuses_shifted_sweeps(shim_lib):
    """the host layer holds the two entry points as weak references: on a stand-in of the C-ABI that lacks them (the unextended shim of
    tests/cpu_shim) the library still loads, and factor() with shifted sweeps raises instead of calling through a null pointer"""
    subprocess.check_call(["make", "-C", SHIM, "-s"])
    with tempfile.TemporaryDirectory() as d:
        z = _launch(1, {"m": 2048, "n": 16, "kappa": 1e10, "variant": 3, "shifted": 1, "graded": False, "serialize": True, "seed": 1, "dir": d},
                    extra_env={"CAPITAL_SHIM_LIB": os.path.join(SHIM, "libcapital_driver_cpu.so")})
        raised = str(z[0]["raised"])
    assert "no shifted sweeps" in raised, raised
