"""CPU: the surface of the least-squares solve (header, built library, driver binding), the two fp64 references of
tests/_lstsq_cases.py against each other on every case the GPU test uses, and the host logic of qr::cacqr::least_squares on 1, 2 and 4
gloo ranks over a CPU stand-in of the C-ABI that has the two streaming kernels in plain C++ (tests/cpu_shim_lstsq) -- and on the unextended
stand-in (tests/cpu_shim), where it must refuse while factor() still runs."""
import json
import os
import re
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _lstsq_cases as lc
from _scqr_ref import U64

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHIM = os.path.join(HERE, "cpu_shim")
SHIM_LSTSQ = os.path.join(HERE, "cpu_shim_lstsq")


def test_entry_points_are_declared_exported_and_bound():
    from capital_amd import capi, driver
    hdr = open(os.path.join(ROOT, "include", "capital_hip.h")).read()
    assert {"capi_dgemtn_ts", "capi_dresid_ts"} <= set(capi.declared_symbols())
    assert re.search(r"CAPI_TS_MAX_RHS\s*=\s*32", hdr)
    assert "capi_dgemtn_ts" in capi._SIGS and "capi_dresid_ts" in capi._SIGS
    lib = os.path.join(ROOT, "capital_amd", "libcapital_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libcapital_hip.so has not been built")
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    for s in ("capi_dgemtn_ts", "capi_dresid_ts"):
        assert re.search(rf"\bT {s}\b", exported), s

    class Lib:                                                  # driver.bind declares the signature on whatever library object it is given
        def __getattr__(self, name):
            f = type("F", (), {})()
            setattr(self, name, f)
            return f
    D = driver.bind(Lib())
    assert len(D.capital_cacqr_lstsq.argtypes) == 5
    assert "capital_cacqr_lstsq" in open(os.path.join(ROOT, "capital_amd", "drivers", "capital_driver.cpp")).read()
    assert callable(driver.Cacqr.lstsq)


@pytest.mark.parametrize("m,n,r,kappa,sweeps,shifted,rho", lc.CASES, ids=lc.IDS)
def test_the_two_references_agree(m, n, r, kappa, sweeps, shifted, rho):
    """Householder QR + triangular solve against the numpy restatement of the sweeps + triangular solve on every case of the GPU test: the
    ratio of their forward errors stays within [0.1, 10], so the rule `within 10 x of the larger` has room; and numpy's ||b - A x|| is rho"""
    A, B, x_true = lc.problem(m, n, r, kappa, rho)
    eta_h, eta_s = lc.reference_etas(A, B, x_true, sweeps, shifted)
    print(f"{m}x{n} r={r} kappa={kappa:.0e} {sweeps}/{shifted} rho={rho:g}: eta Householder {eta_h:.2e}, numpy sweeps {eta_s:.2e}, ratio {eta_s / eta_h:.2f}")
    assert 0.1 <= max(eta_s, U64) / max(eta_h, U64) <= 10.0, (eta_h, eta_s)
    X = lc.solve_householder(A, B)
    res = np.linalg.norm(B.astype(lc.LD) - A.astype(lc.LD) @ X.astype(lc.LD), axis=0).astype(np.float64)
    assert np.all(np.abs(res - rho) <= 1e-13), res


# ---------------------------------------------------------------------------------------------------------------------------------
# the host layer on gloo ranks over the CPU stand-in
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim_lib():
    subprocess.check_call(["make", "-C", SHIM_LSTSQ, "-s"])
    return os.path.join(SHIM_LSTSQ, "libcapital_driver_cpu_lstsq.so")


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
        procs.append(subprocess.Popen([sys.executable, os.path.join(SHIM_LSTSQ, "lstsq_rank_main.py"), json.dumps(cfg)], env=env,
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


@pytest.mark.parametrize("m,n,r,kappa,sweeps,shifted,rho,serialize", [(4096, 32, 3, 1e4, 2, 0, 1.0, True), (4096, 48, 40, 1e10, 3, 1, 1e-8, False),
                                                                      (2048, 24, 1, 1e1, 2, 0, 0.0, True)])
def test_least_squares_on_gloo_ranks(shim_lib, m, n, r, kappa, sweeps, shifted, rho, serialize):
    """1, 2 and 4 ranks, rows dealt cyclically: X and the residual norms are bit-identical on every rank, X obeys the rule against the two
    references, the norms match long double within the derived bound, r = 40 goes in two column blocks, and R is untouched"""
    cfg = {"m": m, "n": n, "r": r, "kappa": kappa, "sweeps": sweeps, "shifted": shifted, "rho": rho, "serialize": serialize}
    A, B, x_true = lc.problem(m, n, r, kappa, rho)
    eta_h, eta_s = lc.reference_etas(A, B, x_true, sweeps, shifted)
    for world in (1, 2, 4):
        with tempfile.TemporaryDirectory() as d:
            z = _launch(world, dict(cfg, dir=d))
            assert all(str(zz["raised"]) == "" and str(zz["factor_raised"]) == "" for zz in z), [str(zz["raised"]) for zz in z]
            for zz in z[1:]:
                np.testing.assert_array_equal(zz["X"], z[0]["X"])
                np.testing.assert_array_equal(zz["res"], z[0]["res"])
            for zz in z:
                np.testing.assert_array_equal(zz["R_after"], zz["R"])
            X, res = z[0]["X"], z[0]["res"]
        assert X.shape == (n, r) and res.shape == (r,)
        assert lc.eta(X, x_true) <= lc.CB * max(eta_h, eta_s, U64), (world, lc.eta(X, x_true), eta_h, eta_s)
        err, bound = lc.residual_check(A, B, X, res)
        assert np.all(err <= bound), (world, err, bound)


def test_residual_pass_is_optional(shim_lib):
    with tempfile.TemporaryDirectory() as d:
        z = _launch(2, {"m": 1024, "n": 16, "r": 2, "kappa": 1e2, "sweeps": 2, "shifted": 0, "rho": 0.5, "serialize": True, "residual": False, "dir": d})
    assert all(str(zz["raised"]) == "" and zz["res"].size == 0 and zz["X"].shape == (16, 2) for zz in z)


def test_refused_before_factor_after_a_failed_factor_and_on_a_cube(shim_lib):
    with tempfile.TemporaryDirectory() as d:
        z = _launch(2, {"m": 1024, "n": 16, "r": 2, "kappa": 1e2, "sweeps": 2, "shifted": 0, "rho": 0.0, "serialize": True, "factor": False, "dir": d})
        assert all("factor() has not run" in str(zz["raised"]) for zz in z), [str(zz["raised"]) for zz in z]
    with tempfile.TemporaryDirectory() as d:
        z = _launch(2, {"m": 2048, "n": 32, "r": 2, "kappa": 1e12, "sweeps": 2, "shifted": 0, "rho": 0.0, "serialize": True, "dir": d})
        assert all("not positive definite" in str(zz["factor_raised"]) and "did not succeed" in str(zz["raised"]) for zz in z), [str(zz["raised"]) for zz in z]
    for world in (4, 8):                                        # c = 2 (2 x 1 x 2 and 2 x 2 x 2): refused on every rank, before any collective
        with tempfile.TemporaryDirectory() as d:
            z = _launch(world, {"m": 512, "n": 32, "r": 2, "c": 2, "sweeps": 2, "shifted": 0, "serialize": False, "dir": d})
            assert all("least_squares is built for the 1-D variant (c == 1) only" in str(zz["raised"]) for zz in z), [str(zz["raised"]) for zz in z]


def test_c_abi_without_the_entry_points_refuses_the_solve(shim_lib):
    """the host layer holds the two kernels as weak references: on the unextended stand-in of tests/cpu_shim the library still loads,
    factor() runs, and least_squares raises the documented error instead of calling through a null pointer"""
    subprocess.check_call(["make", "-C", SHIM, "-s"])
    with tempfile.TemporaryDirectory() as d:
        z = _launch(1, {"m": 2048, "n": 16, "r": 2, "kappa": 1e2, "sweeps": 2, "shifted": 0, "rho": 0.0, "serialize": True, "dir": d},
                    extra_env={"CAPITAL_SHIM_LIB": os.path.join(SHIM, "libcapital_driver_cpu.so")})
    assert str(z[0]["factor_raised"]) == "" and z[0]["R"].shape == (16, 16)
    assert "no least-squares solve" in str(z[0]["raised"]), str(z[0]["raised"])
