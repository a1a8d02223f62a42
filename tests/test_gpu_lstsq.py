"""qr::cacqr::least_squares through driver.Cacqr.lstsq on one GPU, and on 2 and 4 ranks of one GPU over the loopback transport:
X = R^-1 (Q^T B) on the resident CholeskyQR factors, with the residual norms.

The rule is DESIGN.md section 2a's: eta_gpu <= 10 max(eta_ref, u), eta(X) = max_j ||x_j - x_true_j|| / ||x_true_j|| on problems with a planted
solution (tests/_lstsq_cases.py), eta_ref the LARGER of two fp64 references on the same data -- Householder QR + triangular solve and the
numpy restatement of the sweeps + triangular solve.  The GPU is never compared with itself."""
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

import _lstsq_cases as lc
import _scqr_ref as ref
from _scqr_ref import U64

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LOOPBACK = os.path.join(HERE, "rccl_loopback", "librccl_loopback.so")


@pytest.fixture(scope="module")
def drv():
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    yield driver
    driver.finalize()


@pytest.mark.parametrize("m,n,r,kappa,sweeps,shifted,rho", lc.CASES, ids=lc.IDS)
def test_lstsq_against_two_references(drv, m, n, r, kappa, sweeps, shifted, rho):
    A, B, x_true = lc.problem(m, n, r, kappa, rho)
    q = drv.Cacqr(m, n, c=1, variant=sweeps, shifted=shifted)
    try:
        q.set_A(A)
        q.factor()
        before = (q.A(), q.Q(), q.R())
        X, res = q.lstsq(B)
        X2, res2 = q.lstsq(B)
        Xn, none = q.lstsq(B, residual=False)
        after = (q.A(), q.Q(), q.R())
    finally:
        q.close()
    eta_h, eta_s = lc.reference_etas(A, B, x_true, sweeps, shifted)
    eta_g = lc.eta(X, x_true)
    err, bound = lc.residual_check(A, B, X, res)
    print(f"lstsq {m}x{n} r={r} kappa={kappa:.0e} {sweeps}/{shifted} rho={rho:g}: eta gpu {eta_g:.3e}, Householder {eta_h:.3e}, numpy sweeps {eta_s:.3e}; "
          f"resnorm max {res.max():.3e}, max |resnorm - long double| / bound {np.max(err / bound):.3e}")
    assert eta_g <= lc.CB * max(eta_h, eta_s, U64), (eta_g, eta_h, eta_s)
    assert np.all(err <= bound), (err, bound)
    np.testing.assert_array_equal(X2, X)                                    # bit-identical from run to run
    np.testing.assert_array_equal(res2, res)
    np.testing.assert_array_equal(Xn, X)
    assert none is None
    for b, a in zip(before, after):                                         # the solve overwrites nothing of the factorization
        np.testing.assert_array_equal(a, b)


def test_lstsq_refuses_without_valid_factors(drv):
    """before factor() and after a factor() that raised (kappa 1e12 with two plain sweeps): DriverError.  (A grid with c > 1 needs at least four
    ranks; that refusal, with its text, is checked on 4 and 8 ranks in tests/test_lstsq_host.py.)"""
    m, n = 1 << 14, 256
    A, B, _ = lc.problem(m, n, 2, 1e12, 0.0)
    q = drv.Cacqr(m, n, c=1, variant=2)
    try:
        q.set_A(A)
        with pytest.raises(drv.DriverError, match="factor\\(\\) has not run"):
            q.lstsq(B)
        with pytest.raises(drv.DriverError, match="not positive definite"):
            q.factor()
        with pytest.raises(drv.DriverError, match="factor\\(\\) has not run or did not succeed"):
            q.lstsq(B)
    finally:
        q.close()


def test_vector_right_hand_side_and_wrong_shape(drv):
    m, n = 8192, 64
    A, B, x_true = lc.problem(m, n, 1, 1e2, 0.0)
    q = drv.Cacqr(m, n, c=1, variant=2)
    try:
        q.set_A(A)
        q.factor()
        X, res = q.lstsq(B[:, 0])
        assert X.shape == (n, 1) and res.shape == (1,)
        assert lc.eta(X, x_true) <= lc.CB * max(*lc.reference_etas(A, B, x_true, 2, 0), U64)
        with pytest.raises(AssertionError):
            q.lstsq(B[:-1])
    finally:
        q.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2 and 4 ranks of one GPU over the loopback transport, both of its modes
# ---------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(world, cfg, mode, timeout=300):
    """at most 4 GPU processes under ONE deadline for the whole launch; a failed launch ends the case"""
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), GLOO_SOCKET_IFNAME="lo",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", CAPI_RCCL_LIB=LOOPBACK, CAPI_LOOPBACK_MODE=mode, CAPITAL_TEST_GLOO_TIMEOUT_S="120")
        env.setdefault("CAPI_LOOPBACK_TIMEOUT_S", "90")
        procs.append(subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "_gpu_lstsq_rank_main.py"), json.dumps(cfg)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs, timed_out = [], False
    deadline = time.monotonic() + timeout
    try:
        for p in procs:
            outs.append(p.communicate(timeout=max(0.1, deadline - time.monotonic()))[0] or "")
    except subprocess.TimeoutExpired:
        timed_out = True
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    if timed_out:
        outs = [p.communicate()[0] or "" for p in procs]
    assert not timed_out and all(p.returncode == 0 for p in procs), "\n".join(o[-3000:] for o in outs)


@pytest.mark.parametrize("world,mode", [(2, "host"), (4, "host"), (2, "async"), (4, "async")], ids=["loopback2", "loopback4", "loopback2_async", "loopback4_async"])
def test_lstsq_on_ranks_of_one_gpu(world, mode):
    """X bit-identical on all ranks, and within the rule of x_true (the row split changes the summation order, so X is not
    bit-identical to one rank's); the residual norms are global: the same on every rank, and within the derived bound of long double"""
    subprocess.check_call(["make", "-C", os.path.dirname(LOOPBACK), "-s"])
    cases = [{"tag": "cqr2", "m": 1 << 14, "n": 256, "r": 4, "kappa": 1e4, "sweeps": 2, "shifted": 0, "rho": 1.0, "serialize": True},
             {"tag": "scqr3", "m": 1 << 14, "n": 256, "r": 40, "kappa": 1e10, "sweeps": 3, "shifted": 1, "rho": 1e-8, "serialize": False}]
    with tempfile.TemporaryDirectory() as d:
        _launch(world, {"dir": d, "cases": cases}, mode)
        for case in cases:
            z = [np.load(os.path.join(d, f"{case['tag']}_rank{r}.npz")) for r in range(world)]
            A, B, x_true = lc.problem(case["m"], case["n"], case["r"], case["kappa"], case["rho"])
            for zz in z[1:]:
                np.testing.assert_array_equal(zz["X"], z[0]["X"])
                np.testing.assert_array_equal(zz["res"], z[0]["res"])
            eta_h, eta_s = lc.reference_etas(A, B, x_true, case["sweeps"], case["shifted"])
            eta_g = lc.eta(z[0]["X"], x_true)
            err, bound = lc.residual_check(A, B, z[0]["X"], z[0]["res"])
            print(f"lstsq on {world} ranks ({mode}) {case['tag']}: eta gpu {eta_g:.3e}, Householder {eta_h:.3e}, numpy sweeps {eta_s:.3e}")
            assert eta_g <= lc.CB * max(eta_h, eta_s, U64), (eta_g, eta_h, eta_s)
            assert np.all(err <= bound), (err, bound)

