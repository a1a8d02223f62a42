"""qr::cacqr::svd through driver.Cacqr.svd on one GPU, and on two ranks of one GPU over the loopback transport: A = (Q U_R) Sigma V^T from the
resident CholeskyQR factors, R = U_R Sigma V^T by capi_dgesvj on the device.

The panels are _scqr_ref.panel's, whose singular values are planted (log-spaced 1 .. 1 / kappa).  Per metric the rule is DESIGN.md section 2a's:
gpu <= 10 max(ref, u), ref the LARGER of two fp64 references on the same data -- numpy.linalg.svd(A) and the numpy restatement of the whole path
(_scqr_ref.scqr, then _jacobi_ref) -- and the caps of tests/test_gpu_gesvj.py on top.  The GPU is never compared with itself."""
import functools
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

import _jacobi_ref as jr
import _scqr_ref as ref
from _scqr_ref import U64

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LOOPBACK = os.path.join(HERE, "rccl_loopback", "librccl_loopback.so")
CASES = [(8192, 64, 1e2, 2, 0), (8192, 130, 1e4, 2, 0), (16384, 256, 1e7, 2, 0), (16384, 256, 1e10, 3, 1), (16384, 256, 1e12, 4, 2)]
IDS = [f"{m}x{n}-k{k:.0e}-{sw}of{sh}" for m, n, k, sw, sh in CASES]
NAMES = ("sigma", "residual", "orthogonality of U", "orthogonality of V")
CAPS = (1e-12, 1e-12, 2e-11, 2e-11)


def metrics(A, U, s, V, planted):
    res, ou, ov, sig = jr.metrics(A, U, s, V, planted)
    return sig, res, ou, ov


@functools.lru_cache(maxsize=None)
def problem(m, n, kappa, sweeps, shifted):
    """(A, planted sigma, metrics of numpy.linalg.svd(A), metrics of the numpy restatement), computed once and shared"""
    A = ref.panel(m, n, kappa, 0)
    planted = np.logspace(0, -np.log10(kappa), n)
    Un, sn, Vtn = np.linalg.svd(A, full_matrices=False)
    Q, R, _ = ref.scqr(A, sweeps, shifted)
    Uj, sj, Vj, sw = jr.jacobi_svd(R)
    assert 1 <= sw <= jr.MAX_SWEEPS
    for a in (A, planted):
        a.setflags(write=False)
    return A, planted, metrics(A, Un, sn, Vtn.T, planted), metrics(A, Q @ Uj, sj, Vj, planted)


def check(tag, A, U, s, V, planted, m_np, m_jr):
    m_gpu = metrics(A, U, s, V, planted)
    for name, g, a, b in zip(NAMES, m_gpu, m_np, m_jr):
        print(f"svd {tag} {name}: gpu {g:.3e}, numpy.linalg.svd {a:.3e}, numpy restatement {b:.3e}")
    assert np.all(s >= 0.0) and np.all(np.diff(s) <= 0.0)
    for name, g, a, b, cap in zip(NAMES, m_gpu, m_np, m_jr, CAPS):
        assert g <= 10.0 * max(a, b, U64), (name, g, a, b)
        assert g <= cap, (name, g, cap)


@pytest.fixture(scope="module")
def drv():
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    yield driver
    driver.finalize()


@pytest.mark.parametrize("m,n,kappa,sweeps,shifted", CASES, ids=IDS)
def test_svd_against_two_references(drv, m, n, kappa, sweeps, shifted):
    A, planted, m_np, m_jr = problem(m, n, kappa, sweeps, shifted)
    q = drv.Cacqr(m, n, c=1, variant=sweeps, shifted=shifted)
    try:
        q.set_A(A)
        q.factor()
        before = (q.A(), q.Q(), q.R())
        U, s, V = q.svd()
        jacobi_sweeps = q.svd_sweeps
        U2, s2, V2 = q.svd()
        none, s_v, V_v = q.svd(left=False)
        after = (q.A(), q.Q(), q.R())
    finally:
        q.close()
    print(f"svd {m}x{n} kappa={kappa:.0e} {sweeps}/{shifted}: {jacobi_sweeps} Jacobi sweeps, cond2 {s[0] / s[-1]:.3e}")
    assert 1 <= jacobi_sweeps <= 30
    check(f"{m}x{n} kappa={kappa:.0e}", A, U, s, V, planted, m_np, m_jr)
    for a, b in ((U2, U), (s2, s), (V2, V), (s_v, s), (V_v, V)):            # bit-identical from run to run, and without U
        np.testing.assert_array_equal(a, b)
    assert none is None
    for b, a in zip(before, after):                                         # nothing of the factorization is overwritten
        np.testing.assert_array_equal(a, b)


def test_svd_refuses_without_valid_factors(drv):
    """before factor() and after a factor() that raised (kappa 1e12 with two plain sweeps): DriverError"""
    m, n = 1 << 14, 256
    A = ref.panel(m, n, 1e12, 0)
    q = drv.Cacqr(m, n, c=1, variant=2)
    try:
        q.set_A(A)
        with pytest.raises(drv.DriverError, match="factor\\(\\) has not run"):
            q.svd()
        with pytest.raises(drv.DriverError, match="not positive definite"):
            q.factor()
        with pytest.raises(drv.DriverError, match="factor\\(\\) has not run or did not succeed"):
            q.svd(left=False)
    finally:
        q.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# two ranks of one GPU over the loopback transport
# ---------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(world, cfg, mode, timeout=300):
    """at most 4 GPU processes under ONE deadline for the whole launch; a failed launch ends the case"""
    assert world <= 4
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), GLOO_SOCKET_IFNAME="lo",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", CAPI_RCCL_LIB=LOOPBACK, CAPI_LOOPBACK_MODE=mode, CAPITAL_TEST_GLOO_TIMEOUT_S="120")
        env.setdefault("CAPI_LOOPBACK_TIMEOUT_S", "90")
        procs.append(subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "_gpu_svd_rank_main.py"), json.dumps(cfg)], env=env,
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


def test_svd_on_two_ranks_of_one_gpu():
    """s and V bit-identical on both ranks (R is replicated bit for bit and the device SVD is deterministic: nothing is communicated), and the
    gathered U within the rule (the row split changes the Gram matrix's summation order, so the factors are not bit-identical to one rank's)"""
    subprocess.check_call(["make", "-C", os.path.dirname(LOOPBACK), "-s"])
    world = 2
    m, n, kappa, sweeps, shifted = CASES[2]
    case = {"tag": "cqr2", "m": m, "n": n, "kappa": kappa, "sweeps": sweeps, "shifted": shifted}
    with tempfile.TemporaryDirectory() as d:
        _launch(world, {"dir": d, "cases": [case]}, "host")
        z = [dict(np.load(os.path.join(d, f"{case['tag']}_rank{r}.npz"))) for r in range(world)]
    A, planted, m_np, m_jr = problem(m, n, kappa, sweeps, shifted)
    np.testing.assert_array_equal(z[1]["s"], z[0]["s"])
    np.testing.assert_array_equal(z[1]["V"], z[0]["V"])
    assert int(z[1]["sweeps"]) == int(z[0]["sweeps"])
    U = np.empty((m, n), order="F")
    for r in range(world):
        U[r::world] = z[r]["U"]
    check(f"on {world} ranks", A, U, z[0]["s"], z[0]["V"], planted, m_np, m_jr)
