"""qr::cacqr::factor_pivoted through driver.Cacqr on one GPU, and on two ranks of one GPU over the loopback transport: A P = Q R for tall panels
whose columns are linearly dependent, the rank from a pivoted Cholesky of the Gram matrix on the device (capi_dpstrf), and the basic least-squares
solution on the factors.

The panels are tests/_pcqr_cases.py's, of planted rank.  Per metric the rule is DESIGN.md section 2a's: gpu <= 10 max(ref, u), ref the LARGER of two
fp64 references on the same data -- scipy.linalg.qr(pivoting=True) truncated at the rank, and the numpy restatement of the whole path
(tests/_pcqr_ref.py) -- and on top the caps residual <= 2e-13 and orthogonality <= 5e-14 (10 x the restatement's worst values on these inputs,
1.9e-14 and 5.0e-15).  The residual of the least-squares solution is compared with numpy.linalg.lstsq's at rcond = sqrt(tol).  The GPU is never
compared with itself."""
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest
import scipy.linalg as sla

import _pcqr_cases as pc
import _pcqr_ref as pref
import _scqr_ref as ref
from _scqr_ref import U64

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LOOPBACK = os.path.join(HERE, "rccl_loopback", "librccl_loopback.so")
CAP_RESIDUAL, CAP_ORTHOGONALITY = 2e-13, 5e-14


@pytest.fixture(scope="module")
def drv():
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    yield driver
    driver.finalize()


def check(tag, m, n, k, rank, piv, Q, R, X, resnorms):
    """the single-rank rule on a gathered result"""
    A, B = pc.matrix(m, n, k), pc.rhs(m, n, k)
    r = pc.restatement(m, n, k)
    assert rank == k
    assert sorted(piv.tolist()) == list(range(n))
    assert Q.shape == (m, k) and R.shape == (k, n)
    assert np.all(np.tril(R[:, :k], -1) == 0.0)
    res, orth = pref.metrics(A, Q, R, piv)
    res_q, orth_q = pc.qrcp_metrics(m, n, k, k)
    print(f"pcqr {tag}: rank {rank}; residual gpu {res:.3e}, QRCP {res_q:.3e}, restatement {r['residual']:.3e}; "
          f"orthogonality gpu {orth:.3e}, QRCP {orth_q:.3e}, restatement {r['orthogonality']:.3e}")
    assert res <= 10.0 * max(res_q, r["residual"], U64) and res <= CAP_RESIDUAL
    assert orth <= 10.0 * max(orth_q, r["orthogonality"], U64) and orth <= CAP_ORTHOGONALITY
    mine = np.linalg.norm(A @ X - B, axis=0)
    ratio = mine / pc.lstsq_reference(m, n, k)
    print(f"pcqr {tag}: least-squares residual over numpy.linalg.lstsq's, minus 1: {np.array2string(ratio - 1.0, precision=2)}")
    assert np.all(ratio <= 1.0 + 1e-8)
    np.testing.assert_allclose(resnorms, mine, rtol=1e-9)
    dropped = np.setdiff1d(np.arange(n), piv[:k])
    assert dropped.size == n - k and np.all(X[dropped] == 0.0)


@pytest.mark.parametrize("m,n,k", pc.CASES, ids=pc.IDS)
def test_against_two_references(drv, m, n, k):
    q = drv.Cacqr(m, n, c=1, variant=2)
    try:
        q.set_A(pc.matrix(m, n, k))
        rank = q.factor_pivoted()
        assert q.rank == rank
        piv, Q, R = q.piv, q.Q_pivoted(), q.R_pivoted()
        full = q._get(4, (n, n))
        X, resnorms = q.lstsq(pc.rhs(m, n, k))
    finally:
        q.close()
    assert np.all(full[rank:] == 0.0)                                           # rows >= rank of Rp are zero
    check(f"{m}x{n}", m, n, k, rank, piv, Q, R, X, resnorms)


def test_user_tolerance(drv):
    """rtol = 1e-3 on a panel of kappa 1e6: a truncated pivoted QR"""
    m, n = 8320, 130
    A = ref.panel(m, n, 1e6, 5)
    o = pref.pcqr(A, rtol=1e-3)
    q = drv.Cacqr(m, n, c=1, variant=2)
    try:
        q.set_A(A)
        rank = q.factor_pivoted(rtol=1e-3)
        piv, Q, R = q.piv, q.Q_pivoted(), q.R_pivoted()
    finally:
        q.close()
    res, orth = pref.metrics(A, Q, R, piv)
    Qs, Rs, Ps = sla.qr(A, mode="economic", pivoting=True)
    res_q, _ = pref.metrics(A, Qs[:, :rank], Rs[:rank], Ps)
    bound = np.sqrt((n - rank) * o["tol"]) * np.sqrt(o["trace"]) / np.linalg.norm(A)
    print(f"pcqr rtol 1e-3: rank gpu {rank}, restatement {o['rank']}; residual gpu {res:.3e}, QRCP at that rank {res_q:.3e}, bound {bound:.3e}; orthogonality {orth:.3e}")
    assert abs(rank - o["rank"]) <= 1
    assert res <= 1.5 * res_q and res <= 1.01 * bound
    assert orth <= CAP_ORTHOGONALITY


def test_plain_factor_is_untouched_by_a_pivoted_one(drv):
    """factor() then lstsq on a full-rank panel gives the same bits before and after a factor_pivoted on the same object; svd() after
    factor_pivoted raises, and works again after factor()"""
    m, n, k = 4160, 65, 64
    A, B = pc.matrix(m, n, k), pc.rhs(m, n, k)
    q = drv.Cacqr(m, n, c=1, variant=2)
    try:
        q.set_A(A)
        q.factor()
        before = (q.Q(), q.R()) + q.lstsq(B)
        assert q.factor_pivoted() == k
        with pytest.raises(drv.DriverError, match="factor_pivoted"):
            q.svd()
        with pytest.raises(drv.DriverError, match="factor_pivoted"):        # factor()'s square R and its validators do not describe these factors
            q.R()
        with pytest.raises(drv.DriverError, match="factor_pivoted"):
            q.residual()
        q.lstsq(B)
        q.factor()
        after = (q.Q(), q.R()) + q.lstsq(B)
        q.svd(left=False)
    finally:
        q.close()
    for a, b in zip(after, before):
        np.testing.assert_array_equal(a, b)


def test_plain_factor_still_refuses_a_rank_deficient_panel(drv):
    m, n, k = 4160, 65, 40
    q = drv.Cacqr(m, n, c=1, variant=2)
    try:
        q.set_A(pc.matrix(m, n, k))
        with pytest.raises(drv.DriverError, match="numerically rank deficient for CholeskyQR"):
            q.factor()
        with pytest.raises(drv.DriverError, match="factor\\(\\) has not run or did not succeed"):
            q.lstsq(pc.rhs(m, n, k))
        assert q.factor_pivoted() == k                                          # and the pivoted path takes it from there
    finally:
        q.close()


def test_a_zero_panel_has_no_rank(drv):
    q = drv.Cacqr(2048, 32, c=1, variant=2)
    try:
        q.set_A(np.zeros((2048, 32)))
        with pytest.raises(drv.DriverError, match="numerical rank 0"):
            q.factor_pivoted()
        assert q.rank == 0
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
        procs.append(subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "_gpu_pcqr_rank_main.py"), json.dumps(cfg)], env=env,
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


@pytest.mark.parametrize("mode", ["host", "async"])
def test_on_two_ranks_of_one_gpu(mode):
    """rank, piv, R and X bit-identical on both ranks (the all-reduced Gram matrix is, and capi_dpstrf is deterministic: the ranks agree on the
    permutation without communication), and the gathered factors within the single-rank rule"""
    subprocess.check_call(["make", "-C", os.path.dirname(LOOPBACK), "-s"])
    world = 2
    cases = [{"tag": f"pcqr{n}", "m": m, "n": n, "k": k} for m, n, k in ((4160, 65, 40), (2048, 32, 32))]
    with tempfile.TemporaryDirectory() as d:
        _launch(world, {"dir": d, "cases": cases}, mode)
        z = {c["tag"]: [dict(np.load(os.path.join(d, f"{c['tag']}_rank{r}.npz"))) for r in range(world)] for c in cases}
    for c in cases:
        a, b = z[c["tag"]]
        for name in ("rank", "piv", "R", "X", "res"):
            np.testing.assert_array_equal(b[name], a[name], err_msg=name)
        m, n, k = c["m"], c["n"], c["k"]
        Q = np.empty((m, int(a["rank"])), order="F")
        for r in range(world):
            Q[r::world] = z[c["tag"]][r]["Q"]
        check(f"on {world} ranks ({mode}) {m}x{n}", m, n, k, int(a["rank"]), a["piv"], Q, a["R"], a["X"], a["res"])
