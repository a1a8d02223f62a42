"""GPU parity: LAPACK-level C-ABI (capi_dpotrf / capi_dtrtri / capi_dpotrf_trtri) against the oracle's
restatement of LAPACKE_dpotrf/dtrtri (reference src/lapack/interface.hpp:30-58) on the reference's own SPD
generator (structure.hpp:68-103).  Tolerance 1e-12 relative elementwise (SURVEY.md 8c ii)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 17, 64, 65, 128, 200, 513, 1000, 1280, 1600, 2048, 3000]   # 1280 / 1600: aggregated base cases of the 2- and 4-GPU bench grids


def _spd(oracle, n):
    return oracle.distribute_symmetric(n, n, 0, 0, 1, 1)


@pytest.mark.parametrize("n", SIZES)
def test_potrf_trtri_fused(hip, oracle, n):
    from capital_amd import capi
    A = _spd(oracle, n)
    Rref = A.copy(order="F")
    assert oracle.dpotrf(1, Rref) == 0
    Rref = np.triu(Rref)
    Xref = Rref.copy(order="F")
    assert oracle.dtrtri(1, 0, Xref) == 0
    dA, dX = capi.to_device(A), capi.to_device(np.full((n, n), np.nan))
    hip.call("capi_reset_info")
    hip.call("capi_dpotrf_trtri", n, capi.ptr(dA), n, capi.ptr(dX), n)
    assert hip.info() == 0
    R, X = capi.to_host(dA), capi.to_host(dX)
    assert np.abs(R - Rref).max() <= 1e-12 * np.abs(Rref).max()
    assert np.abs(X - np.triu(Xref)).max() <= 1e-12 * np.abs(Xref).max()
    assert np.all(np.tril(R, -1) == 0) and np.all(np.tril(X, -1) == 0)     # cyclic_to_local zeroing, util.hpp:131-164


@pytest.mark.parametrize("uplo", (0, 1))
@pytest.mark.parametrize("n", [5, 64, 300, 1500])
def test_potrf(hip, oracle, uplo, n):
    from capital_amd import capi
    A = _spd(oracle, n)
    ref = A.copy(order="F")
    assert oracle.dpotrf(uplo, ref) == 0
    junk = A.copy(order="F")
    dA = capi.to_device(junk)
    hip.call("capi_reset_info")
    hip.call("capi_dpotrf", uplo, n, capi.ptr(dA), n)
    assert hip.info() == 0
    got = capi.to_host(dA)
    tri = np.triu(np.ones((n, n), bool)) if uplo else np.tril(np.ones((n, n), bool))
    assert np.abs(got[tri] - ref[tri]).max() <= 1e-12 * np.abs(ref[tri]).max()
    np.testing.assert_array_equal(got[~tri], junk[~tri])     # LAPACK leaves the other triangle alone


@pytest.mark.parametrize("uplo,diag", [(1, 0), (1, 1), (0, 0), (0, 1)])
@pytest.mark.parametrize("n", [3, 64, 129, 700])
def test_trtri(hip, oracle, uplo, diag, n):
    from capital_amd import capi
    rng = np.random.default_rng(n + uplo + diag)
    T = np.asfortranarray(rng.uniform(-1, 1, (n, n)) * 0.1 + np.eye(n) * 3)
    ref = T.copy(order="F")
    assert oracle.dtrtri(uplo, diag, ref) == 0
    dT = capi.to_device(T)
    hip.call("capi_dtrtri", uplo, diag, n, capi.ptr(dT), n)
    got = capi.to_host(dT)
    tri = np.triu(np.ones((n, n), bool), 1 if diag else 0) if uplo else np.tril(np.ones((n, n), bool), -1 if diag else 0)
    assert np.abs(got[tri] - ref[tri]).max() <= 1e-12 * max(1.0, np.abs(ref[tri]).max())
    other = ~(np.triu(np.ones((n, n), bool)) if uplo else np.tril(np.ones((n, n), bool)))
    np.testing.assert_array_equal(got[other], T[other])


def test_potrf_reports_non_spd(hip, oracle):
    """The reference drops LAPACK's info (lapack/interface.hpp:39); the C-ABI keeps it on the device."""
    from capital_amd import capi
    n = 150
    A = _spd(oracle, n)
    A[100, 100] = -5.0
    ref = A.copy(order="F")
    info_ref = oracle.dpotrf(1, ref)
    dA, dX = capi.to_device(A), capi.zeros(n, n)
    hip.call("capi_reset_info")
    hip.call("capi_dpotrf_trtri", n, capi.ptr(dA), n, capi.ptr(dX), n)
    assert hip.info() == info_ref == 101
    hip.call("capi_reset_info")
    assert hip.info() == 0


@pytest.mark.parametrize("fn,uplo,n,j,j2", [("capi_dpotrf_trtri", 1, 300, 200, 230),      # second leaf of the blocked routine (j2: same leaf)
                                            ("capi_dpotrf", 1, 1500, 1100, 1400),          # second order-1024 block, inner leaf
                                            ("capi_dpotrf", 0, 1500, 1100, 1400),          # ... through the transpose
                                            ("capi_dpotrf_trtri", 1, 4200, 3000, 3500)])   # the halving recursion: info_base + n1
def test_info_index_beyond_the_first_leaf(hip, oracle, fn, uplo, n, j, j2):
    """A[j, j] = -5 in an SPD matrix: the first leading minor that is not positive definite has order j + 1, which is LAPACK's info
    whatever the blocking -- every leaf, block and recursion level must add its own offset.  A second bad pivot further down must lose."""
    from capital_amd import capi
    A = _spd(oracle, n)
    A[j, j] = -5.0
    A[j2, j2] = -5.0
    hip.call("capi_reset_info")
    assert hip.info() == 0
    dA = capi.to_device(A)
    if fn == "capi_dpotrf_trtri":
        dX = capi.zeros(n, n)
        hip.call(fn, n, capi.ptr(dA), n, capi.ptr(dX), n)
    else:
        hip.call(fn, uplo, n, capi.ptr(dA), n)
    assert hip.info() == j + 1
    if n <= 1500:
        assert oracle.dpotrf(uplo, A.copy(order="F")) == j + 1
    hip.call("capi_reset_info")
    assert hip.info() == 0


def _padded(A, ld, fill):
    """A on top of ld - n rows of `fill`: the device image is column-major with leading dimension ld."""
    n = A.shape[0]
    out = np.full((ld, A.shape[1]), fill, order="F")
    out[:n] = A
    return out


_bits = lambda a: np.ascontiguousarray(a).view(np.int64)


# cholinv.h calls the factor routines on sub-blocks (ld > n): test_potrf_trtri_fused, test_potrf and test_trtri once more with lda = n + 3
# and ldi = n + 5 -- same references and tolerances, and the rows between n and ld stay as they were, bit for bit
@pytest.mark.parametrize("n", [513, 1600])
def test_potrf_trtri_fused_padded_ld(hip, oracle, n):
    from capital_amd import capi
    lda, ldi = n + 3, n + 5
    A = _spd(oracle, n)
    Rref = A.copy(order="F")
    assert oracle.dpotrf(1, Rref) == 0
    Rref = np.triu(Rref)
    Xref = Rref.copy(order="F")
    assert oracle.dtrtri(1, 0, Xref) == 0
    Ap, Xp = _padded(A, lda, 7.25), _padded(np.full((n, n), np.nan), ldi, -3.5)
    dA, dX = capi.to_device(Ap), capi.to_device(Xp)
    hip.call("capi_reset_info")
    hip.call("capi_dpotrf_trtri", n, capi.ptr(dA), lda, capi.ptr(dX), ldi)
    assert hip.info() == 0
    R, X = capi.to_host(dA), capi.to_host(dX)
    assert np.abs(R[:n] - Rref).max() <= 1e-12 * np.abs(Rref).max()
    assert np.abs(X[:n] - np.triu(Xref)).max() <= 1e-12 * np.abs(Xref).max()
    assert np.all(np.tril(R[:n], -1) == 0) and np.all(np.tril(X[:n], -1) == 0)
    assert np.array_equal(_bits(R[n:]), _bits(Ap[n:])) and np.array_equal(_bits(X[n:]), _bits(Xp[n:]))


@pytest.mark.parametrize("uplo", (0, 1))
@pytest.mark.parametrize("n", [513, 1600])
def test_potrf_padded_ld(hip, oracle, uplo, n):
    from capital_amd import capi
    lda = n + 3
    A = _spd(oracle, n)
    ref = A.copy(order="F")
    assert oracle.dpotrf(uplo, ref) == 0
    Ap = _padded(A, lda, 7.25)
    dA = capi.to_device(Ap)
    hip.call("capi_reset_info")
    hip.call("capi_dpotrf", uplo, n, capi.ptr(dA), lda)
    assert hip.info() == 0
    got = capi.to_host(dA)
    tri = np.triu(np.ones((n, n), bool)) if uplo else np.tril(np.ones((n, n), bool))
    assert np.abs(got[:n][tri] - ref[tri]).max() <= 1e-12 * np.abs(ref[tri]).max()
    assert np.array_equal(_bits(got[:n][~tri]), _bits(A[~tri]))     # LAPACK leaves the other triangle alone
    assert np.array_equal(_bits(got[n:]), _bits(Ap[n:]))


@pytest.mark.parametrize("uplo,diag", [(1, 0), (0, 1)])
@pytest.mark.parametrize("n", [513, 1600])
def test_trtri_padded_ld(hip, oracle, uplo, diag, n):
    from capital_amd import capi
    lda = n + 3
    rng = np.random.default_rng(n + uplo + diag)
    T = np.asfortranarray(rng.uniform(-1, 1, (n, n)) * 0.1 + np.eye(n) * 3)
    ref = T.copy(order="F")
    assert oracle.dtrtri(uplo, diag, ref) == 0
    Tp = _padded(T, lda, 7.25)
    dT = capi.to_device(Tp)
    hip.call("capi_dtrtri", uplo, diag, n, capi.ptr(dT), lda)
    hip.sync()
    got = capi.to_host(dT)
    tri = np.triu(np.ones((n, n), bool), 1 if diag else 0) if uplo else np.tril(np.ones((n, n), bool), -1 if diag else 0)
    assert np.abs(got[:n][tri] - ref[tri]).max() <= 1e-12 * max(1.0, np.abs(ref[tri]).max())
    other = ~(np.triu(np.ones((n, n), bool)) if uplo else np.tril(np.ones((n, n), bool)))
    assert np.array_equal(_bits(got[:n][other]), _bits(T[other]))
    assert np.array_equal(_bits(got[n:]), _bits(Tp[n:]))


@pytest.mark.gpu
@pytest.mark.parametrize("m,n", [(64, 64), (100, 37), (300, 96), (1000, 130), (33, 70)])
def test_geqrf_matches_oracle(hip, oracle, m, n):
    """capi_dgeqrf (lapack::engine::_geqrf, lapack/interface.hpp:60-73) against the oracle's unblocked dgeqr2: same
    reflector convention (beta = -sign(alpha) ||x||), so R, the stored reflectors and tau agree elementwise; 1e-12."""
    import torch
    from capital_amd import capi
    rng = np.random.default_rng(m * 1000 + n)
    A = np.asfortranarray(rng.random((m, n)) - 0.5)
    ref = A.copy(order="F")
    tau_ref = oracle.dgeqrf(ref)
    dA = capi.to_device(A)
    dtau = torch.zeros(min(m, n), dtype=torch.float64, device="cuda")
    hip.call("capi_dgeqrf", m, n, capi.ptr(dA), m, capi.ptr(dtau))
    hip.sync()
    out = capi.to_host(dA)
    scale = np.abs(ref).max()
    assert np.abs(out - ref).max() <= 1e-12 * scale
    assert np.abs(dtau.cpu().numpy() - tau_ref).max() <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("m,n", [(96, 96), (500, 64), (4096, 200), (100000, 96)])
def test_geqrf_orgqr_properties(hip, oracle, m, n):
    """Q = capi_dorgqr(capi_dgeqrf(A)): Q^T Q = I (1e-13), Q R = A (1e-13 relative), R upper triangular; for the small
    shapes also elementwise against the oracle's dorg2r (1e-12).  An ill-conditioned input (kappa ~ 1e12, where
    CholeskyQR2 breaks down) is included: Householder QR does not care."""
    import torch
    from capital_amd import capi
    rng = np.random.default_rng(m + n)
    A = np.asfortranarray(rng.random((m, n)) - 0.5)
    if m == 4096:                                              # graded column scaling: condition number ~ 1e12
        A *= np.logspace(0, -12, n)[None, :]
        A = np.asfortranarray(A)
    dA = capi.to_device(A)
    dtau = torch.zeros(n, dtype=torch.float64, device="cuda")
    hip.call("capi_dgeqrf", m, n, capi.ptr(dA), m, capi.ptr(dtau))
    hip.sync()
    fac = capi.to_host(dA)
    R = np.triu(fac[:n, :])
    hip.call("capi_dorgqr", m, n, n, capi.ptr(dA), m, capi.ptr(dtau))
    hip.sync()
    Q = capi.to_host(dA)
    assert np.abs(Q.T @ Q - np.eye(n)).max() <= 1e-13
    assert np.abs(Q @ R - A).max() <= 1e-13 * np.abs(A).max() * n
    if m <= 500:
        ref = fac.copy(order="F")
        oracle.dorgqr(ref, dtau.cpu().numpy())
        assert np.abs(Q - ref).max() <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("m,n", [(8192, 64), (20011, 96), (30000, 192), (16384, 256)])
def test_geqrf_tall_reconstruction_matches_oracle(hip, oracle, m, n):
    """Tall panels (m >= 64 n) take CholeskyQR2 + Householder reconstruction (csrc/qr_f64.hip: Q - [S; 0] = Y U): the output is
    still LAPACK's -- R, the stored reflectors and tau agree elementwise with the oracle's column-by-column dgeqr2 (1e-12),
    and dorgqr on it gives back an orthonormal Q with Q R = A."""
    import torch
    from capital_amd import capi
    rng = np.random.default_rng(m + 7 * n)
    A = np.asfortranarray(rng.random((m, n)) - 0.5)
    ref = A.copy(order="F")
    tau_ref = oracle.dgeqrf(ref)
    dA = capi.to_device(A)
    dtau = torch.zeros(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    hip.call("capi_dgeqrf", m, n, capi.ptr(dA), m, capi.ptr(dtau))
    hip.sync()
    out = capi.to_host(dA)
    assert np.abs(np.triu(out[:n]) - np.triu(ref[:n])).max() <= 1e-12 * np.abs(np.triu(ref[:n])).max()     # R
    assert np.abs(np.tril(out, -1) - np.tril(ref, -1)).max() <= 1e-12                                      # reflectors (entries <= 1)
    assert np.abs(dtau.cpu().numpy() - tau_ref).max() <= 1e-12
    hip.call("capi_dorgqr", m, n, n, capi.ptr(dA), m, capi.ptr(dtau))
    hip.sync()
    Q = capi.to_host(dA)
    assert np.abs(Q.T @ Q - np.eye(n)).max() <= 1e-13
    assert np.abs(Q @ np.triu(out[:n]) - A).max() <= 1e-13 * n


@pytest.mark.gpu
def test_geqrf_tall_ill_conditioned_falls_back(hip, oracle):
    """kappa ~ 1e12 on a tall panel: CholeskyQR2 is not safe (the first sweep's diagonal ratio says so), the Householder panels
    run instead and the factorisation is as good as ever"""
    import torch
    from capital_amd import capi
    m, n = 20000, 64
    rng = np.random.default_rng(5)
    A = np.asfortranarray((rng.random((m, n)) - 0.5) * np.logspace(0, -12, n)[None, :])
    dA = capi.to_device(A)
    dtau = torch.zeros(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    hip.call("capi_dgeqrf", m, n, capi.ptr(dA), m, capi.ptr(dtau))
    hip.sync()
    fac = capi.to_host(dA)
    ref = A.copy(order="F")
    tau_ref = oracle.dgeqrf(ref)
    assert np.abs(dtau.cpu().numpy() - tau_ref).max() <= 1e-12
    R = np.triu(fac[:n])
    hip.call("capi_dorgqr", m, n, n, capi.ptr(dA), m, capi.ptr(dtau))
    hip.sync()
    Q = capi.to_host(dA)
    assert np.abs(Q.T @ Q - np.eye(n)).max() <= 1e-13
    assert np.abs(Q @ R - A).max() <= 1e-13 * np.abs(A).max() * n


@pytest.mark.gpu
def test_diagonal_block_routine_replayed_from_a_graph():
    """CAPI_GRAPH: the blocked diagonal-block routine captured into a hipGraph on its second call for the same block and replayed from
    the third on (factor_f64.hip: capi_dpotrf_trtri).  Off by default -- measured 1 % slower than plain launches --
    but it must stay correct: the probe factors the same blocks eight times and reports the residuals of the LAST (replayed) result."""
    import os, re, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_probe.py")], env=dict(os.environ, CAPI_GRAPH="2"), cwd=root,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = res.stdout + res.stderr
    assert out.count("order 1024 captured") == 1 and out.count("order 1024 replayed") >= 5, out[-2000:]
    vals = re.findall(r"\|R\^T R - S\| ([0-9.e+-]+)  \|Rinv R - I\| ([0-9.e+-]+)", out)
    assert len(vals) == 2
    for a, b in vals:
        assert float(a) <= 1e-14 and float(b) <= 1e-13


@pytest.mark.gpu
def test_geqrf_tall_without_workspace_takes_the_householder_panels(hip, oracle, monkeypatch):
    """The tall-panel routines ask the handle for 2 m n doubles; when that allocation fails (here: CAPI_WS_CAP_MB makes requests above
    8 MiB fail the way an out-of-memory hipMalloc does) geqrf must fall back to the column-by-column panels, which need
    none of it -- not return the allocator's stale error -- and still give LAPACK's factorisation."""
    import torch
    from capital_amd import capi
    m, n = 16384, 64                                              # 2 m n doubles = 16 MiB: above the cap; every other block stays below it
    rng = np.random.default_rng(99)
    A = np.asfortranarray(rng.random((m, n)) - 0.5)
    ref = A.copy(order="F")
    tau_ref = oracle.dgeqrf(ref)
    h2 = capi.Handle(0)                                           # a fresh handle: nothing cached from earlier tests
    dA = capi.to_device(A)
    dtau = torch.zeros(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    monkeypatch.setenv("CAPI_WS_CAP_MB", "8")
    h2.call("capi_dgeqrf", m, n, capi.ptr(dA), m, capi.ptr(dtau))
    h2.sync()
    out = capi.to_host(dA)
    assert np.abs(np.triu(out[:n]) - np.triu(ref[:n])).max() <= 1e-12 * np.abs(np.triu(ref[:n])).max()
    assert np.abs(np.tril(out, -1) - np.tril(ref, -1)).max() <= 1e-12
    assert np.abs(dtau.cpu().numpy() - tau_ref).max() <= 1e-12
    # (orgqr's one-block path asks for LESS than the panels behind it need at this shape -- 8.5 against 13.6 MB -- so no cap separates
    #  them: its fallback cannot be reached by a failing allocation that the slow path would survive)
    monkeypatch.delenv("CAPI_WS_CAP_MB")
    h2.call("capi_dorgqr", m, n, n, capi.ptr(dA), m, capi.ptr(dtau))
    h2.sync()
    Q = capi.to_host(dA)
    assert np.abs(Q.T @ Q - np.eye(n)).max() <= 1e-13
    assert np.abs(Q @ np.triu(out[:n]) - A).max() <= 1e-13 * n
