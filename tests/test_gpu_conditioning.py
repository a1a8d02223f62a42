"""Factorisations on ill-conditioned, graded, exact-factor, indefinite and Kahan-type inputs (tests/_conditioning.py: F1-F5),
held to extended-precision residuals (oracle.ld_*) instead of the fp64 elementwise yardstick of the parity tests -- which, on the
diagonally dominant generator (kappa ~ 1.5), cannot tell an accurate kernel from one that has lost half its digits.

Backward errors follow one rule, with one constant C: eta_gpu <= C max(eta_ref, u), eta_ref the long-double backward error of
the oracle's fp64 run of the same algorithm (LAPACK semantics for the C-ABI routines, the cholinv / CholeskyQR2 schedules for the
driver).  u = 2^-53.  The floor is u, not n u: the measured errors of both runs are a few u at every order here, and a floor of
n u (1e-13 at n = 1000) would let a kernel that lost two digits pass.  Inverse residuals keep the n u of their a-priori bound."""
import numpy as np
import pytest

from _conditioning import (U64, f1_device, f1_spectrum, f2_exponents, f2_graded, f3_exact, f4_factor, f4_indefinite, f5_kahan, kappa_tri)

pytestmark = pytest.mark.gpu

CB = 10.0            # the constant of every bound in this file
KAPPAS = (1e3, 1e8, 1e12)


def _dev(A, ld=None, fill=0.0):
    """A (m x n) on the device, column-major with leading dimension ld (padding rows hold `fill`)"""
    from capital_amd import capi
    m, n = A.shape
    ld = m if ld is None else ld
    P = np.full((ld, n), fill, order="F")
    P[:m] = A
    return capi.to_device(P)


def _host(t, m):
    from capital_amd import capi
    return np.asfortranarray(capi.to_host(t)[:m])


def _potrf_trtri(hip, A, ld=None):
    from capital_amd import capi
    n = A.shape[0]
    ld = n if ld is None else ld
    dA, dX = _dev(A, ld), _dev(np.full((n, n), np.nan), ld)
    hip.call("capi_reset_info")
    hip.call("capi_dpotrf_trtri", n, capi.ptr(dA), ld, capi.ptr(dX), ld)
    info = hip.info()
    return _host(dA, n), _host(dX, n), info


def _potrf(hip, uplo, A, ld=None):
    from capital_amd import capi
    n = A.shape[0]
    ld = n if ld is None else ld
    dA = _dev(A, ld)
    hip.call("capi_reset_info")
    hip.call("capi_dpotrf", uplo, n, capi.ptr(dA), ld)
    info = hip.info()
    return _host(dA, n), info


def _lapack_R(oracle, A):
    R = A.copy(order="F")
    assert oracle.dpotrf(1, R) == 0
    return np.asfortranarray(np.triu(R))


def _eta(oracle, A, R):
    """long-double backward error; the probe form above order 2500 (O(n^2) instead of O(n^3) on the host)"""
    return oracle.ld_cholesky_backward(A, R) if A.shape[0] <= 2500 else oracle.ld_cholesky_probe(A, R, k=4)


def _f1(n, kappa, seed):
    """F1 of order n: numpy up to 2048, above that built on the device -- whose kappa is what the construction reaches, reported
    and held to within a factor of 10 of the target"""
    if n <= 2048:
        return f1_spectrum(n, kappa, seed)
    A, reached = f1_device(n, kappa, seed)
    print(f"F1 on the device, n={n}: kappa target {kappa:.1e}, reached {reached:.2e}")
    assert kappa / 10 <= reached <= kappa * 10, (kappa, reached)
    return A


# ---------------------------------------------------------------------------------------------------------------------------
# pivots: on a diagonal matrix every pivot is one rsqrt -- R_ii = sqrt(a_ii) and X_ii = 1/sqrt(a_ii) within 2 ulp
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 16, 17, 128, 1000])
@pytest.mark.parametrize("routine", ["potrf_trtri", "potrf_U", "potrf_L"])
def test_pivots_are_correctly_rounded(hip, n, routine):
    """The leaf's pivot is v_rsq_f64 plus one third-order correction (error below 2^-66 before rounding): sqrt and 1/sqrt come out
    within 2 ulp of the long-double values.  One Newton step instead leaves ~2^-45, about 100 ulp."""
    rng = np.random.default_rng(n)
    p = np.ldexp(rng.uniform(1.0, 4.0, n), 2 * rng.integers(-40, 41, n))
    A = np.asfortranarray(np.diag(p))
    s = np.sqrt(p.astype(np.longdouble))
    if routine == "potrf_trtri":
        R, X, info = _potrf_trtri(hip, A)
        xd = np.diag(X).astype(np.longdouble)
        assert np.all(np.abs(xd - 1 / s) <= 2 * np.spacing(np.diag(X))), np.max(np.abs(xd - 1 / s) / np.spacing(np.diag(X)))
    else:
        R, info = _potrf(hip, 1 if routine == "potrf_U" else 0, A)
    assert info == 0
    rd = np.diag(R).astype(np.longdouble)
    assert np.all(np.abs(rd - s) <= 2 * np.spacing(np.diag(R))), np.max(np.abs(rd - s) / np.spacing(np.diag(R)))


# ---------------------------------------------------------------------------------------------------------------------------
# backward error, F1 (kappa 1e3 .. 1e12), every schedule of the fused routine and of capi_dpotrf
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kappa", KAPPAS)
@pytest.mark.parametrize("n,pad", [(1, 0), (16, 0), (16, 1), (17, 0), (127, 0), (128, 0), (128, 1), (129, 0), (255, 0), (1000, 0),
                                   (1000, 1), (2048, 0), (4224, 0)])
def test_potrf_trtri_backward_error(hip, oracle, n, pad, kappa):
    """capi_dpotrf_trtri against LAPACK's dpotrf (the oracle) on F1.  R: eta <= C max(eta_ref, u).  X: the halving recursion
    X12 = -X11 R12 X22 is a block form of Higham's method 2 (Accuracy and Stability, section 14.2), whose bound is on the LEFT
    residual: ||X R - I||_F <= C n u || |X||R| ||_F.  (pad 1: an odd leading dimension, the leaf's 8-byte load path.)"""
    A = _f1(n, kappa, n)
    R, X, info = _potrf_trtri(hip, A, n + pad)
    assert info == 0
    assert np.all(np.tril(R, -1) == 0) and np.all(np.tril(X, -1) == 0)
    eta = _eta(oracle, A, R)
    eta_ref = _eta(oracle, A, _lapack_R(oracle, A))
    bound = CB * max(eta_ref, U64)
    print(f"potrf_trtri n={n} pad={pad} kappa={kappa:.0e}: eta {eta:.3e} eta_ref {eta_ref:.3e} ratio {eta / max(eta_ref, U64):.2f}")
    assert eta <= bound, (eta, eta_ref)
    if n <= 2048:
        e, mag = oracle.ld_inverse_residual(X, R, 0)
        print(f"    ||XR - I|| {e:.3e}  n u || |X||R| || {n * U64 * mag:.3e}")
        assert e <= CB * n * U64 * mag, (e, mag)


@pytest.mark.parametrize("kappa", (1e3, 1e12))
@pytest.mark.parametrize("uplo", (1, 0))
@pytest.mark.parametrize("n,pad", [(17, 0), (128, 1), (1000, 0), (2500, 0), (2500, 1)])
def test_potrf_backward_error(hip, oracle, uplo, n, pad, kappa):
    """capi_dpotrf (NB = 1024 blocks; 2500 leaves a ragged last block; uplo L through the transpose) against LAPACK's dpotrf."""
    A = _f1(n, kappa, n + 1)
    F, info = _potrf(hip, uplo, A, n + pad)
    assert info == 0
    R = np.asfortranarray(np.triu(F) if uplo else np.tril(F).T)
    eta = _eta(oracle, A, R)
    eta_ref = _eta(oracle, A, _lapack_R(oracle, A))
    print(f"potrf uplo={uplo} n={n} kappa={kappa:.0e}: eta {eta:.3e} eta_ref {eta_ref:.3e} ratio {eta / max(eta_ref, U64):.2f}")
    assert eta <= CB * max(eta_ref, U64), (eta, eta_ref)


# ---------------------------------------------------------------------------------------------------------------------------
# forward error where the truth is exact
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [17, 128, 1000, 2500])
def test_exact_factor_forward_error(hip, oracle, n):
    """F3: A = R*^T R* exactly, so R* is the Cholesky factor with no rounding in it.  ||R - R*||_F / ||R*||_F <= C n u kappa(R*)
    for the fused routine (n <= 4096: leaf / blocked) and capi_dpotrf U and L -- and, since that bound is loose (kappa_F(R*) is
    about 1e5 here), the backward error by the same-algorithm rule as well: eta <= C max(eta_ref, u)."""
    A, Rs = f3_exact(n, seed=n)
    kap = kappa_tri(Rs)
    bound = CB * n * U64 * kap
    eta_ref = oracle.ld_cholesky_backward(A, _lapack_R(oracle, A))
    outs = {"potrf_L": np.tril(_potrf(hip, 0, A)[0]).T, "potrf_U": np.triu(_potrf(hip, 1, A)[0])}
    if n <= 2048:
        outs["potrf_trtri"] = _potrf_trtri(hip, A)[0]
    for name, R in outs.items():
        err = np.linalg.norm(R - Rs) / np.linalg.norm(Rs)
        eta = oracle.ld_cholesky_backward(A, np.asfortranarray(R))
        print(f"F3 {name} n={n}: forward {err:.3e}  n u kappa {n * U64 * kap:.3e}  eta {eta:.3e} eta_ref {eta_ref:.3e}")
        assert err <= bound, (name, err, bound)
        assert eta <= CB * max(eta_ref, U64), (name, eta, eta_ref)


@pytest.mark.parametrize("scaled", (False, True))
@pytest.mark.parametrize("n", [100, 300])
@pytest.mark.parametrize("uplo,diag", [(1, 0), (1, 1), (0, 0), (0, 1)])
def test_trtri_kahan(hip, oracle, uplo, diag, n, scaled):
    """F5: T = I - (strictly upper ones); X* = T^-1 has entries 2^(j-i-1), 2^0 .. 2^(n-2) in one matrix, known exactly.  Elementwise
    |X - X*| <= C n u (|X*||T||X*|)_ij.  The unit forms get a junk diagonal (7.0): LAPACK's dtrtri does not read it."""
    from capital_amd import capi
    T, Xs = f5_kahan(n, uplo, scale_seed=n if scaled and not diag else None)
    bnd = CB * n * U64 * (np.abs(Xs) @ np.abs(T) @ np.abs(Xs))
    Tin = T.copy(order="F")
    if diag:
        np.fill_diagonal(Tin, 7.0)
    dT = _dev(Tin)
    hip.call("capi_dtrtri", uplo, diag, n, capi.ptr(dT), n)
    X = _host(dT, n)
    tri = np.triu(np.ones((n, n), bool), diag) if uplo else np.tril(np.ones((n, n), bool), -diag)
    err = np.abs(X - Xs)
    assert np.all(err[tri] <= bnd[tri]), np.max(err[tri] / bnd[tri])
    np.testing.assert_array_equal(X[~tri & ~np.eye(n, dtype=bool)], Tin[~tri & ~np.eye(n, dtype=bool)])


def _op_dense(T, uplo, trans, diag):
    E = np.triu(T) if uplo else np.tril(T)
    if diag:
        np.fill_diagonal(E, 1.0)
    return np.asfortranarray(E.T if trans else E)


def _trsm_eta(oracle, side, E, X, alpha, B):
    r, _, nb = oracle.ld_gemm_residual(E, X, alpha, B) if side == 0 else oracle.ld_gemm_residual(X, E, alpha, B)
    return r / (np.linalg.norm(E) * np.linalg.norm(X) + nb)


@pytest.fixture(scope="module")
def trsm_factors():
    """upper triangles of the trsm tests: F5 (order 300, column-scaled) and the Cholesky factor of an F1 matrix at kappa 1e12 (600)"""
    T5, _ = f5_kahan(300, 1, scale_seed=3)
    A = f1_spectrum(600, 1e12, 600)
    import oracle as O
    R = _lapack_R(O, A)
    return {"F5": T5, "F1": R}


@pytest.mark.parametrize("src", ["F5", "F1"])
@pytest.mark.parametrize("side,uplo,trans,diag", [(s, u, t, d) for s in (0, 1) for u in (0, 1) for t in (0, 1) for d in (0, 1)])
def test_trsm_backward_error(hip, oracle, trsm_factors, src, side, uplo, trans, diag):
    """capi_dtrsm in all 16 forms: ||op(T) X - alpha B|| / (||T|| ||X|| + ||alpha B||) <= C max(eta_ref, u), eta_ref the same
    measure of the oracle's dtrsm (LAPACK semantics).  What T must not read -- the other triangle, and the diagonal of the unit
    forms -- holds NaN, then +-1e300, on two more runs: the output is bit-identical to that of the clean triangle."""
    from capital_amd import capi
    Tu = trsm_factors[src]
    nt = Tu.shape[0]
    T = np.asfortranarray(Tu if uplo else Tu.T)
    m, n = (nt, 48) if side == 0 else (48, nt)
    rng = np.random.default_rng(side * 8 + uplo * 4 + trans * 2 + diag)
    B = np.asfortranarray(rng.standard_normal((m, n)))
    alpha = -0.75
    ref = B.copy(order="F")
    oracle.dtrsm(side, uplo, trans, diag, alpha, T, ref)
    outs = []
    other = np.tril(np.ones((nt, nt), bool), -1) if uplo else np.triu(np.ones((nt, nt), bool), 1)
    if diag:
        other |= np.eye(nt, dtype=bool)
    clean = np.where(other, 0.0, T)
    if diag:
        np.fill_diagonal(clean, 1.0)
    for junk in (None, np.full((nt, nt), np.nan), np.where(rng.random((nt, nt)) < 0.5, -1e300, 1e300)):
        Tj = np.asfortranarray(clean if junk is None else np.where(other, junk, T))
        dT, dB = _dev(Tj), _dev(B)
        hip.call("capi_dtrsm", side, uplo, trans, diag, m, n, alpha, capi.ptr(dT), nt, capi.ptr(dB), m)
        outs.append(_host(dB, m))
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], outs[2])
    E = _op_dense(T, uplo, trans, diag)
    eta = _trsm_eta(oracle, side, E, outs[0], alpha, B)
    eta_ref = _trsm_eta(oracle, side, E, ref, alpha, B)
    print(f"trsm {src} side={side} uplo={uplo} trans={trans} diag={diag}: eta {eta:.3e} eta_ref {eta_ref:.3e}")
    assert eta <= CB * max(eta_ref, U64), (eta, eta_ref)


# ---------------------------------------------------------------------------------------------------------------------------
# scale equivariance: bit-identical
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ramp", (False, True))
@pytest.mark.parametrize("n", [16, 17, 129, 1000, 2500])
def test_scale_equivariance_capi(hip, n, ramp):
    """F2: Cholesky is equivariant under power-of-two scaling, R(DBD) = R(B) D, X(DBD) = D^-1 X(B), and every operation on these
    paths (products, FMAs, MFMAs, rsqrt with its polynomial step) is homogeneous with a summation order fixed by the shape: the
    results are bit-identical, not merely close.  capi_dpotrf_trtri, capi_dpotrf U and L."""
    B = f1_spectrum(n, 10.0, 7 * n) if n <= 2048 else _f1(n, 10.0, 7 * n)
    e = f2_exponents(n, seed=n, ramp=ramp)
    A = f2_graded(B, e)
    colD = lambda M: np.ldexp(M, e[None, :])
    rowDi = lambda M: np.ldexp(M, -e[:, None])
    if n <= 2048:
        R0, X0, _ = _potrf_trtri(hip, B)
        R1, X1, info = _potrf_trtri(hip, A)
        assert info == 0
        np.testing.assert_array_equal(R1, colD(R0))
        np.testing.assert_array_equal(X1, rowDi(X0))
    U0, U1 = np.triu(_potrf(hip, 1, B)[0]), np.triu(_potrf(hip, 1, A)[0])
    np.testing.assert_array_equal(U1, colD(U0))
    L0, L1 = np.tril(_potrf(hip, 0, B)[0]), np.tril(_potrf(hip, 0, A)[0])
    np.testing.assert_array_equal(L1, np.ldexp(L0, e[:, None]))


@pytest.fixture(scope="module")
def drv():
    from capital_amd import driver
    driver.init(0, 0, 1, None, use_torch_stream=False)
    yield driver
    driver.finalize()


def _cholinv(drv, A, bc, ci, trsm):
    p = drv.Cholinv(A.shape[0], c=1, complete_inv=ci, split=1, bc_mult=bc, serialize=True, trsm_mode=trsm)
    p.set_A(A)
    p.factor()
    R = p.R()
    Ri = None if trsm else p.Rinv()
    st = p.stats()
    p.close()
    return R, Ri, st


@pytest.mark.parametrize("bc,ci,trsm", [(-1, 0, False), (-3, 1, False), (-2, 0, True)])
def test_scale_equivariance_schedules(drv, bc, ci, trsm):
    """the cholinv schedule (two base-case depths, with and without complete_inv) and TRSM mode on F2: bit-identical"""
    n = 1024
    B = f1_spectrum(n, 10.0, 11)
    e = f2_exponents(n, seed=5)
    R0, X0, _ = _cholinv(drv, B, bc, ci, trsm)
    R1, X1, _ = _cholinv(drv, f2_graded(B, e), bc, ci, trsm)
    np.testing.assert_array_equal(R1, np.ldexp(R0, e[None, :]))
    if not trsm:
        np.testing.assert_array_equal(X1, np.ldexp(X0, -e[:, None]))


@pytest.mark.parametrize("m,n", [(16384, 256), (8192, 130)])
def test_scale_equivariance_cacqr2(drv, oracle, m, n):
    """CholeskyQR2 through Cacqr.set_A on a column-graded panel: R(A D) = R(A) D and Q(A D) = Q(A), bit for bit"""
    A = oracle.distribute_random(n, m, 0, 0, 1, 1, key=3)
    e = f2_exponents(n, seed=n, lo=-100, hi=100)
    out = []
    for M in (A, np.ldexp(A, e[None, :])):
        q = drv.Cacqr(m, n, c=1, variant=2)
        q.set_A(np.asfortranarray(M))
        q.factor()
        out.append((q.Q(), q.R()))
        q.close()
    np.testing.assert_array_equal(out[1][0], out[0][0])
    np.testing.assert_array_equal(out[1][1], np.ldexp(out[0][1], e[None, :]))


# ---------------------------------------------------------------------------------------------------------------------------
# the triangle a routine must not read
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,pad", [(16, 0), (17, 0), (128, 1), (1000, 0), (2500, 1)])
def test_unread_triangle(hip, n, pad):
    """NaN, and separately +-1e300, in the triangle the header says is not read: capi_dpotrf_trtri and capi_dpotrf(U) read the upper
    triangle, capi_dpotrf(L) the lower, capi_dtrtri(U) the upper.  Outputs are bit-identical to those of a clean input, and
    capi_dpotrf / capi_dtrtri leave the other triangle as it was (LAPACK)."""
    from capital_amd import capi
    ld = n + pad
    A = f1_spectrum(n, 1e6, 3 * n) if n <= 2048 else _f1(n, 1e6, 3 * n)
    up = np.triu(np.ones((n, n), bool))
    lo_strict = ~up
    up_strict = ~np.tril(np.ones((n, n), bool))
    rng = np.random.default_rng(n)
    junks = (np.full((n, n), np.nan), np.where(rng.random((n, n)) < 0.5, -1e300, 1e300))

    def with_junk(M, where, J):
        M = M.copy(order="F")
        M[where] = J[where]
        return M

    cleanU, _ = _potrf(hip, 1, A, ld)
    cleanL, _ = _potrf(hip, 0, A, ld)
    if n <= 2048:
        cR, cX, _ = _potrf_trtri(hip, A, ld)
    Rt = np.asfortranarray(np.triu(cleanU))
    dT = _dev(Rt, ld)
    hip.call("capi_dtrtri", 1, 0, n, capi.ptr(dT), ld)
    cT = _host(dT, n)
    for J in junks:
        gU, info = _potrf(hip, 1, with_junk(A, lo_strict, J), ld)
        assert info == 0
        np.testing.assert_array_equal(gU[up], cleanU[up])
        np.testing.assert_array_equal(gU[lo_strict], J[lo_strict])
        gL, info = _potrf(hip, 0, with_junk(A, up_strict, J), ld)
        assert info == 0
        np.testing.assert_array_equal(gL[~up_strict], cleanL[~up_strict])
        np.testing.assert_array_equal(gL[up_strict], J[up_strict])
        if n <= 2048:
            gR, gX, info = _potrf_trtri(hip, with_junk(A, lo_strict, J), ld)
            assert info == 0
            np.testing.assert_array_equal(gR, cR)
            np.testing.assert_array_equal(gX, cX)
        dT = _dev(with_junk(Rt, lo_strict, J), ld)
        hip.call("capi_dtrtri", 1, 0, n, capi.ptr(dT), ld)
        gT = _host(dT, n)
        np.testing.assert_array_equal(gT[up], cT[up])
        np.testing.assert_array_equal(gT[lo_strict], J[lo_strict])


# ---------------------------------------------------------------------------------------------------------------------------
# info at tile, leaf and block boundaries
# ---------------------------------------------------------------------------------------------------------------------------
INFO_KS = (0, 3, 4, 15, 16, 17, 127, 128, 129, 1023, 1024)


def _f4_device(n, ks, seed):
    """F4 built on the device (integer entries: the product is exact in any summation order); returns a column-major device image"""
    import torch
    R, s = f4_factor(n, ks, seed)
    Rt = torch.from_numpy(np.ascontiguousarray(R)).cuda()
    st = torch.from_numpy(s).cuda()
    A = Rt.T @ (st[:, None] * Rt)             # symmetric: its row-major storage is the column-major image
    assert A.abs().max().item() < 2.0 ** 53
    return A.contiguous()


@pytest.mark.parametrize("n", [2304, 4224])
def test_info_at_boundaries(hip, oracle, n):
    """F4 with the first failing pivot at k + 1 and a positive diagonal entry of A there: capi_dpotrf_trtri (blocked at 2304,
    recursion at 4224) and capi_dpotrf (U and L) report exactly k + 1, which is what LAPACK's dpotrf reports."""
    import torch
    from capital_amd import capi
    dX = torch.empty((n, n), dtype=torch.float64, device="cuda")
    for k in INFO_KS + (n - 1,):
        A = _f4_device(n, (k,), seed=k)
        if k > 0:
            assert (torch.diagonal(A) > 0).all()
        got = []
        for routine in ("potrf_trtri", "potrf_U", "potrf_L"):
            W = A.clone()
            hip.call("capi_reset_info")
            if routine == "potrf_trtri":
                hip.call("capi_dpotrf_trtri", n, capi.ptr(W), n, capi.ptr(dX), n)
            else:
                hip.call("capi_dpotrf", 1 if routine == "potrf_U" else 0, n, capi.ptr(W), n)
            got.append(hip.info())
        assert got == [k + 1] * 3, (k, got)
        if n == 2304 or k in (1024, n - 1):
            H = np.asfortranarray(A.cpu().numpy())
            assert oracle.dpotrf(1, H) == k + 1
    # two failing pivots: the first is reported
    A = _f4_device(n, (129, 1024), seed=1)
    hip.call("capi_reset_info")
    hip.call("capi_dpotrf_trtri", n, capi.ptr(A), n, capi.ptr(dX), n)
    assert hip.info() == 130
    hip.call("capi_reset_info")
    B = torch.from_numpy(np.ascontiguousarray(f1_spectrum(256, 10.0, 1))).cuda()
    hip.call("capi_dpotrf", 1, 256, capi.ptr(B), 256)
    assert hip.info() == 0


@pytest.mark.parametrize("trsm", (False, True))
def test_schedule_names_the_failing_pivot(drv, trsm):
    """the cholinv schedule and TRSM mode raise DriverError naming the pivot local to the failing base case (stats' bc_dimension)"""
    from capital_amd.driver import DriverError
    n, bc = 2048, -2
    for k in (3, 129, 700, 1024, 2047):
        A = f4_indefinite(n, (k,), seed=k)
        p = drv.Cholinv(n, c=1, complete_inv=0, split=1, bc_mult=bc, serialize=True, trsm_mode=trsm)
        p.set_A(A)
        with pytest.raises(DriverError, match="non-positive pivot") as ei:
            p.factor()
        bcd = p.stats()["bc_dimension"]
        assert bcd == 512
        assert f"non-positive pivot {k % bcd + 1} of a diagonal block" in str(ei.value), (k, str(ei.value))
        p.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the cholinv schedule and TRSM mode: backward error against the oracle's run of the same schedule
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kappa", KAPPAS)
@pytest.mark.parametrize("n,bc,ci,trsm", [(1024, -1, 0, False), (1024, -3, 1, False), (1000, -2, 1, False), (1024, -2, 0, True)])
def test_cholinv_backward_error(drv, oracle, n, bc, ci, trsm, kappa):
    """R: eta <= C max(eta_ref, u) with eta_ref from oracle.cholinv_factor (same n, bc, split, complete_inv).  R^-1 (complete_inv):
    ||X R - I||_F <= C n u || |X||R| ||_F; without complete_inv, the same on the two diagonal halves."""
    A = f1_spectrum(n, kappa, n + int(np.log10(kappa)))
    R, X, _ = _cholinv(drv, A, bc, ci, trsm)
    Rref, Xref, info = oracle.cholinv_factor(A, ci, 1, bc, 1, 1)
    assert info == 0
    eta, eta_ref = oracle.ld_cholesky_backward(A, R), oracle.ld_cholesky_backward(A, Rref)
    print(f"cholinv n={n} bc={bc} ci={ci} trsm={trsm} kappa={kappa:.0e}: eta {eta:.3e} eta_ref {eta_ref:.3e}")
    assert eta <= CB * max(eta_ref, U64), (eta, eta_ref)
    if trsm:
        return
    blocks = [slice(0, n)] if ci else [slice(0, n // 2), slice(n // 2, n)]
    if not ci:
        assert np.all(X[:n // 2, n // 2:] == 0)
    for s in blocks:
        Xs, Rs_ = np.asfortranarray(X[s, s]), np.asfortranarray(R[s, s])
        e, mag = oracle.ld_inverse_residual(Xs, Rs_, 0)
        assert e <= CB * Xs.shape[0] * U64 * mag, (e, mag)


# ---------------------------------------------------------------------------------------------------------------------------
# CholeskyQR2 on ill-conditioned panels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,kappa", [(1 << 16, 256, 1e2), (1 << 16, 256, 1e5), (1 << 16, 256, 1e7),
                                      (1 << 14, 1024, 1e2), (1 << 14, 1024, 1e5), (1 << 14, 1024, 1e7)])
def test_cacqr2_conditioning(drv, oracle, m, n, kappa):
    """A = U diag(sigma) V^T, sigma log-spaced 1 .. 1/kappa, built on the device.  Orthogonality ||Q^T Q - I||_F and the residual
    ||A - QR||_F / ||A||_F in long double, each <= C max(oracle CholeskyQR2's, u).  Width 256 (the panel32 path) at m = 2^16; width
    1024 at m = 2^14 rather than 2^16: the host side (the oracle's CholeskyQR2 and two O(m n^2) long-double checks) grows with m, and
    at 2^16 the three width-1024 cases alone would take ~70 s of the file's 120 s budget."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(int(m + n + np.log10(kappa)))
    Uq, _ = torch.linalg.qr(torch.randn(m, n, dtype=torch.float64, device="cuda", generator=g))
    Vq, _ = torch.linalg.qr(torch.randn(n, n, dtype=torch.float64, device="cuda", generator=g))
    sig = torch.logspace(0, -np.log10(kappa), n, dtype=torch.float64, device="cuda")
    A = np.asfortranarray(((Uq * sig[None, :]) @ Vq.T).cpu().numpy())
    del Uq, Vq
    q = drv.Cacqr(m, n, c=1, variant=2)
    q.set_A(A)
    q.factor()
    Q, R = q.Q(), q.R()
    q.close()
    Qref, Rref, info = oracle.cacqr_factor_1d(A, 1, 2)
    assert info == 0
    orth, res = oracle.ld_qr(A, Q, R)
    orth_ref, res_ref = oracle.ld_qr(A, Qref, Rref)
    print(f"cqr2 {m}x{n} kappa={kappa:.0e}: orth {orth:.3e} (ref {orth_ref:.3e})  res {res:.3e} (ref {res_ref:.3e})")
    assert orth <= CB * max(orth_ref, U64), (orth, orth_ref)
    assert res <= CB * max(res_ref, U64), (res, res_ref)
