"""GPU parity: the triangular product C = alpha op(T) B + beta C (capi_dtrmm_acc -- what the chunked SUMMA pipeline issues for every TRMM
on a grid) and its beta == 0 forms on every path launch_gemm has for a triangular operand: the 32-tile burst kernel, the 64- / 128-tile
kernel with and without split-K, tile pairs, the full-width trmm_ts32 kernel, and the tall right-TRMM with a dense copy of T and one
launch per 256-column block.  The reference is a plain fp64 product of the explicitly masked triangle (numpy on the host; torch fp64
from order 2048 up); for the thin shapes it is also formed in np.longdouble, and the fp64 reference itself must sit inside the
tolerance -- the tolerance is then about rounding, not about the reference.
Tolerances are test_gpu_blas.py's: 1e-14 * max(k, 16) * max(scale, 1) against numpy (k = order of T, scale = largest entry of the
reference), 1e-12 relative to the largest entry against torch.
The planner's choices these shapes rely on are asserted by test_the_plans_are_the_intended_ones (a child process: the plan trace,
CAPI_DEBUG_GEMM, is read once per process)."""
import functools
import itertools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALPHA = -1.5
BETAS = (1.0, -0.75)
LD_FLOPS = 1.1e8          # m * n * k up to which the reference is also formed in np.longdouble
FORMS8 = list(itertools.product((0, 1), (0, 1), (0, 1)))                 # uplo x trans x diag
FORMS16 = list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1)))        # side x uplo x trans x diag
NOTRANS_NONUNIT = [(1, 0, 0), (0, 0, 0)]                                 # upper and lower


def _rand(rng, m, n):
    return np.asfortranarray(rng.uniform(-1, 1, size=(m, n)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _up(*arrays):
    """Host arrays to the device, complete before the handle's stream (which need not be torch's) touches them."""
    import torch
    from capital_amd import capi
    out = [capi.to_device(np.array(a, order="F")) for a in arrays]          # (a copy: the shared operands are read-only)
    torch.cuda.synchronize()
    return out if len(out) > 1 else out[0]


def _down(hip, t):
    from capital_amd import capi
    hip.sync()
    return capi.to_host(t)


def _pad(m, side, uplo, trans, diag):
    """Leading-dimension pad of T and B: none in half of the forms, 1 (odd: no 16-byte loads) or 2 in the others."""
    return (0, 1, 0, 2)[(m + side + uplo + 2 * trans + 3 * diag) % 4]


@functools.lru_cache(maxsize=None)
def _operands(m, n, side, pad):
    """T (nt + pad rows, junk in both triangles), B (m + pad rows), C (m + 3 rows): read-only, shared by every test of the shape."""
    nt = m if side == 0 else n
    rng = np.random.default_rng(1000003 * m + 1009 * n + 10 * side + pad)
    out = (_rand(rng, nt + pad, nt), _rand(rng, m + pad, n), _rand(rng, m + 3, n))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _product(m, n, side, uplo, trans, diag, pad):
    """op(T) B (left) or B op(T) (right) of the masked triangle: fp64, and np.longdouble for the thin shapes (else None)."""
    Tf, Bf, _ = _operands(m, n, side, pad)
    nt = m if side == 0 else n
    T = np.triu(Tf[:nt]) if uplo == 1 else np.tril(Tf[:nt])
    if diag:
        np.fill_diagonal(T, 1.0)
    opT, B = (T.T if trans else T), Bf[:m]
    P = opT @ B if side == 0 else B @ opT
    Pl = None
    if float(m) * n * nt <= LD_FLOPS:
        ld = np.longdouble
        Pl = opT.astype(ld) @ B.astype(ld) if side == 0 else B.astype(ld) @ opT.astype(ld)
        Pl.setflags(write=False)
    P.setflags(write=False)
    return P, Pl


def _check(tag, got, ref, k, ref_ld=None):
    scale = float(np.abs(ref).max())
    tol = 1e-14 * max(k, 16) * max(scale, 1.0)
    err = float(np.abs(got - ref).max())
    gap = None if ref_ld is None else float(np.abs(ref.astype(np.longdouble) - ref_ld).max())
    print(f"[trmm_acc] {tag}: err {err:.3e} tol {tol:.3e} err/tol {err / tol:.1e}" + ("" if gap is None else f" fp64-vs-longdouble {gap:.3e}"))
    assert np.isfinite(got).all(), tag
    if gap is not None:
        assert gap <= tol, f"{tag}: the fp64 reference is {gap:.3e} from the longdouble one, tol {tol:.3e}"
    assert err <= tol, f"{tag}: max err {err:.3e} > tol {tol:.3e}"


def _acc_numpy(hip, m, n, side, uplo, trans, diag, pad):
    """Sub-cases (a)-(d) of one form against numpy; returns the device operands' host images for further checks."""
    from capital_amd import capi
    nt = m if side == 0 else n
    Tf, Bf, Cf = _operands(m, n, side, pad)
    P, Pl = _product(m, n, side, uplo, trans, diag, pad)
    tag = f"{m}x{n} side{side} uplo{uplo} trans{trans} diag{diag} pad{pad}"
    dT, dB = _up(Tf, Bf)
    ldt, ldb, ldc = nt + pad, m + pad, m + 3
    form = (side, uplo, trans, diag, m, n)
    for beta in BETAS:                                                        # (a), and (c): the rows beyond m
        dC = _up(Cf)
        hip.call("capi_dtrmm_acc", *form, ALPHA, capi.ptr(dT), ldt, capi.ptr(dB), ldb, beta, capi.ptr(dC), ldc)
        got = _down(hip, dC)
        _check(f"{tag} beta {beta}", got[:m], ALPHA * P + beta * Cf[:m], nt, None if Pl is None else ALPHA * Pl + beta * Cf[:m].astype(np.longdouble))
        assert np.array_equal(_bits(got[m:]), _bits(Cf[m:])), f"{tag}: rows of C beyond m"
    Cnan = Cf.copy()                                                          # (b): beta == 0 never reads C
    Cnan[:m] = np.nan
    dC, dO = _up(Cnan, Cnan)
    hip.call("capi_dtrmm_acc", *form, ALPHA, capi.ptr(dT), ldt, capi.ptr(dB), ldb, 0.0, capi.ptr(dC), ldc)
    hip.call("capi_dtrmm_oop", *form, ALPHA, capi.ptr(dT), ldt, capi.ptr(dB), ldb, capi.ptr(dO), ldc)
    got, oop = _down(hip, dC), _down(hip, dO)
    _check(f"{tag} beta 0", got[:m], ALPHA * P, nt, None if Pl is None else ALPHA * Pl)
    assert np.array_equal(_bits(got), _bits(oop)), f"{tag}: beta == 0 differs from capi_dtrmm_oop"
    assert np.array_equal(_bits(got[m:]), _bits(Cf[m:]))
    dC, dBn = _up(Cf, np.full(Bf.shape, np.nan))                                  # (d): alpha == 0 reads neither T nor B
    hip.call("capi_dtrmm_acc", *form, 0.0, capi.ptr(dT), ldt, capi.ptr(dBn), ldb, 0.5, capi.ptr(dC), ldc)
    got = _down(hip, dC)
    assert np.array_equal(_bits(got[:m]), _bits(0.5 * Cf[:m])), f"{tag}: alpha == 0"
    assert np.array_equal(_bits(got[m:]), _bits(Cf[m:]))
    return dT, dB


@pytest.mark.parametrize("side,uplo,trans,diag", FORMS16)
@pytest.mark.parametrize("m,n", [(200, 130), (129, 257)])
def test_acc_small(hip, m, n, side, uplo, trans, diag):
    """The 32-tile burst kernel: its epilogue reads the old C once per register when beta != 0."""
    _acc_numpy(hip, m, n, side, uplo, trans, diag, _pad(m, side, uplo, trans, diag))


@pytest.mark.parametrize("uplo,trans,diag", FORMS8)
def test_acc_tile(hip, uplo, trans, diag):
    """Left 1024 x 1024: the 64-tile kernel in one launch, no split."""
    _acc_numpy(hip, 1024, 1024, 0, uplo, trans, diag, _pad(1024, 0, uplo, trans, diag))


SPLITK = [(0, 1024, 64, f) for f in FORMS8] + [(1, 64, 1024, f) for f in FORMS8] + \
         [(s, m, n, f) for s, m, n in ((0, 777, 40), (0, 2048, 128), (1, 100, 2048)) for f in NOTRANS_NONUNIT]


@pytest.mark.parametrize("side,m,n,form", SPLITK, ids=[f"{'LR'[s]}-{m}x{n}-uplo{f[0]}-trans{f[1]}-diag{f[2]}" for s, m, n, f in SPLITK])
def test_splitk_triangular(hip, side, m, n, form):
    """Thin TRMMs are split along k: every slice intersects its k-range with the tile's live range, which ends at T's diagonal (a
    slice wholly in the dead part still contributes an exact zero slab), and the reduction applies alpha and beta.  beta != 0 through
    capi_dtrmm_acc, beta == 0 through capi_dtrmm_oop and the in-place capi_dtrmm, whose result must have the same bits."""
    from capital_amd import capi
    uplo, trans, diag = form
    pad = _pad(m, side, uplo, trans, diag)
    dT, dB = _acc_numpy(hip, m, n, side, uplo, trans, diag, pad)
    nt = m if side == 0 else n
    Bf = _operands(m, n, side, pad)[1]
    dO = _up(np.full((m, n), np.nan))
    hip.call("capi_dtrmm_oop", side, uplo, trans, diag, m, n, ALPHA, capi.ptr(dT), nt + pad, capi.ptr(dB), m + pad, capi.ptr(dO), m)
    hip.call("capi_dtrmm", side, uplo, trans, diag, m, n, ALPHA, capi.ptr(dT), nt + pad, capi.ptr(dB), m + pad)
    oop, inp = _down(hip, dO), _down(hip, dB)
    P, Pl = _product(m, n, side, uplo, trans, diag, pad)
    _check(f"{m}x{n} side{side} uplo{uplo} trans{trans} diag{diag} pad{pad} oop", oop, ALPHA * P, nt, None if Pl is None else ALPHA * Pl)
    assert np.array_equal(_bits(inp[:m]), _bits(oop)), "in-place differs from out-of-place"
    assert np.array_equal(_bits(inp[m:]), _bits(Bf[m:])), "in-place: rows of B beyond m"


# ---- orders of 2048 and up, and the tall shapes: operands made on the device, torch fp64 as the reference ---------------------------------
def _torch_case(m, n, side, uplo, trans, diag, padT, padB, padC, seed, poison=False):
    """Row-major (cols, ld) tensors that hold the column-major operands; the logical op(T) of the masked triangle."""
    import torch
    nt = m if side == 0 else n
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.rand(s, dtype=torch.float64, device="cuda", generator=g) - 0.5
    Tt, Bt, Ct = rnd(nt, nt + padT), rnd(n, m + padB), rnd(n, m + padC)
    T = Tt[:, :nt].T
    T = torch.triu(T) if uplo == 1 else torch.tril(T)
    if diag:
        T = T - torch.diag(torch.diagonal(T)) + torch.eye(nt, dtype=torch.float64, device="cuda")
    if poison:                    # NaN wherever BLAS promises not to look: the other strict triangle, a unit diagonal, the padding rows
        Tt = Tt.clone()
        keep = torch.triu(torch.ones((nt, nt), dtype=torch.bool, device="cuda"), 1 if diag else 0)      # logical upper part
        keep = keep if uplo == 1 else keep.T
        Tt[:, :nt][~keep.T] = float("nan")
        Tt[:, nt:] = float("nan")
    return Tt, Bt, Ct, (T.T if trans else T)


def _acc_torch(tag, m, n, side, uplo, trans, diag, padT, padB, padC, betas):
    import torch
    from capital_amd import capi
    h = capi.Handle(0)
    nt = m if side == 0 else n
    Tt, Bt, C0, opT = _torch_case(m, n, side, uplo, trans, diag, padT, padB, padC, seed=m + n + 8 * side + 4 * uplo + 2 * trans + diag)
    Bm = Bt[:, :m].T
    prod = opT @ Bm if side == 0 else Bm @ opT                              # logical m x n
    form = (side, uplo, trans, diag, m, n)
    ldt, ldb, ldc = nt + padT, m + padB, m + padC
    torch.cuda.synchronize()

    def check(Ct, ref, what):
        err, scale = (Ct[:, :m].T - ref).abs().max().item(), ref.abs().max().item()
        print(f"[trmm_acc] {tag} {what}: err {err:.3e} tol {1e-12 * scale:.3e} err/tol {err / (1e-12 * scale):.1e}")
        assert torch.isfinite(Ct[:, :m]).all().item(), (tag, what)
        assert err <= 1e-12 * scale, (tag, what, err, scale)
        assert torch.equal(Ct[:, m:], C0[:, m:]), (tag, what, "rows of C beyond m")

    for beta in betas:
        if beta != 0.0:                                                       # (a), (c)
            Ct = C0.clone()
            h.call("capi_dtrmm_acc", *form, ALPHA, capi.ptr(Tt), ldt, capi.ptr(Bt), ldb, beta, capi.ptr(Ct), ldc)
            h.sync()
            check(Ct, ALPHA * prod + beta * C0[:, :m].T, f"beta {beta}")
        else:                                                                 # (b)
            Ct = C0.clone()
            Ct[:, :m] = float("nan")
            Co = Ct.clone()
            h.call("capi_dtrmm_acc", *form, ALPHA, capi.ptr(Tt), ldt, capi.ptr(Bt), ldb, 0.0, capi.ptr(Ct), ldc)
            h.call("capi_dtrmm_oop", *form, ALPHA, capi.ptr(Tt), ldt, capi.ptr(Bt), ldb, capi.ptr(Co), ldc)
            h.sync()
            check(Ct, ALPHA * prod, "beta 0")
            assert torch.equal(Ct, Co), (tag, "beta == 0 differs from capi_dtrmm_oop")
    Ct, Bn = C0.clone(), torch.full_like(Bt, float("nan"))                    # (d)
    h.call("capi_dtrmm_acc", *form, 0.0, capi.ptr(Tt), ldt, capi.ptr(Bn), ldb, 0.5, capi.ptr(Ct), ldc)
    h.sync()
    assert torch.equal(Ct[:, :m], 0.5 * C0[:, :m]) and torch.equal(Ct[:, m:], C0[:, m:]), (tag, "alpha == 0")
    h.close()


@pytest.mark.parametrize("side,uplo,trans", [(0, 1, 0), (0, 0, 1), (1, 0, 0), (1, 1, 1)])
def test_acc_order_4096(side, uplo, trans):
    """beta != 0 keeps an order-4096 TRMM off the pair kernel (gemm_plan.h): the 128-tile kernel with unequal k-ranges, longest first."""
    _acc_torch(f"4096x4096 side{side} uplo{uplo} trans{trans}", 4096, 4096, side, uplo, trans, 0, 0, 0, 3, (1.0, 0.0))


@pytest.mark.parametrize("m,padB,padC", [(64 * 256 + 77, 3, 3), (64 * 256, 0, 3), (64 * 256, 0, 0)])
def test_acc_ts32(m, padB, padC):
    """The full-width T-stationary kernel (right, upper, n = 256, m >= 64 n) and its beta branch: a ragged last 32-row tile with odd
    leading dimensions, whole tiles, and whole tiles with even leading dimensions (the branch-free steady iterations when beta == 0)."""
    _acc_torch(f"ts32 {m}x256 padB{padB} padC{padC}", m, 256, 1, 1, 0, 0, 1 if padB else 0, padB, padC, (0.0, 1.0, -0.75))


@pytest.mark.parametrize("uplo", (1, 0))
def test_acc_tall_right_dense_t(uplo):
    """Right, n = 512, m = 64 n + 77: T's triangle is copied into a zeroed block; upper op(T) then goes out as one launch per
    256-column block (the first on the T-stationary kernel, the second on the 128-tile kernel with K = 512), lower as one launch."""
    m = 64 * 512 + 77
    _acc_torch(f"dense-T {m}x512 uplo{uplo}", m, 512, 1, uplo, 0, 0, 2 * uplo, 3 * uplo, 3, (0.0, 1.0))


# ---- NaN where T must not be read ---------------------------------------------------------------------------------------------------
def _poisoned(Tf, nt, uplo, diag):
    T = np.array(Tf, order="F")
    i, j = np.indices((nt, nt))
    dead = (i > j) if uplo == 1 else (i < j)
    if diag:
        dead |= i == j
    T[:nt][dead] = np.nan
    T[nt:] = np.nan
    return T


NAN_NUMPY = [(0, 200, 130), (1, 200, 130), (0, 1024, 1024), (0, 1024, 64), (1, 64, 1024)]


@pytest.mark.parametrize("uplo,trans,diag", FORMS8)
@pytest.mark.parametrize("side,m,n", NAN_NUMPY)
def test_nan_outside_the_triangle(hip, side, m, n, uplo, trans, diag):
    """The other strict triangle of T, a unit diagonal and the rows between nt and ldt are never read: with NaN there (0 * NaN is NaN:
    masking by multiplication would show) the product is finite and unchanged.  Even pad: the 16-byte loads stay in play."""
    from capital_amd import capi
    nt, pad = (m if side == 0 else n), 2
    Tf, Bf, _ = _operands(m, n, side, pad)
    P, Pl = _product(m, n, side, uplo, trans, diag, pad)
    dT, dB, dC = _up(_poisoned(Tf, nt, uplo, diag), Bf, np.full((m, n), np.nan))
    hip.call("capi_dtrmm_oop", side, uplo, trans, diag, m, n, ALPHA, capi.ptr(dT), nt + pad, capi.ptr(dB), m + pad, capi.ptr(dC), m)
    _check(f"NaN-T {m}x{n} side{side} uplo{uplo} trans{trans} diag{diag}", _down(hip, dC), ALPHA * P, nt, None if Pl is None else ALPHA * Pl)


@pytest.mark.parametrize("tag,m,n,side,uplo,diag", [("pair", 4096, 4096, 0, 1, 0), ("pair", 4096, 4096, 0, 0, 1), ("pair", 4096, 4096, 1, 1, 1),
                                                    ("pair", 4096, 4096, 1, 0, 0), ("ts32", 16461, 256, 1, 1, 0), ("ts32", 16461, 256, 1, 1, 1),
                                                    ("dense-T", 32845, 512, 1, 1, 0), ("dense-T", 32845, 512, 1, 0, 0)])
def test_nan_outside_the_triangle_large(tag, m, n, side, uplo, diag):
    import torch
    from capital_amd import capi
    h = capi.Handle(0)
    nt = m if side == 0 else n
    Tt, Bt, _, opT = _torch_case(m, n, side, uplo, 0, diag, 2, 0, 0, seed=m + n + side + uplo + diag, poison=True)
    Ct = torch.full((n, m), float("nan"), dtype=torch.float64, device="cuda")
    Bm = Bt.T
    ref = ALPHA * (opT @ Bm if side == 0 else Bm @ opT)
    torch.cuda.synchronize()
    h.call("capi_dtrmm_oop", side, uplo, 0, diag, m, n, ALPHA, capi.ptr(Tt), nt + 2, capi.ptr(Bt), m, capi.ptr(Ct), m)
    h.sync()
    err, scale = (Ct.T - ref).abs().max().item(), ref.abs().max().item()
    print(f"[trmm_acc] NaN-T {tag} {m}x{n} side{side} uplo{uplo} diag{diag}: err {err:.3e} tol {1e-12 * scale:.3e} err/tol {err / (1e-12 * scale):.1e}")
    assert torch.isfinite(Ct).all().item()
    assert err <= 1e-12 * scale
    h.close()


@pytest.mark.parametrize("uplo,diag", list(itertools.product((0, 1), (0, 1))))
@pytest.mark.parametrize("m,n", [(300, 70), (600, 520)])
def test_dtrsm_nan_outside_the_triangle(hip, oracle, m, n, uplo, diag):
    """capi_dtrsm's leaves copy and transpose only the referenced triangle; the rest of the caller's T may hold anything (test_dtrsm's
    operands and tolerance)."""
    from capital_amd import capi
    rng = np.random.default_rng(uplo * 4 + diag + m)
    pad = 2
    Tf = np.asfortranarray(_rand(rng, m + pad, m) * 0.1)
    Tf[:m] += np.eye(m) * 4.0                                                 # well conditioned
    B = _rand(rng, m, n)
    Tclean = np.asfortranarray(Tf[:m])
    ref = B.copy(order="F")
    oracle.dtrsm(0, uplo, 0, diag, 0.5, Tclean, ref)
    dT, dB = _up(_poisoned(Tf, m, uplo, diag), B)
    hip.call("capi_dtrsm", 0, uplo, 0, diag, m, n, 0.5, capi.ptr(dT), m + pad, capi.ptr(dB), m)
    got = _down(hip, dB)
    tol = 1e-12 * max(1.0, np.abs(ref).max())
    err = np.abs(got - ref).max()
    print(f"[trmm_acc] NaN-T trsm {m}x{n} uplo{uplo} diag{diag}: err {err:.3e} tol {tol:.3e} err/tol {err / tol:.1e}")
    assert np.isfinite(got).all()
    assert err <= tol


# ---- the paths must be the intended ones -----------------------------------------------------------------------------------------------
def _row(tag, side, uplo, m, n, beta, fn="acc", trans=0):
    return dict(tag=tag, fn=fn, side=side, uplo=uplo, trans=trans, diag=0, m=m, n=n, beta=beta)


PLAN_ROWS = [
    _row("small_200x130", 0, 1, 200, 130, 1.0), _row("small_129x257", 1, 1, 129, 257, 1.0),
    _row("tile_1024", 0, 1, 1024, 1024, 1.0),
    _row("tile_4096_beta1", 0, 1, 4096, 4096, 1.0), _row("pair_4096_beta0", 0, 1, 4096, 4096, 0.0),
    _row("tile_4096_right_beta1", 1, 0, 4096, 4096, 1.0),
    _row("dense_upper_beta0", 1, 1, 64 * 512 + 77, 512, 0.0), _row("dense_upper_beta1", 1, 1, 64 * 512 + 77, 512, 1.0),
    _row("dense_lower_beta1", 1, 0, 64 * 512 + 77, 512, 1.0),
]
for _s, _m, _n in ((0, 1024, 64), (0, 777, 40), (0, 2048, 128), (1, 64, 1024), (1, 100, 2048)):
    PLAN_ROWS += [_row(f"splitk_{_m}x{_n}_beta0", _s, 1, _m, _n, 0.0, fn="oop"), _row(f"splitk_{_m}x{_n}_beta1", _s, 1, _m, _n, 1.0),
                  _row(f"splitk_{_m}x{_n}_lower_beta1", _s, 0, _m, _n, -0.75), _row(f"splitk_{_m}x{_n}_inplace", _s, 1, _m, _n, 0.0, fn="inplace")]
for _m in (64 * 256 + 77, 64 * 256):
    PLAN_ROWS += [_row(f"ts32_{_m}_beta0", 1, 1, _m, 256, 0.0), _row(f"ts32_{_m}_beta1", 1, 1, _m, 256, 1.0)]


def test_the_plans_are_the_intended_ones():
    """A parity test that silently runs on another kernel proves nothing: one call per row of the case table in a fresh process with the
    plan trace on; every row must take the path the tests above are named after (plans of a 256-CU device)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, "tests", "_gpu_trmm_plan_main.py"), json.dumps(PLAN_ROWS)],
                         env=dict(os.environ, CAPI_DEBUG_GEMM="1"), cwd=root, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    cus = int(re.search(r"^num_cu (\d+)$", res.stderr, re.M).group(1))
    if cus != 256:
        pytest.skip(f"the expected plans are those of a 256-CU device; this one has {cus}")
    plans, cur = {}, None
    for line in res.stderr.splitlines():
        if line.startswith("row "):
            cur = plans.setdefault(line[4:].strip(), [])
        elif line.startswith("[capi gemm]") and cur is not None:
            prod, plan = line[len("[capi gemm] "):].split(" -> ")
            cur.append({k: v for k, v in (t.split("=", 1) for t in (prod + " " + plan).split())})
    assert set(plans) == {r["tag"] for r in PLAN_ROWS}
    one = lambda tag: (plans[tag][0] if len(plans[tag]) == 1 else pytest.fail(f"{tag}: {len(plans[tag])} products, expected one"))
    for r in PLAN_ROWS:
        tag = r["tag"]
        for p in plans[tag]:
            assert p["tri_side"] == str(r["side"]) and float(p["beta"]) == r["beta"], (tag, p)
        if tag.startswith("small"):
            assert one(tag)["path"] == "small", (tag, plans[tag])
        elif tag == "tile_1024":
            p = one(tag)
            assert (p["path"], p["ts"], p["splitk"]) == ("tile", "64", "1"), (tag, p)
        elif tag.startswith("tile_4096"):
            p = one(tag)
            assert (p["path"], p["ts"], p["splitk"]) == ("tile", "128", "1"), (tag, p)
        elif tag.startswith("pair"):
            assert one(tag)["path"] == "pair", (tag, plans[tag])
        elif tag.startswith("splitk"):
            p = one(tag)
            assert p["path"] == "tile" and int(p["splitk"]) > 1 and p["reduce"] == "narrow", (tag, p)
        elif tag.startswith("ts32"):
            assert one(tag)["path"] == "trmm_ts32", (tag, plans[tag])
        elif tag.startswith("dense_upper"):
            got = [(p["tri_dense"], p["tri_block"], p["K"], p["tri_koff"], p["path"]) for p in plans[tag]]
            assert got == [("1", "1", "256", "0", "trmm_ts32"), ("1", "1", "512", "256", "tile")], (tag, got)
        elif tag.startswith("dense_lower"):
            p = one(tag)
            assert (p["tri_dense"], p["tri_block"], p["path"], p["K"]) == ("1", "0", "tile", "512"), (tag, p)
        else:
            pytest.fail(f"no expectation for row {tag}")
    assert {plans[f"splitk_{m}x{n}_beta1"][0]["splitk"] for m, n in ((1024, 64), (64, 1024))} == {"4"}
    assert plans["splitk_777x40_beta1"][0]["splitk"] == "3" and plans["splitk_777x40_beta1"][0]["k_per_split"] == "272"
    assert plans["splitk_2048x128_beta1"][0]["splitk"] == "7" and plans["splitk_2048x128_beta1"][0]["k_per_split"] == "304"
    assert plans["splitk_100x2048_beta1"][0]["splitk"] == "7"
