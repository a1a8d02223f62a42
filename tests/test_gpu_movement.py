"""GPU parity (bit-exact): generators, serialize / pack, triangle removal, block<->cyclic re-indexing against
the oracle's loop-for-loop restatement of structure.hpp:36-129, serialize.hpp:12-150, util.hpp:56-318; past one workgroup, on
rectangular pieces and with padded leading dimensions against the numpy references of tests/_movement_ref.py, which
tests/test_movement_ref.py holds against the same oracle."""
import numpy as np
import pytest

import _movement_cases as mc
import _movement_ref as mref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,d,px,py", [(64, 1, 0, 0), (1000, 1, 0, 0), (1001, 2, 1, 0), (1001, 2, 1, 1), (777, 3, 2, 1), (4096, 2, 0, 1)])
def test_distribute_symmetric_bit_exact(hip, oracle, n, d, px, py):
    from capital_amd import capi
    ref = oracle.distribute_symmetric(n, n, px, py, d, d, key=7)
    dy, dx = ref.shape
    dev = capi.to_device(np.full((dy, dx), np.nan))
    hip.call("capi_distribute_symmetric", capi.ptr(dev), dx, dy, n, n, px, py, d, d, 7, 1)
    np.testing.assert_array_equal(capi.to_host(dev), ref)


@pytest.mark.parametrize("m,n,P,p", [(4096, 64, 1, 0), (100003, 33, 4, 3), (100003, 33, 4, 2), (65536, 256, 8, 5), (31, 7, 1, 0)])
def test_distribute_random_bit_exact(hip, oracle, m, n, P, p):
    """One sequential drand48 stream per rank (structure.hpp:105-129) reproduced with 48-bit LCG jump-ahead."""
    from capital_amd import capi
    key = p  # bench/qr/cacqr.cpp:34: key = rank / c
    ref = oracle.distribute_random(n, m, 0, p, 1, P, key=key)
    dy, dx = ref.shape
    dev = capi.to_device(np.full((dy, dx), np.nan))
    hip.call("capi_distribute_random", capi.ptr(dev), dx, dy, n, m, 0, p, 1, P, key)
    np.testing.assert_array_equal(capi.to_host(dev), ref)


def test_distribute_identity(hip, oracle):
    from capital_amd import capi
    ref = oracle.distribute_identity(101, 101, 1, 1, 2, 2, 3.5)
    dy, dx = ref.shape
    dev = capi.to_device(np.full((dy, dx), np.nan))
    hip.call("capi_distribute_identity", capi.ptr(dev), dx, dy, 101, 101, 1, 1, 2, 2, 3.5)
    np.testing.assert_array_equal(capi.to_host(dev), ref)


def _packed_len(st, n):
    return n * n if st == 0 else n * (n + 1) // 2


@pytest.mark.parametrize("ss,ds", [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0), (2, 2)])
def test_serialize(hip, oracle, ss, ds):
    """The seven specialisations of serialize<S1,S2> (serialize.h:19-70) on a sub-range."""
    import ctypes as C
    from capital_amd import capi
    rng = np.random.default_rng(ss * 3 + ds)
    sn, dn = 90, 70
    src = rng.uniform(size=_packed_len(ss, sn))
    dst0 = rng.uniform(size=_packed_len(ds, dn))
    # diagonal sub-block so that triangular layouts are addressed legally
    ssx, sex, ssy, sey = 20, 60, 20, 60
    dsx, dex, dsy, dey = 10, 50, 10, 50
    ref = dst0.copy()
    dp = C.POINTER(C.c_double)
    oracle.lib().orc_serialize(ss, ds, src.ctypes.data_as(dp), sn, sn, ref.ctypes.data_as(dp), dn, dn, ssx, sex, ssy, sey, dsx, dex, dsy, dey)
    import torch
    dsrc, ddst = torch.from_numpy(src).cuda(), torch.from_numpy(dst0).cuda()
    hip.call("capi_serialize", ss, ds, capi.ptr(dsrc), sn, sn, capi.ptr(ddst), dn, dn, ssx, sex, ssy, sey, dsx, dex, dsy, dey)
    np.testing.assert_array_equal(ddst.cpu().numpy(), ref)


def test_lacpy_trizero_axpby_remove_triangle(hip, oracle):
    from capital_amd import capi
    import torch
    rng = np.random.default_rng(3)
    m, n = 150, 140
    A, B = rng.uniform(size=(m, n)), rng.uniform(size=(m, n))
    for part in (0, 1, 2):
        dA, dB = capi.to_device(A), capi.to_device(B)
        hip.call("capi_dlacpy", part, m, n, capi.ptr(dA), m, capi.ptr(dB), m)
        i, j = np.indices((m, n))
        sel = np.ones((m, n), bool) if part == 0 else (i <= j if part == 1 else i >= j)
        np.testing.assert_array_equal(capi.to_host(dB), np.where(sel, A, B))
    S = rng.uniform(size=(n, n))
    for keep in (0, 1):
        dS = capi.to_device(S)
        hip.call("capi_dtrizero", keep, n, capi.ptr(dS), n)
        np.testing.assert_array_equal(capi.to_host(dS), np.triu(S) if keep else np.tril(S))
    x, y = rng.uniform(size=100001), rng.uniform(size=100001)
    dx, dy = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    hip.call("capi_daxpby", x.size, -0.25, capi.ptr(dx), capi.ptr(dy))
    np.testing.assert_array_equal(dy.cpu().numpy(), -0.25 * y + x)       # summa.hpp:33,153
    # util::remove_triangle (util.hpp:266-291) by GLOBAL index on a 2x2 grid piece
    L = rng.uniform(size=(40, 40))
    for d_, (px, py) in ((b'U', (1, 0)), (b'L', (0, 1)), (b'U', (0, 0))):
        dL = capi.to_device(L)
        hip.call("capi_remove_triangle", d_, capi.ptr(dL), 40, 40, px, py, 2)
        jj, ii = np.indices((40, 40))     # L[row j, col i]
        gx, gy = px + ii * 2, py + jj * 2
        ref = np.where((gy > gx) if d_ == b'U' else (gy < gx), 0.0, L)
        np.testing.assert_array_equal(capi.to_host(dL), ref)


def _fma_exact(alpha, X, beta, Y):
    """fl(beta * y + fl(alpha * x)), the sum and the product beta * y rounded ONCE: exact rational arithmetic, correctly rounded."""
    from fractions import Fraction
    ax, out, fb = alpha * X, np.empty_like(X), Fraction(beta)
    for idx in np.ndindex(X.shape):
        out[idx] = float(fb * Fraction(float(Y[idx])) + Fraction(float(ax[idx])))
    return out


@pytest.mark.parametrize("part,m,n", [(p, m, n) for m, n in ((150, 140), (1, 1), (513, 9), (1024, 1024), (3, 65538)) for p in (0, 1, 2) if p or m < 1024])
def test_geadd(hip, part, m, n):
    """capi_dgeadd, Y(part) = alpha X + beta Y: the beta-axpy of every SUMMA product (parts 1 / 2: the triangular-output forms) and the
    final accumulation of cholinv::solve; triangle convention of capi_dlacpy.  The kernel does one multiply and one multiply-add per
    element, and the compiler contracts the latter (v_fmac_f64: beta * y is not rounded on its own).  So: the result equals
    fl(beta y + fl(alpha x)) BIT FOR BIT (checked in exact arithmetic at the small shapes, signed operands), and numpy's twice-rounded
    alpha * X + beta * Y to 1 ulp of the result (operands of one sign: the two forms differ by half an ulp of beta y, which nothing
    bounds by the result when the terms cancel).  Everything outside the part, and the padding rows, stays as it was."""
    import torch
    from capital_amd import capi
    rng = np.random.default_rng(100 * m + 10 * n + part)
    ldx, ldy = m + 2, m + 5
    X, Y = rng.uniform(-1, 1, size=(ldx, n)), rng.uniform(-1, 1, size=(ldy, n))
    i, j = np.indices((m, n))
    sel = np.ones((m, n), bool) if part == 0 else (i <= j if part == 1 else i >= j)
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)

    def run(alpha, Xh, beta, Yh, x_is_y=False):
        dY = capi.to_device(Yh)
        dX = dY if x_is_y else capi.to_device(Xh)
        torch.cuda.synchronize()
        hip.call("capi_dgeadd", part, m, n, alpha, capi.ptr(dX), ldy if x_is_y else ldx, beta, capi.ptr(dY), ldy)
        hip.sync()
        got = capi.to_host(dY)
        assert np.array_equal(bits(got[:m][~sel]), bits(Yh[:m][~sel])), "outside the part"
        assert np.array_equal(bits(got[m:]), bits(Yh[m:])), "padding rows"
        return got[:m][sel]

    if m * n <= 25000:
        got = run(-1.5, X, -0.75, Y)
        assert np.array_equal(bits(got), bits(_fma_exact(-1.5, X[:m][sel], -0.75, Y[:m][sel])))
    Xp, Yp = np.abs(X), np.abs(Y)
    got, ref = run(0.75, Xp, 1.25, Yp), (0.75 * Xp[:m] + 1.25 * Yp[:m])[sel]
    assert np.all(np.abs(got - ref) <= np.spacing(ref))
    Ynan = np.full((ldy, n), np.nan)
    got = run(0.0, None, 0.0, Ynan, x_is_y=True)                      # the Y = 0 idiom of summa.h: alpha = beta = 0, X == Y
    assert np.array_equal(bits(got), bits(np.zeros(got.shape)))
    got = run(1.0, X, 0.0, Ynan)                                      # beta == 0 never reads Y
    assert np.array_equal(bits(got), bits(X[:m][sel]))


@pytest.mark.parametrize("rl,d", [(8, 2), (5, 3), (16, 1)])
def test_block_cyclic(hip, oracle, rl, d):
    import ctypes as C
    import torch
    from capital_amd import capi
    rng = np.random.default_rng(rl + d)
    blocked = rng.uniform(size=rl * rl * d * d)
    ref = np.zeros((rl * d) * (rl * d))
    dp = C.POINTER(C.c_double)
    oracle.lib().orc_block_to_cyclic_rect(blocked.ctypes.data_as(dp), ref.ctypes.data_as(dp), rl, rl, d)
    db, dc = torch.from_numpy(blocked).cuda(), torch.zeros(ref.size, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()             # torch fills on ITS stream; the handle runs on its own
    hip.call("capi_block_to_cyclic", capi.ptr(db), capi.ptr(dc), rl, rl, d)
    hip.sync()
    np.testing.assert_array_equal(dc.cpu().numpy(), ref)
    full = rng.uniform(size=ref.size)
    back = np.zeros_like(blocked)
    oracle.lib().orc_cyclic_to_block_rect(back.ctypes.data_as(dp), full.ctypes.data_as(dp), rl, rl, d)
    db2, dfull = torch.zeros(blocked.size, dtype=torch.float64, device="cuda"), torch.from_numpy(full).cuda()
    torch.cuda.synchronize()
    hip.call("capi_cyclic_to_block", capi.ptr(db2), capi.ptr(dfull), rl, rl, d)
    hip.sync()
    np.testing.assert_array_equal(db2.cpu().numpy(), back)


def test_diff_norms(hip, oracle):
    from capital_amd import capi
    rng = np.random.default_rng(9)
    m, n = 300, 200
    X, Y = rng.uniform(size=(m, n)), rng.uniform(size=(m, n))
    import ctypes as C
    out = (C.c_double * 2)()
    dX, dY = capi.to_device(X), capi.to_device(Y)
    hip.call("capi_diff_norms", 1, m, n, capi.ptr(dX), m, capi.ptr(dY), m, out)
    i, j = np.indices((m, n))
    sel = i <= j
    assert abs(out[0] - ((X - Y)[sel] ** 2).sum()) <= 1e-10 and abs(out[1] - (Y[sel] ** 2).sum()) <= 1e-10


def test_two_streams_and_events(hip, oracle):
    """capi_stream_select / capi_event_record / capi_event_wait: work issued on the communication stream is ordered
    against the compute stream only through events (the chunked SUMMA pipeline relies on exactly this)."""
    import torch
    from capital_amd import capi
    n = 1 << 22
    x = torch.ones(n, dtype=torch.float64, device="cuda")
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    z = torch.zeros(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for rep in range(3):
        hip.call("capi_daxpby", n, 1.0, capi.ptr(x), capi.ptr(y))          # compute stream: y += x
        hip.call("capi_event_record", 0)
        hip.call("capi_stream_select", 1)
        hip.call("capi_event_wait", 0)
        hip.call("capi_daxpby", n, 0.0, capi.ptr(y), capi.ptr(z))          # comm stream: z = y (must see the update)
        hip.call("capi_event_record", 1)
        hip.call("capi_stream_select", 0)
        hip.call("capi_event_wait", 1)
        hip.call("capi_daxpby", n, 1.0, capi.ptr(z), capi.ptr(y))          # compute stream: y += z
    hip.sync()
    # y: 1 -> 2 | 3 -> 6 | 7 -> 14 ; z follows y before the doubling
    assert float(y[0]) == 14.0 and float(y[-1]) == 14.0 and float(z[12345]) == 7.0


def test_stream_select_takes_two_indices(hip):
    """capi_stream_select: 0 (compute) and 1 (communication / packing) are the handle's streams; any other index is CAPI_EINVAL,
    names the argument, and leaves the selected stream as it was: a product launched afterwards is right"""
    from capital_amd import capi
    hip.call("capi_stream_select", 1)
    hip.call("capi_stream_select", 0)
    for bad in (2, -1):
        assert hip.L.capi_stream_select(hip.h, bad) == -1                    # CAPI_EINVAL
        assert "stream index" in hip.L.capi_last_error(hip.h).decode()
    n = 128
    A = np.asfortranarray(np.eye(n))
    B = np.asfortranarray(np.arange(n * n, dtype=np.float64).reshape(n, n) % 97 + np.arange(n)[:, None] * 0.5)
    dA, dB, dC = capi.to_device(A), capi.to_device(B), capi.zeros(n, n)
    hip.call("capi_dgemm", 0, 0, n, n, n, 1.0, capi.ptr(dA), n, capi.ptr(dB), n, 0.0, capi.ptr(dC), n)
    np.testing.assert_array_equal(capi.to_host(dC), B)


@pytest.mark.parametrize("rl,d", [(8, 2), (5, 3), (16, 1), (33, 2)])
def test_block_cyclic_triangle(hip, oracle, rl, d):
    """packed-triangle pieces (util.hpp:57-102,167-201): device kernels bit-exact against the oracle's restatement, and a round
    trip through the aggregate restores every packed entry that lies in the aggregate's upper triangle"""
    import ctypes as C
    import torch
    from capital_amd import capi
    psz = rl * (rl + 1) // 2
    rng = np.random.default_rng(rl * 7 + d)
    blocked = rng.uniform(0.5, 1.5, size=psz * d * d)
    ref = np.zeros((rl * d) * (rl * d))
    dp = C.POINTER(C.c_double)
    oracle.lib().orc_block_to_cyclic_triangle(blocked.ctypes.data_as(dp), ref.ctypes.data_as(dp), blocked.size, rl, rl, d)
    db = torch.from_numpy(blocked).cuda()
    dc = torch.full((ref.size,), -3.0, dtype=torch.float64, device="cuda")          # every entry of the aggregate must be written
    torch.cuda.synchronize()             # torch fills on ITS stream; the handle runs on its own
    hip.call("capi_block_to_cyclic_tri", capi.ptr(db), capi.ptr(dc), rl, d)
    hip.sync()
    np.testing.assert_array_equal(dc.cpu().numpy(), ref)
    back = np.full(blocked.size, -5.0)
    oracle.lib().orc_cyclic_to_block_triangle(back.ctypes.data_as(dp), ref.ctypes.data_as(dp), blocked.size, rl, rl, d)
    db2 = torch.full((blocked.size,), -9.0, dtype=torch.float64, device="cuda")      # every packed entry must be written
    torch.cuda.synchronize()
    hip.call("capi_cyclic_to_block_tri", capi.ptr(db2), capi.ptr(dc), rl, d)
    hip.sync()
    got = db2.cpu().numpy()
    np.testing.assert_array_equal(got, back)
    changed = np.nonzero(got != blocked)[0]
    assert len(changed) == rl * (d * (d - 1) // 2) and np.all(got[changed] == 0.0)   # local diagonals of the pieces with y > x


@pytest.mark.parametrize("L,d", [(8, 2), (5, 3), (33, 2), (16, 1)])
def test_cyclic_to_local(hip, oracle, L, d):
    """util::cyclic_to_local (util.hpp:131-164) for every slice rank: bit-exact against the oracle's front-to-back restatement"""
    import ctypes as C
    import torch
    from capital_amd import capi
    bc = L * d
    rng = np.random.default_rng(L + 13 * d)
    dp = C.POINTER(C.c_double)
    for sr in range(d * d):
        T, TI = rng.uniform(size=bc * bc), rng.uniform(size=bc * bc)
        rT, rTI = T.copy(), TI.copy()
        oracle.lib().orc_cyclic_to_local.argtypes = [dp, dp] + [C.c_int64] * 4
        oracle.lib().orc_cyclic_to_local(rT.ctypes.data_as(dp), rTI.ctypes.data_as(dp), L, bc, d, sr)
        dT, dTI = torch.from_numpy(T).cuda(), torch.from_numpy(TI).cuda()
        torch.cuda.synchronize()
        hip.call("capi_cyclic_to_local", capi.ptr(dT), capi.ptr(dTI), L, bc, d, sr)
        hip.sync()
        got, goti = dT.cpu().numpy().reshape(bc, bc), dTI.cpu().numpy().reshape(bc, bc)
        np.testing.assert_array_equal(got[:L, :L], rT.reshape(bc, bc)[:L, :L])           # the leading corner (column index first)
        np.testing.assert_array_equal(goti[:L, :L], rTI.reshape(bc, bc)[:L, :L])


@pytest.mark.parametrize("m,n,lda,ldb,off", [(1, 1, 1, 1, 0), (7, 5, 9, 11, 0), (512, 8, 512, 512, 0), (513, 9, 513, 514, 0), (1024, 33, 1030, 1026, 1),
                                             (8192, 8, 8192, 8192, 0), (8192, 9, 8192, 8192, 0), (100003, 3, 100003, 100003, 0), (4096, 70001 // 4096 + 1, 4096, 4100, 0)])
def test_own_copy_kernel_bit_exact(hip, m, n, lda, ldb, off):
    """capi_dlacpy(part 0) and capi_memcpy_d2d_async run on the product's own copy kernel (round 4; no hipMemcpy2DAsync / hipMemcpyAsync blits):
    ragged heights, odd leading dimensions, an operand 8 bytes off a 16-byte boundary, contiguous blocks re-cut into 8192-columns with a rest.
    Everything outside the destination block must stay untouched."""
    import torch
    from capital_amd import capi
    torch.manual_seed(m * 31 + n)
    A = torch.rand(lda * n + off + 4, dtype=torch.float64, device="cuda")
    B = torch.full((ldb * n + off + 4,), -7.0, dtype=torch.float64, device="cuda")
    hip.call("capi_dlacpy", 0, m, n, capi.ptr(A) + 8 * off, lda, capi.ptr(B) + 8 * off, ldb)
    hip.sync()
    ref = torch.full_like(B, -7.0)
    Av = A[off:off + lda * n].view(n, lda)
    ref[off:off + ldb * n].view(n, ldb)[:, :m] = Av[:, :m]
    assert torch.equal(B, ref)
    # the contiguous 1-D form
    cnt = lda * n
    D = torch.full((cnt + 6,), 3.0, dtype=torch.float64, device="cuda")
    hip.call("capi_memcpy_d2d_async", capi.ptr(D) + 8 * (1 + off), capi.ptr(A) + 8 * off, 8 * cnt)
    hip.sync()
    ref = torch.full_like(D, 3.0)
    ref[1 + off:1 + off + cnt] = A[off:off + cnt]
    assert torch.equal(D, ref)


# ---- past one workgroup, off-square, padded ------------------------------------------------------------------------------------------------
# The tables (tests/_movement_cases.py) and the numpy references (tests/_movement_ref.py) are held against the oracle on the CPU by
# tests/test_movement_ref.py.  Every source holds pairwise distinct values (k + 0.5), every destination a sentinel (distinct negative values,
# or NaN where the kernel must store and not multiply), and the WHOLE destination buffer is compared bit for bit with the reference applied to
# the same buffer: what lies outside the written set -- padding rows, the other triangle, the guard elements behind the block -- must come back
# as it went in.  Not reached: the column stride loops of trizero, block_cyclic_tri and cyclic_to_local, which need a square of order above
# 65535 (34 GB); triangular serialize shapes on non-square ranges, which the reference does not define.
EINVAL = -1


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _serialize_on_device(hip, c, entry):
    from capital_amd import capi
    src, dst = mc.distinct(c["src_len"]), mc.sentinel(c["dst_len"])
    dsrc, ddst = _dev(src), _dev(dst)
    args = (c["ss"], c["ds"], capi.ptr(dsrc), c["sdimX"], c["sdimY"], capi.ptr(ddst), c["ddimX"], c["ddimY"]) + tuple(c["ranges"])
    hip.call(entry, *(((c["shape"],) if entry == "capi_serialize_shape" else ()) + args))
    hip.sync()
    assert mc.same_bits(_host(ddst), mc.serialize_reference(c, src, dst))
    assert mc.same_bits(_host(dsrc), src)


@pytest.mark.parametrize("r", mc.SERIALIZE_ORDERS)
@pytest.mark.parametrize("ss,ds", mc.SERIALIZE_PAIRS)
def test_serialize_lanes_and_workgroups(hip, ss, ds, r):
    """capi_serialize, the seven pairs on a diagonal sub-range of order r: 257 rows bring in lanes q = 1 (1025: all four and workgroup 1, 2051:
    workgroup 2), and a triangle's diagonal crosses the workgroup boundaries"""
    _serialize_on_device(hip, mc.serialize_case(ss, ds, r), "capi_serialize")


@pytest.mark.parametrize("name", sorted(mc.SERIALIZE_SHAPE_CASES))
def test_serialize_shape_callers_forms(hip, name):
    """capi_serialize_shape as summa.h (pack_tri / unpack_tri) and cholinv.h (pack_piece / unpack_piece, the unpacking of R11^-1's blocks) call
    it: a rect side with a leading dimension above the range, whose entries outside the shape must stay; a rect copy and two triangular
    copies out of sub-ranges of one packed triangle; 65539 columns of three rows (the column stride loop)"""
    _serialize_on_device(hip, mc.SERIALIZE_SHAPE_CASES[name], "capi_serialize_shape")


def test_serialize_empty_and_unequal_ranges(hip):
    from capital_amd import capi
    src, dst = mc.distinct(81), mc.sentinel(81)
    dsrc, ddst = _dev(src), _dev(dst)
    head = (capi.ptr(dsrc), 9, 9, capi.ptr(ddst), 9, 9)
    for ss, ds in ((0, 0), (0, 1), (2, 0)):
        assert hip.L.capi_serialize(hip.h, ss, ds, *head, 2, 2, 0, 5, 3, 3, 0, 5) == 0                        # sex == ssx
        assert hip.L.capi_serialize_shape(hip.h, 0, ss, ds, *head, 0, 5, 4, 4, 0, 5, 1, 1) == 0                # sey == ssy
        assert hip.L.capi_serialize(hip.h, ss, ds, *head, 0, 5, 0, 5, 0, 4, 0, 5) == EINVAL
        assert "ranges differ" in hip.L.capi_last_error(hip.h).decode()
        assert hip.L.capi_serialize_shape(hip.h, 0, ss, ds, *head, 0, 5, 0, 5, 0, 5, 1, 5) == EINVAL
    hip.sync()
    assert mc.same_bits(_host(ddst), dst) and mc.same_bits(_host(dsrc), src)


def _lacpy_operands(part, m, n, lda, ldb):
    """A holds NaN wherever the part does not read it (the other triangle and the padding rows), B its sentinel"""
    A, B = mc.distinct(lda * n + 4), mc.sentinel(ldb * n + 4)
    Av = A[:lda * n].reshape(n, lda)
    Av[:, m:] = np.nan
    Av[:, :m][~mref.part_mask(part, m, n)] = np.nan
    return A, B


@pytest.mark.parametrize("part", (1, 2))
@pytest.mark.parametrize("m,n,lda,ldb", mc.LACPY_CASES)
def test_lacpy_triangles_padded(hip, part, m, n, lda, ldb):
    from capital_amd import capi
    A, B = _lacpy_operands(part, m, n, lda, ldb)
    dA, dB = _dev(A), _dev(B)
    hip.call("capi_dlacpy", part, m, n, capi.ptr(dA), lda, capi.ptr(dB), ldb)
    hip.sync()
    want = mref.lacpy(part, m, n, A, lda, B, ldb)
    assert not np.isnan(want).any()
    assert mc.same_bits(_host(dB), want)


def test_lacpy_triangle_wider_than_the_launch(hip):
    """part 1 on 524288 columns of one row: 65536 groups of eight columns, one more than the grid's y holds.  The call may do the copy or
    refuse it (CAPI_EINVAL, B untouched -- what it does today); it may not copy a part and report success."""
    from capital_amd import capi
    m, n = mc.LACPY_WIDE
    A, B = _lacpy_operands(1, m, n, m, m)
    dA, dB = _dev(A), _dev(B)
    rc = hip.L.capi_dlacpy(hip.h, 1, m, n, capi.ptr(dA), m, capi.ptr(dB), m)
    hip.sync()
    assert rc in (0, EINVAL)
    assert mc.same_bits(_host(dB), mref.lacpy(1, m, n, A, m, B, m) if rc == 0 else B)


@pytest.mark.parametrize("keep", (0, 1))
@pytest.mark.parametrize("n", mc.TRIZERO_ORDERS)
def test_trizero_padded(hip, n, keep):
    """capi_dtrizero with lda = n + 3 (cacqr.h zeroes a k x k corner of an n x n matrix): NaN in the triangle that goes becomes +0.0; the
    diagonal, the kept triangle and the padding rows stay bit for bit"""
    from capital_amd import capi
    lda = n + 3
    A = mc.distinct(lda * n + 4)
    A[:lda * n].reshape(n, lda)[:, :n][~mref.part_mask(1 if keep else 2, n, n)] = np.nan
    dA = _dev(A)
    hip.call("capi_dtrizero", keep, n, capi.ptr(dA), lda)
    hip.sync()
    want = mref.trizero(keep, n, A, lda)
    assert not np.isnan(want).any()
    assert mc.same_bits(_host(dA), want)


@pytest.mark.parametrize("dimX,dimY", mc.REMOVE_TRIANGLE_SHAPES)
def test_remove_triangle_rectangular(hip, dimX, dimY):
    """capi_remove_triangle on rectangular pieces (index i * dimY + j) of 1 x 1, 2 x 2 and 3 x 3 grids, both directions: NaN in the removed
    region becomes 0.0, the kept region stays; 65538 local columns enter the column stride loop"""
    from capital_amd import capi
    for dr, P, px, py in mc.remove_triangle_grids(dimX):
        A = mc.distinct(dimX * dimY + 4)
        A[:dimX * dimY].reshape(dimX, dimY)[mref.remove_triangle_mask(dr, dimX, dimY, px, py, P)] = np.nan
        dA = _dev(A)
        hip.call("capi_remove_triangle", dr.encode(), capi.ptr(dA), dimX, dimY, px, py, P)
        hip.sync()
        want = mref.remove_triangle(dr, A, dimX, dimY, px, py, P)
        assert not np.isnan(want).any()
        assert mc.same_bits(_host(dA), want), (dr, P, px, py)


@pytest.mark.parametrize("rl,cl,d", mc.BLOCK_CYCLIC_CASES)
def test_block_cyclic_rectangular(hip, rl, cl, d):
    """capi_block_to_cyclic, capi_block_to_cyclic_full (cholinv.h: the gathered R12 pieces, L1 != L2) and capi_cyclic_to_block on rl != cl,
    past 256 aggregate rows and past 65535 aggregate columns: every entry of a NaN destination is written, and full -> to_block is the identity"""
    from capital_amd import capi
    blocked = mc.distinct(rl * cl * d * d)
    nan = np.full(blocked.size, np.nan)
    db, dcyc, dfull = _dev(blocked), _dev(nan), _dev(nan)
    hip.call("capi_block_to_cyclic", capi.ptr(db), capi.ptr(dcyc), rl, cl, d)
    hip.call("capi_block_to_cyclic_full", capi.ptr(db), capi.ptr(dfull), rl, cl, d)
    hip.sync()
    assert mc.same_bits(_host(dcyc), mref.block_to_cyclic(1, blocked, rl, cl, d))
    assert mc.same_bits(_host(dfull), mref.block_to_cyclic(2, blocked, rl, cl, d))
    assert mc.same_bits(_host(db), blocked)
    cyc = mc.distinct(blocked.size, 0.75)
    dsrc, dback, dtrip = _dev(cyc), _dev(nan), _dev(nan)
    hip.call("capi_cyclic_to_block", capi.ptr(dback), capi.ptr(dsrc), rl, cl, d)
    hip.call("capi_cyclic_to_block", capi.ptr(dtrip), capi.ptr(dfull), rl, cl, d)
    hip.sync()
    assert mc.same_bits(_host(dback), mref.cyclic_to_block(cyc, rl, cl, d))
    assert mc.same_bits(_host(dtrip), blocked)


@pytest.mark.parametrize("rl,d", mc.BLOCK_CYCLIC_TRI_CASES)
def test_block_cyclic_triangle_past_one_workgroup(hip, rl, d):
    """the assertions of test_block_cyclic_triangle at aggregate orders 258 and 300 (workgroup 1 along the row index)"""
    from capital_amd import capi
    psz = rl * (rl + 1) // 2
    blocked = mc.distinct(psz * d * d)
    db, dc = _dev(blocked), _dev(np.full((rl * d) ** 2, np.nan))                  # every entry of the aggregate must be written
    hip.call("capi_block_to_cyclic_tri", capi.ptr(db), capi.ptr(dc), rl, d)
    hip.sync()
    cyc = _host(dc)
    assert mc.same_bits(cyc, mref.block_to_cyclic_tri(blocked, rl, d))
    db2 = _dev(np.full(blocked.size, np.nan))                                     # every packed entry must be written
    hip.call("capi_cyclic_to_block_tri", capi.ptr(db2), capi.ptr(dc), rl, d)
    hip.sync()
    got = _host(db2)
    assert mc.same_bits(got, mref.cyclic_to_block_tri(cyc, rl, d))
    changed = np.nonzero(got != blocked)[0]
    assert len(changed) == rl * (d * (d - 1) // 2) and np.all(got[changed] == 0.0)   # local diagonals of the pieces with y > x
    full = mc.distinct(cyc.size, 0.75)                                            # an aggregate with values below its diagonal: they must not travel
    db3, dfull = _dev(np.full(blocked.size, np.nan)), _dev(full)
    hip.call("capi_cyclic_to_block_tri", capi.ptr(db3), capi.ptr(dfull), rl, d)
    hip.sync()
    assert mc.same_bits(_host(db3), mref.cyclic_to_block_tri(full, rl, d))


@pytest.mark.parametrize("L,d,bc", mc.CYCLIC_TO_LOCAL_CASES)
def test_cyclic_to_local_padded(hip, L, d, bc):
    """capi_cyclic_to_local past 256 rows and with bc_dim > local_dim * d: the leading L x L corner of T and TI against the reference, and every
    entry outside that corner as it went in (the kernel writes nothing else)"""
    from capital_amd import capi
    T, TI = mc.distinct(bc * bc), mc.sentinel(bc * bc)
    for sr in mc.slice_ranks(L, d):
        dT, dTI = _dev(T), _dev(TI)
        hip.call("capi_cyclic_to_local", capi.ptr(dT), capi.ptr(dTI), L, bc, d, sr)
        hip.sync()
        for got, src in ((_host(dT), T), (_host(dTI), TI)):
            want = mref.cyclic_to_local(src, L, bc, d, sr)
            assert mc.same_bits(got.reshape(bc, bc)[:L, :L], want.reshape(bc, bc)[:L, :L]), sr
            assert mc.same_bits(got, want), sr


def _offset_block(block, off):
    """the (n, ld) image behind `off` NaN elements of a larger allocation, four more behind it: (flat buffer, byte offset of the block)"""
    return np.concatenate([np.full(off, np.nan), block.reshape(-1), np.full(4, np.nan)]), 8 * off


def _diff_norms_on_device(hip, part, m, n, X, Y):
    import ctypes as C
    from capital_amd import capi
    (bx, ox), (by, oy) = _offset_block(X, 5), _offset_block(Y, 3)
    dX, dY = _dev(bx), _dev(by)
    out = (C.c_double * 2)(-1.0, -1.0)
    hip.call("capi_diff_norms", part, m, n, capi.ptr(dX) + ox, X.shape[1], capi.ptr(dY) + oy, Y.shape[1], out)
    return out[0], out[1]


@pytest.mark.parametrize("part", (0, 1, 2))
@pytest.mark.parametrize("m,n", mc.DIFF_NORMS_SHAPES)
def test_diff_norms_bound(hip, part, m, n):
    """capi_diff_norms as validate.h calls it (parts 0 and 1, padded leading dimensions, pointers into a larger allocation), NaN in the padding
    rows and in the excluded triangle, against sums formed and added exactly.  All terms are non-negative, so every rounding is a relative
    one: 2 for x - y under the square and 1 for each product (the + 4 covers them), ceil(m / 256) serial adds per thread, the 8 levels of
    the workgroup's tree, n adds on the host:  |got - exact| <= (ceil(m / 256) + 8 + n + 4) 2^-53 exact  -- derived, not measured; 3e-14 of
    the sum at the largest shape, where one dropped element moves it by 1e-5."""
    rng = np.random.default_rng(1000 * m + 10 * n + part)
    sel = mref.part_mask(part, m, n)
    X, Y = np.full((n, m + 3), np.nan), np.full((n, m + 7), np.nan)
    X[:, :m][sel], Y[:, :m][sel] = rng.uniform(-1, 1, size=int(sel.sum())), rng.uniform(-1, 1, size=int(sel.sum()))
    got = _diff_norms_on_device(hip, part, m, n, X, Y)
    exact = mref.diff_norms(part, X[:, :m], Y[:, :m])
    k = -(-m // 256) + 8 + n + 4
    for g, e, what in zip(got, exact, ("sum (x - y)^2", "sum y^2")):
        err = abs(np.longdouble(g) - e)
        print(f"diff_norms part {part} {m} x {n} {what}: got {g!r} err {float(err / e):.3e} bound {k * 2.0 ** -53:.3e}")
        assert e > 0 and err <= k * np.longdouble(2.0) ** -53 * e


@pytest.mark.parametrize("part", (0, 1, 2))
@pytest.mark.parametrize("m,n", mc.DIFF_NORMS_SHAPES)
def test_diff_norms_sees_every_element_of_its_part(hip, part, m, n):
    """X == Y but for one element, off by 2^-3: the first sum is 2^-6 exactly when that element lies in the part and 0.0 exactly when it does
    not -- at the corners, on both sides of the thread stride (rows 255, 256), on the diagonal and right above and below it.  The entries
    are multiples of 0.5 below 64, so the second sum is exact in any order and must equal the part's sum of squares."""
    i, j = np.arange(m)[None, :], np.arange(n)[:, None]
    base = ((7 * i + 13 * j) % 64 + 0.5).astype(np.float64)
    sel = mref.part_mask(part, m, n)
    delta = 0.125
    for pi, pj in mc.diff_norms_positions(m, n):
        X, Y = np.full((n, m + 3), np.nan), np.full((n, m + 7), np.nan)
        X[:, :m][sel] = Y[:, :m][sel] = base[sel]
        X[pj, pi], Y[pj, pi] = base[pj, pi] + delta, base[pj, pi]
        e, c = _diff_norms_on_device(hip, part, m, n, X, Y)
        inside = mc.in_part(part, pi, pj)
        assert e == (delta * delta if inside else 0.0), (pi, pj, inside, e)
        assert c == float((base[sel] ** 2).sum()), (pi, pj, c)


@pytest.mark.parametrize("gen,gx,gy,px,py,P", [("symmetric", 65538, 2, 0, 0, 1), ("identity", 65538, 3, 0, 0, 1), ("random", 2 * 65538 - 1, 3, 1, 1, 2)])
def test_generators_past_65535_local_columns(hip, oracle, gen, gx, gy, px, py, P):
    """the generators' column stride loops: 65538 local columns; the random piece is the last of a 2 x 2 grid on odd global dims, 65538 x 2
    with a trailing padding column AND row (gen_pad_zero_kernel's loop)"""
    from capital_amd import capi
    if gen == "symmetric":
        ref = oracle.distribute_symmetric(gx, gy, px, py, P, P, key=7)
    elif gen == "identity":
        ref = oracle.distribute_identity(gx, gy, px, py, P, P, -2.5)
    else:
        ref = oracle.distribute_random(gx, gy, px, py, P, P, key=3)
    dy, dx = ref.shape
    assert dx == 65538 and (gen != "random" or (dy == 2 and not ref[:, -1].any() and not ref[-1].any() and ref[0, :-1].all()))
    dev = capi.to_device(np.full((dy, dx), np.nan))
    tail = {"symmetric": (7, 1), "identity": (-2.5,), "random": (3,)}[gen]
    hip.call("capi_distribute_" + gen, capi.ptr(dev), dx, dy, gx, gy, px, py, P, P, *tail)
    hip.sync()
    assert mc.same_bits(capi.to_host(dev), ref)


@pytest.mark.parametrize("gx,gy,P,px,py", [(101, 101, 2, 0, 0), (101, 101, 2, 1, 0), (101, 101, 2, 0, 1), (101, 101, 2, 1, 1), (7, 300, 1, 0, 0), (300, 7, 1, 0, 0),
                                           (7, 300, 2, 1, 1), (300, 7, 2, 0, 0)])
def test_distribute_identity_pieces(hip, oracle, gx, gy, P, px, py):
    """every piece of a 2 x 2 grid (the off-diagonal ones hold no diagonal entry), non-square global dims, a negative value"""
    from capital_amd import capi
    ref = oracle.distribute_identity(gx, gy, px, py, P, P, -3.5)
    dy, dx = ref.shape
    assert (ref != 0).any() == (px == py)
    dev = capi.to_device(np.full((dy, dx), np.nan))
    hip.call("capi_distribute_identity", capi.ptr(dev), dx, dy, gx, gy, px, py, P, P, -3.5)
    hip.sync()
    assert mc.same_bits(capi.to_host(dev), ref)


@pytest.mark.parametrize("beta", mc.AXPBY_BETAS)
@pytest.mark.parametrize("count", mc.AXPBY_COUNTS)
def test_axpby_whole_vector(hip, count, beta):
    """capi_daxpby's grid-stride loop (3 000 001 elements: more than 16 workgroups of 256 per CU on any CU count of this part), the whole
    vector bit for bit.  beta is a power of two (or zero), so beta * y is exact and the kernel's fused multiply-add rounds as numpy's two
    operations do.  Four guard elements behind `count` stay."""
    from capital_amd import capi
    x, y = mc.distinct(count + 4), mc.sentinel(count + 4)
    dx, dy = _dev(x), _dev(y)
    hip.call("capi_daxpby", count, beta, capi.ptr(dx), capi.ptr(dy))
    hip.sync()
    want = y.copy()
    want[:count] = beta * y[:count] + x[:count]
    assert mc.same_bits(_host(dy), want)
    assert mc.same_bits(_host(dx), x)
