"""CPU: the numpy references of tests/test_gpu_movement.py (tests/_movement_ref.py) against the oracle's loop-for-loop restatement of the
reference's serialize.hpp and util.hpp, bit for bit, at every case of the GPU tables (tests/_movement_cases.py) that the oracle covers --
so that the device tests compare against formulas that are themselves held to the reference's loops, rectangular pieces included."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import _movement_cases as mc
import _movement_ref as ref

_dp = C.POINTER(C.c_double)


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_dp)


def _orc_serialize(oracle, c, src, dst):
    out = dst.copy()
    oracle.lib().orc_serialize(c["ss"], c["ds"], _p(src), c["sdimX"], c["sdimY"], _p(out), c["ddimX"], c["ddimY"], *c["ranges"])
    return out


def test_offset_matches_the_oracle(oracle):
    for st in (0, 1, 2):
        for dimY in (7, 12):
            for x in range(7):
                for y in range(7):
                    assert int(ref.offset(st, x, y, dimY)) == oracle.lib().orc_offset(st, x, y, 7, dimY)
    x = np.arange(5, dtype=np.int64)
    assert ref.offset(2, x, x + 1, 9).tolist() == [int(ref.offset(2, int(v), int(v) + 1, 9)) for v in x]


@pytest.mark.parametrize("r", mc.SERIALIZE_ORDERS)
@pytest.mark.parametrize("ss,ds", mc.SERIALIZE_PAIRS)
def test_serialize_pairs(oracle, ss, ds, r):
    c = mc.serialize_case(ss, ds, r)
    src, dst = mc.distinct(c["src_len"]), mc.sentinel(c["dst_len"])
    got = mc.serialize_reference(c, src, dst)
    assert mc.same_bits(got, _orc_serialize(oracle, c, src, dst))
    so, do = ref.serialize_indices(c["shape"], ss, ds, c["sdimY"], c["ddimY"], *c["ranges"])
    assert so.size == (r * r if c["shape"] == 0 else r * (r + 1) // 2) and np.unique(do).size == do.size          # every element once
    assert 0 <= so.min() and so.max() < c["src_len"] and 0 <= do.min() and do.max() < c["dst_len"]


@pytest.mark.parametrize("name", sorted(mc.SERIALIZE_SHAPE_CASES))
def test_serialize_shape_forms(oracle, name):
    """the callers' forms: against the oracle where the copy shape is the one the structures imply; the rect copy out of a packed triangle,
    which the reference has no specialisation for, against the definition, column by column"""
    c = mc.SERIALIZE_SHAPE_CASES[name]
    src, dst = mc.distinct(c["src_len"]), mc.sentinel(c["dst_len"])
    got = mc.serialize_reference(c, src, dst)
    so, do = ref.serialize_indices(c["shape"], c["ss"], c["ds"], c["sdimY"], c["ddimY"], *c["ranges"])
    assert 0 <= so.min() and so.max() < c["src_len"] and 0 <= do.min() and do.max() < c["dst_len"] and np.unique(do).size == do.size
    if c["oracle"]:
        assert ref.derived_shape(c["ss"], c["ds"]) == c["shape"]
        assert mc.same_bits(got, _orc_serialize(oracle, c, src, dst))
    else:
        ssx, sex, ssy, sey, dsx, dex, dsy, dey = c["ranges"]
        want = dst.copy()
        for i in range(sex - ssx):
            s0 = oracle.lib().orc_offset(c["ss"], ssx + i, ssy, c["sdimX"], c["sdimY"])
            d0 = oracle.lib().orc_offset(c["ds"], dsx + i, dsy, c["ddimX"], c["ddimY"])
            want[d0:d0 + sey - ssy] = src[s0:s0 + sey - ssy]
        assert mc.same_bits(got, want)


def test_serialize_empty_range_moves_nothing():
    dst = mc.sentinel(50)
    assert mc.same_bits(ref.serialize_shape(0, 0, 0, mc.distinct(50), 7, dst, 7, 2, 2, 0, 5, 1, 1, 0, 5), dst)


@pytest.mark.parametrize("rl,cl,d", mc.BLOCK_CYCLIC_CASES)
def test_block_cyclic_rect(oracle, rl, cl, d):
    blocked = mc.distinct(rl * cl * d * d)
    want = np.full(blocked.size, np.nan)
    oracle.lib().orc_block_to_cyclic_rect(_p(blocked), _p(want), rl, cl, d)
    assert mc.same_bits(ref.block_to_cyclic(1, blocked, rl, cl, d), want)
    full = ref.block_to_cyclic(2, blocked, rl, cl, d)
    rg = rl * d
    gcol, grow = np.indices((cl * d, rl * d))
    assert mc.same_bits(np.where(grow > gcol, 0.0, full.reshape(cl * d, rg)).reshape(-1), want)                  # mode 2 is mode 1 without the zeroing ...
    assert np.array_equal(np.sort(full), blocked)                                                             # ... and a permutation
    cyc = mc.distinct(blocked.size, 0.75)
    back = np.full(blocked.size, np.nan)
    oracle.lib().orc_cyclic_to_block_rect(_p(back), _p(cyc), rl, cl, d)
    assert mc.same_bits(ref.cyclic_to_block(cyc, rl, cl, d), back)
    assert mc.same_bits(ref.cyclic_to_block(full, rl, cl, d), blocked)


@pytest.mark.parametrize("rl,d", mc.BLOCK_CYCLIC_TRI_CASES + [(8, 2), (5, 3), (16, 1)])
def test_block_cyclic_triangle(oracle, rl, d):
    psz = rl * (rl + 1) // 2
    blocked = mc.distinct(psz * d * d)
    want = np.full((rl * d) ** 2, np.nan)
    oracle.lib().orc_block_to_cyclic_triangle(_p(blocked), _p(want), blocked.size, rl, rl, d)
    got = ref.block_to_cyclic_tri(blocked, rl, d)
    assert mc.same_bits(got, want)
    cyc = mc.distinct(want.size, 0.75)                       # a full aggregate: what lies below its diagonal must not reach the pieces
    back = np.full(blocked.size, np.nan)
    oracle.lib().orc_cyclic_to_block_triangle(_p(back), _p(cyc), blocked.size, rl, rl, d)
    assert mc.same_bits(ref.cyclic_to_block_tri(cyc, rl, d), back)
    trip = ref.cyclic_to_block_tri(got, rl, d)
    changed = np.nonzero(trip != blocked)[0]
    assert len(changed) == rl * (d * (d - 1) // 2) and np.all(trip[changed] == 0.0)


@pytest.mark.parametrize("L,d,bc", mc.CYCLIC_TO_LOCAL_CASES)
def test_cyclic_to_local(oracle, L, d, bc):
    T, TI = mc.distinct(bc * bc), mc.sentinel(bc * bc)
    for sr in mc.slice_ranks(L, d):
        wT, wTI = T.copy(), TI.copy()
        oracle.lib().orc_cyclic_to_local(_p(wT), _p(wTI), L, bc, d, sr)
        assert mc.same_bits(ref.cyclic_to_local(T, L, bc, d, sr), wT)
        assert mc.same_bits(ref.cyclic_to_local(TI, L, bc, d, sr), wTI)


@pytest.mark.parametrize("m,n,lda,ldb", [(1, 1, 1, 1), (5, 9, 7, 6), (9, 5, 9, 12), (23, 29, 26, 25)])
def test_lacpy_trizero_by_loops(m, n, lda, ldb):
    A, B = mc.distinct(lda * n + 2), mc.sentinel(ldb * n + 2)
    for part in (0, 1, 2):
        want = B.copy()
        for j in range(n):
            for i in range(m):
                if mc.in_part(part, i, j):
                    want[i + j * ldb] = A[i + j * lda]
        assert mc.same_bits(ref.lacpy(part, m, n, A, lda, B, ldb), want)
    for keep in (0, 1):
        want = A.copy()
        for j in range(min(m, n)):
            for i in range(min(m, n)):
                if (i > j) if keep else (i < j):
                    want[i + j * lda] = 0.0
        assert mc.same_bits(ref.trizero(keep, min(m, n), A, lda), want)


@pytest.mark.parametrize("dimX,dimY", [(7, 11), (11, 7)])
def test_remove_triangle_by_loops(dimX, dimY):
    A = mc.distinct(dimX * dimY + 3)
    for dr, P, px, py in mc.remove_triangle_grids(dimX):
        want = A.copy()
        for i in range(dimX):
            for j in range(dimY):
                gx, gy = px + i * P, py + j * P
                if (gy > gx) if dr == "U" else (gy < gx):
                    want[i * dimY + j] = 0.0
        assert mc.same_bits(ref.remove_triangle(dr, A, dimX, dimY, px, py, P), want)


@pytest.mark.parametrize("part", (0, 1, 2))
def test_diff_norms_is_exact(part):
    """against a double loop in rational arithmetic: the reference is good to 2^-60 relative, 128 times below a double's unit roundoff"""
    rng = np.random.default_rng(5 + part)
    m, n = 23, 17
    X, Y = rng.uniform(-1, 1, size=(n, m)), rng.uniform(-1, 1, size=(n, m)) * np.exp2(rng.integers(-6, 6, size=(n, m)))
    e = c = Fraction(0)
    for j in range(n):
        for i in range(m):
            if mc.in_part(part, i, j):
                e += (Fraction(float(X[j, i])) - Fraction(float(Y[j, i]))) ** 2
                c += Fraction(float(Y[j, i])) ** 2
    ge, gc = ref.diff_norms(part, X, Y)
    for got, want in ((ge, e), (gc, c)):
        hi = float(got)
        frac = Fraction(hi) + Fraction(float(got - np.longdouble(hi)))
        assert abs(frac - want) <= want * Fraction(1, 2 ** 60)


def test_tables_reach_the_paths_they_are_named_for():
    assert max(mc.SERIALIZE_ORDERS) > 2048 and 1025 in mc.SERIALIZE_ORDERS and 257 in mc.SERIALIZE_ORDERS
    assert mc.SERIALIZE_SHAPE_CASES["wide_rect"]["ranges"][1] > 65535
    assert any(rl != cl for rl, cl, _ in mc.BLOCK_CYCLIC_CASES) and any(cl * d > 65535 for _, cl, d in mc.BLOCK_CYCLIC_CASES)
    assert any(bc > L * d for L, d, bc in mc.CYCLIC_TO_LOCAL_CASES) and any(L > 256 for L, _, _ in mc.CYCLIC_TO_LOCAL_CASES)
    assert (mc.LACPY_WIDE[1] + 7) // 8 > 65535 and max(mc.AXPBY_COUNTS) > 16 * 256 * 256
    for m, n in mc.DIFF_NORMS_SHAPES:
        assert all(0 <= i < m and 0 <= j < n for i, j in mc.diff_norms_positions(m, n))
    assert (255, 20) in mc.diff_norms_positions(700, 40) and (256, 20) in mc.diff_norms_positions(700, 40)
