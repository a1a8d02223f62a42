"""Plain numpy references of the data-movement kernels (capital_amd/csrc/movement.hip), written from the index formulas and not from the
kernels' loops.  numpy only: no ctypes, no torch, no GPU.  Everything is vectorised: no Python loop runs per element.

Conventions: a matrix is a FLAT float64 array, column-major with a leading dimension (element (row i, column j) at i + j * ld), or in one of
the three layouts of structure.h addressed by (x = column, y = row).  Every function returns a NEW array and leaves its arguments alone.
tests/test_movement_ref.py holds these against the oracle's loop-for-loop restatement, bit for bit."""
import math

import numpy as np

RECT, UPPERTRI, LOWERTRI = 0, 1, 2
KEEP_LOWER, KEEP_UPPER = 0, 1


def offset(st, x, y, dimY):
    """structure.h:13 (rect), :39 (packed upper), :59 (packed lower); x = column, y = row, scalars or int64 arrays"""
    x, y = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    if st == RECT:
        return x * dimY + y
    if st == UPPERTRI:
        return x * (x + 1) // 2 + y
    return x * dimY + y - x * (x + 1) // 2


def packed_len(st, dimX, dimY=None):
    dimY = dimX if dimY is None else dimY
    return dimX * dimY if st == RECT else dimX * (dimX + 1) // 2


def derived_shape(ss, ds):
    """the copy shape of serialize<S1, S2>: lower if either side is lower, else upper if either is upper, else rect"""
    return LOWERTRI if LOWERTRI in (ss, ds) else (UPPERTRI if UPPERTRI in (ss, ds) else RECT)


def serialize_indices(shape, ss, ds, sdimY, ddimY, ssx, sex, ssy, sey, dsx, dex, dsy, dey):
    """(source offsets, destination offsets) of every element the copy moves.  Column i of the range moves rangeY elements (rect), the
    i + 1 elements from the range's first row (upper), or the rangeY - i elements from the diagonal on (lower)."""
    rx, ry = sex - ssx, sey - ssy
    assert rx == dex - dsx and ry == dey - dsy
    if rx <= 0 or ry <= 0:
        e = np.zeros(0, dtype=np.int64)
        return e, e
    i = np.arange(rx, dtype=np.int64)
    cnt = np.full(rx, ry, dtype=np.int64) if shape == RECT else (i + 1 if shape == UPPERTRI else ry - i)
    first = i if shape == LOWERTRI else np.zeros(rx, dtype=np.int64)            # first row of column i, relative to the range
    col = np.repeat(i, cnt)
    t = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    row = np.repeat(first, cnt)
    so = offset(ss, ssx + col, ssy + row, sdimY) + t
    do = offset(ds, dsx + col, dsy + row, ddimY) + t
    return so, do


def serialize_shape(shape, ss, ds, src, sdimY, dst, ddimY, ssx, sex, ssy, sey, dsx, dex, dsy, dey):
    so, do = serialize_indices(shape, ss, ds, sdimY, ddimY, ssx, sex, ssy, sey, dsx, dex, dsy, dey)
    out = dst.copy()
    out[do] = src[so]
    return out


def serialize(ss, ds, src, sdimY, dst, ddimY, *ranges):
    return serialize_shape(derived_shape(ss, ds), ss, ds, src, sdimY, dst, ddimY, *ranges)


def part_mask(part, m, n):
    """[j, i] (column first, like the flat column-major image reshaped to (n, ld)): part 0 all, 1 i <= j, 2 i >= j"""
    i, j = np.arange(m, dtype=np.int64)[None, :], np.arange(n, dtype=np.int64)[:, None]
    return np.ones((n, m), dtype=bool) if part == 0 else (i <= j if part == 1 else i >= j)


def lacpy(part, m, n, A, lda, B, ldb):
    out = B.copy()
    Av, Bv = A[:lda * n].reshape(n, lda)[:, :m], out[:ldb * n].reshape(n, ldb)[:, :m]
    sel = part_mask(part, m, n)
    Bv[sel] = Av[sel]
    return out


def trizero(keep, n, A, lda):
    out = A.copy()
    out[:lda * n].reshape(n, lda)[:, :n][~part_mask(1 if keep == KEEP_UPPER else 2, n, n)] = 0.0
    return out


def remove_triangle_mask(direction, dimX, dimY, px, py, P):
    """[i, j] (local column, local row): True where the entry is REMOVED; global column gx = px + i P, global row gy = py + j P"""
    gx = px + np.arange(dimX, dtype=np.int64)[:, None] * P
    gy = py + np.arange(dimY, dtype=np.int64)[None, :] * P
    return gy > gx if direction == "U" else gy < gx


def remove_triangle(direction, A, dimX, dimY, px, py, P):
    out = A.copy()
    out[:dimX * dimY].reshape(dimX, dimY)[remove_triangle_mask(direction, dimX, dimY, px, py, P)] = 0.0
    return out


def _zero_below(cyc2):
    """cyc2[gcol, grow]: zero grow > gcol"""
    cg, rg = cyc2.shape
    cyc2[np.arange(rg, dtype=np.int64)[None, :] > np.arange(cg, dtype=np.int64)[:, None]] = 0.0


def block_to_cyclic(mode, blocked, rl, cl, d):
    """cyclic[(i d + x) rg + (k d + y)] = blocked[(y d + x) rl cl + i rl + k]; mode 1 zeroes grow > gcol, mode 2 zeroes nothing"""
    cyc = np.ascontiguousarray(blocked.reshape(d, d, cl, rl).transpose(2, 1, 3, 0)).reshape(cl * d, rl * d)     # [y, x, i, k] -> [i, x, k, y]
    if mode == 1:
        _zero_below(cyc)
    return cyc.reshape(-1)


def cyclic_to_block(cyclic, rl, cl, d):
    return np.ascontiguousarray(cyclic.reshape(cl, d, rl, d).transpose(3, 1, 0, 2)).reshape(-1)                # [i, x, k, y] -> [y, x, i, k]


def _tri_index(rl):
    """(i, k, packed offset i (i + 1) / 2 + k) of the rl (rl + 1) / 2 entries of a packed upper piece: local column i, local row k <= i"""
    i = np.repeat(np.arange(rl, dtype=np.int64), np.arange(1, rl + 1))
    k = np.arange(i.size, dtype=np.int64) - i * (i + 1) // 2
    return i, k, i * (i + 1) // 2 + k


def block_to_cyclic_tri(blocked, rl, d):
    """packed-upper pieces -> aggregate: local (column i, row k <= i) of piece (x, y) is global (i d + x, k d + y); everything below the
    aggregate's diagonal (and below every piece's packed triangle) is zero"""
    i, k, p = _tri_index(rl)
    dense = np.zeros((d, d, rl, rl))
    dense[:, :, i, k] = blocked.reshape(d, d, -1)[:, :, p]
    return block_to_cyclic(1, dense.reshape(-1), rl, rl, d)


def cyclic_to_block_tri(cyclic, rl, d):
    """aggregate -> packed-upper pieces; packed entries below the aggregate's diagonal (k == i, y > x) become zero"""
    cyc = cyclic.reshape(rl * d, rl * d).copy()
    _zero_below(cyc)
    i, k, p = _tri_index(rl)
    out = np.empty((d, d, rl * (rl + 1) // 2))
    out[:, :, p] = cyclic_to_block(cyc.reshape(-1), rl, rl, d).reshape(d, d, rl, rl)[:, :, i, k]
    return out.reshape(-1)


def cyclic_to_local(M, L, bc, d, sr):
    """one matrix of util::cyclic_to_local: corner (column i, row j) <- M(column i d + sr % d, row j d + sr / d) where that lies on or above
    the global diagonal, else 0; the rest of the bc x bc image stays"""
    ro, co = sr // d, sr % d
    Mv = M.reshape(bc, bc)
    out = Mv.copy()
    rc = np.arange(L, dtype=np.int64)[:, None] * d + co
    rr = np.arange(L, dtype=np.int64)[None, :] * d + ro
    out[:L, :L] = np.where(rc >= rr, Mv[co:co + (L - 1) * d + 1:d, ro:ro + (L - 1) * d + 1:d], 0.0)
    return out.reshape(-1)


def _exact_sum(terms):
    """sum of long-double terms as a long double good to far below a double ulp: each term split into two doubles, math.fsum (exact,
    correctly rounded) for the head, and again for what the head left over"""
    hi = terms.astype(np.float64)
    lo = (terms - hi).astype(np.float64)
    parts = hi.tolist() + lo.tolist()
    head = math.fsum(parts)
    return np.longdouble(head) + np.longdouble(math.fsum(parts + [-head]))


def diff_norms(part, X, Y):
    """(sum (x - y)^2, sum y^2) over the part of the m x n blocks X, Y given as [j, i] arrays (n, m).  With an 80-bit long double every
    difference of two doubles of like magnitude and every product carries a relative error of 2^-64 at most, 2048 times below a double's;
    without one (long double == double) the terms are formed in rational arithmetic."""
    n, m = X.shape
    sel = part_mask(part, m, n)
    x, y = X[sel], Y[sel]
    if np.finfo(np.longdouble).nmant >= 63:
        xl, yl = x.astype(np.longdouble), y.astype(np.longdouble)
        return _exact_sum((xl - yl) * (xl - yl)), _exact_sum(yl * yl)
    from fractions import Fraction
    e = sum(((Fraction(a) - Fraction(b)) ** 2 for a, b in zip(x.tolist(), y.tolist())), Fraction(0))
    c = sum((Fraction(b) ** 2 for b in y.tolist()), Fraction(0))
    return np.longdouble(float(e)), np.longdouble(float(c))
