"""The case tables and the data of the data-movement tests: tests/test_gpu_movement.py runs them on the device against the numpy references
(tests/_movement_ref.py), tests/test_movement_ref.py holds those references against the oracle at the same cases.  numpy only.

The shapes are the smallest that reach each launch path of capital_amd/csrc/movement.hip: serialize_kernel moves 4 elements per thread, 256
apart, 1024 rows per workgroup (lanes q = 1..3 from 257 rows on, workgroup 1 from 1025, workgroup 2 from 2049); every other kernel has 256
rows per workgroup; the column index is the grid's y, capped at 65535, with a stride loop behind it (entered from 65536 columns on)."""
import numpy as np

import _movement_ref as ref

RECT, U, L = ref.RECT, ref.UPPERTRI, ref.LOWERTRI


def distinct(count, first=0.5):
    """pairwise distinct, exactly representable: k + 0.5"""
    return np.arange(count, dtype=np.float64) + first


def sentinel(count):
    """pairwise distinct, negative, disjoint from distinct(): what a destination holds before the call"""
    return -(np.arange(count, dtype=np.float64) + 0.25)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- capi_serialize: the seven structure pairs on a diagonal sub-range ----------------------------------------------------------------------
SERIALIZE_PAIRS = [(RECT, RECT), (RECT, U), (U, RECT), (U, U), (RECT, L), (L, RECT), (L, L)]
SERIALIZE_ORDERS = (1, 257, 1025, 2051)


def serialize_case(ss, ds, r):
    """source range at (3, 3) in a parent of order r + 9, destination range at (5, 5) in a parent of order r + 7"""
    sn, dn = r + 9, r + 7
    return dict(shape=ref.derived_shape(ss, ds), ss=ss, ds=ds, sdimX=sn, sdimY=sn, ddimX=dn, ddimY=dn, src_len=ref.packed_len(ss, sn), dst_len=ref.packed_len(ds, dn),
                ranges=(3, 3 + r, 3, 3 + r, 5, 5 + r, 5, 5 + r), oracle=True)


# ---- capi_serialize_shape: the callers' forms -----------------------------------------------------------------------------------------------
def _shape_cases():
    out = {}
    for n in (257, 1025):                      # summa.h pack_tri / unpack_tri, cholinv.h pack_piece / unpack_piece: the rect side has ld > n
        for shape, ss, ds in ((U, RECT, U), (U, U, RECT), (L, RECT, L), (L, L, RECT)):
            sy, dy = (n + 3 if ss == RECT else n), (n + 3 if ds == RECT else n)
            out[f"pad_{'ul'[shape - 1]}_{'rul'[ss]}{'rul'[ds]}_{n}"] = dict(
                shape=shape, ss=ss, ds=ds, sdimX=n, sdimY=sy, ddimX=n, ddimY=dy, src_len=ref.packed_len(ss, n, sy), dst_len=ref.packed_len(ds, n, dy),
                ranges=(0, n, 0, n, 0, n, 0, n), oracle=True)
    n, h1 = 1300, 1030                         # cholinv.h unpack: sub-ranges of a packed upper triangle into rects of exactly the range's size
    psz = ref.packed_len(U, n)
    out["sub_offdiag"] = dict(shape=RECT, ss=U, ds=RECT, sdimX=n, sdimY=n, ddimX=n - h1, ddimY=h1, src_len=psz, dst_len=(n - h1) * h1,
                              ranges=(h1, n, 0, h1, 0, n - h1, 0, h1), oracle=False)     # a rect copy out of a triangle: no specialisation of the reference
    out["sub_lowright"] = dict(shape=U, ss=U, ds=RECT, sdimX=n, sdimY=n, ddimX=n - h1, ddimY=n - h1, src_len=psz, dst_len=(n - h1) ** 2,
                               ranges=(h1, n, h1, n, 0, n - h1, 0, n - h1), oracle=True)
    out["sub_upleft"] = dict(shape=U, ss=U, ds=RECT, sdimX=n, sdimY=n, ddimX=h1, ddimY=h1, src_len=psz, dst_len=h1 * h1,
                             ranges=(0, h1, 0, h1, 0, h1, 0, h1), oracle=True)
    out["wide_rect"] = dict(shape=RECT, ss=RECT, ds=RECT, sdimX=65539, sdimY=5, ddimX=65539, ddimY=4, src_len=65539 * 5, dst_len=65539 * 4,
                            ranges=(0, 65539, 1, 4, 0, 65539, 0, 3), oracle=True)       # 65539 columns of 3 rows: the column stride loop
    return out


SERIALIZE_SHAPE_CASES = _shape_cases()


def serialize_reference(c, src, dst):
    return ref.serialize_shape(c["shape"], c["ss"], c["ds"], src, c["sdimY"], dst, c["ddimY"], *c["ranges"])


# ---- the other tables -----------------------------------------------------------------------------------------------------------------------
LACPY_CASES = [(1, 1, 1, 1), (257, 263, 260, 259), (600, 17, 603, 600), (17, 600, 17, 20)]                  # m, n, lda, ldb
LACPY_WIDE = (1, 524288)                                                                                       # m, n: more than 65535 groups of 8 columns
TRIZERO_ORDERS = (1, 256, 257, 600)                                                                            # lda = n + 3
REMOVE_TRIANGLE_SHAPES = [(37, 300), (300, 37), (65538, 3)]                                                    # dimX (columns), dimY (rows)
BLOCK_CYCLIC_CASES = [(8, 5, 2), (5, 8, 3), (130, 3, 2), (129, 129, 2), (1, 32770, 2)]                         # rl, cl, d
BLOCK_CYCLIC_TRI_CASES = [(129, 2), (100, 3)]                                                                  # rl, d
CYCLIC_TO_LOCAL_CASES = [(257, 2, 514), (130, 3, 390), (130, 2, 263), (8, 2, 19)]                              # L, d, bc
DIFF_NORMS_SHAPES = [(1, 1), (255, 3), (256, 3), (257, 5), (300, 200), (700, 40), (40, 700)]                   # m, n; ldx = m + 3, ldy = m + 7
AXPBY_COUNTS = (1, 3000001)
AXPBY_BETAS = (-0.25, 0.0, 1.0)


def remove_triangle_grids(dimX):
    """(direction, P, px, py): every piece of the 1 x 1, 2 x 2 and 3 x 3 grids both ways; at the wide shape one piece per direction"""
    if dimX > 65535:
        return [("U", 3, 2, 1), ("L", 2, 0, 1)]
    return [(dr, P, px, py) for dr in "UL" for P in (1, 2, 3) for px in range(P) for py in range(P)]


def slice_ranks(L, d):
    return list(range(d * d)) if L <= 8 else [0, 1, d * d - 1]


def diff_norms_positions(m, n):
    """(i, j) of the planted difference: the corners, the rows on both sides of the kernel's thread stride, a diagonal element and its two
    neighbours in the column; each once, those outside the block dropped"""
    k = min(m, n) // 2
    cand = [(0, 0), (m - 1, 0), (0, n - 1), (m - 1, n - 1), (255, n // 2), (256, n // 2), (k, k), (k - 1, k), (k + 1, k)]
    return sorted({(i, j) for i, j in cand if 0 <= i < m and 0 <= j < n})


def in_part(part, i, j):
    return part == 0 or (i <= j if part == 1 else i >= j)
