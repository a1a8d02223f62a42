"""The case table, operands, reference and check of the SUMMA grid tests (tests/test_summa_gloo.py on the CPU shim, tests/test_gpu_summa.py on the
device): matmult::summa's gemm, trmm and syrk in every form, one multiply per case through capital_summa_gemm / _trmm / _syrk.

The contract ("SUMMA on a grid"): rank (x, y, z) of a d x d x c grid holds rows y::d and columns x::d of a global operand G -- local
(row i, column j) is global (y + i d, x + j d) --, depth replicas hold the same block.  A transposed operand is passed as the LOCAL transpose of the
rank's block of op(G).  Of a triangular T only the `uplo` triangle of each local block is read, diagonal included: entries of the global other
triangle that land on a local diagonal are stored zeros, what lies strictly inside the local other triangle is NaN here, and so is the global
diagonal of a unit-diagonal T.  syrk writes the `uplo` triangle of each local block and leaves the rest alone.

Everything here is numpy on the host; the operands of a form are seeded by its name, so the ranks (which cut their blocks) and the parent (which
checks them) build the same global matrices without shipping them."""
import functools
import os
import zlib

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
SENTINEL = 3.0517578125e+77                # in the local triangle of a syrk output that the call must not touch
PAD = 2                                    # pad rows of the view mode: ld = rows + 2 stays odd
CHUNKS = 3                                 # 101 columns -> 34, 34, 33
MIN_CHUNK_COLS = "2"                       # read once per process: set for the whole launch
# local extents (odd: 16-byte alignment of a chunk, a K slice or a landing block is earned, not given)
GEMM_MNK = (67, 101, 83)
TRMM_LEFT = (83, 101)                      # order of T, columns of B
TRMM_RIGHT = (67, 101)                     # rows of B, order of T
SYRK_NK = (101, 67)
NARROW = 10                                # with num_chunks = 4 and MIN_CHUNK_COLS = 2: chunks of 4, 4, 2 and an empty fourth
NARROW_CHUNKS = 4

ENVS = [
    ("dflt", {}),
    ("kslice", {"CAPITAL_KSLICE": "1"}),
    ("nopack", {"CAPITAL_NO_PACKED_COMM": "1"}),
    ("mp0", {"CAPITAL_MULTIPATH": "0"}),
    ("mp2", {"CAPITAL_MULTIPATH": "2", "CAPITAL_MULTIPATH_MIN": "8"}),
]
ENV_KEYS = ("CAPITAL_KSLICE", "CAPITAL_NO_PACKED_COMM", "CAPITAL_MULTIPATH", "CAPITAL_MULTIPATH_MIN")      # what a rank clears between two cases
GRID_C = {1: 1, 2: 2, 4: 1, 8: 2}          # world -> c of the d x d x c grid: 1x1x1, 1x1x2, 2x2x1, 2x2x2


def _forms(narrow=False):
    """name -> form.  narrow: the forms whose output columns the chunk pipeline cuts, at NARROW columns."""
    f = {}
    M, N, K = GEMM_MNK
    if narrow:
        N = NARROW
    for ta in (0, 1):
        for tb in (0, 1):
            if not narrow or tb == 0:
                f[f"gemm_{'NT'[ta]}{'NT'[tb]}"] = dict(op="gemm", ta=ta, tb=tb, alpha=0.75, beta=-0.5, nan=False, dims=(M, N, K))
    for ta in (0, 1):
        f[f"gemm_{'NT'[ta]}N_b0"] = dict(op="gemm", ta=ta, tb=0, alpha=0.75, beta=0.0, nan=True, dims=(M, N, K))
    units = {("L", "U", 0), ("L", "L", 1), ("R", "U", 0), ("R", "L", 0)}
    for side in "LR":
        for uplo in "UL":
            for tr in (0, 1):
                nt, n = TRMM_LEFT if side == "L" else TRMM_RIGHT[::-1]
                if narrow:
                    if (side, uplo, tr) not in (("L", "U", 0), ("L", "L", 1), ("R", "U", 0)):
                        continue
                    nt, n = (nt, NARROW) if side == "L" else (NARROW, n)
                dims = (nt, n) if side == "L" else (n, nt)                      # (M, N) of B
                for unit in ((0, 1) if (side, uplo, tr) in units else (0,)):
                    f[f"trmm_{side}{uplo}{'NT'[tr]}{'NU'[unit]}"] = dict(op="trmm", side=side, uplo=uplo, tr=tr, unit=unit, alpha=-1.5, dims=dims)
    N, K = SYRK_NK
    if narrow:
        N = NARROW
    for uplo in "UL":
        for tr in (0, 1):
            if not narrow or (uplo, tr) == ("U", 1):
                f[f"syrk_{uplo}{'NT'[tr]}"] = dict(op="syrk", uplo=uplo, tr=tr, alpha=-1.0, beta=1.0, nan=False, dims=(N, K))
    for uplo, tr in (("U", 1),) if narrow else (("U", 1), ("L", 0)):
        f[f"syrk_{uplo}{'NT'[tr]}_b0"] = dict(op="syrk", uplo=uplo, tr=tr, alpha=0.75, beta=0.0, nan=True, dims=(N, K))
    return {(name + "_narrow" if narrow else name): dict(v, name=(name + "_narrow" if narrow else name)) for name, v in f.items()}


FORMS = dict(_forms(), **_forms(narrow=True))


def cases(only=None):
    """Every multiply of one launch (only: of the forms whose name contains one of these strings), grouped by environment (a rank rebuilds its
    grid only where CAPITAL_MULTIPATH changes): each form with num_chunks 0 and non-zero, through the public overloads (pad 0) and the
    view-level engine, under each of ENVS; the narrow forms with the chunk count that leaves their last chunk empty."""
    out = []
    for ename, env in ENVS:
        for name, form in FORMS.items():
            narrow = name.endswith("_narrow")
            if only and not any(o in name for o in only):
                continue
            for chunks in ((NARROW_CHUNKS,) if narrow else (0, CHUNKS)):
                for pad in (0, PAD):
                    out.append(dict(tag=f"{name}-ch{chunks}-p{pad}-{ename}", form=name, chunks=chunks, pad=pad, env=env))
    return out


def coords(rank, world):
    """(x, y, z, d, c) of a world rank under layout 0 of topo::square"""
    c = GRID_C[world]
    d = int(round((world // c) ** 0.5))
    assert d * d * c == world
    return (rank % (d * c)) // c, rank // (d * c), rank % c, d, c


def _block(G, x, y, d):
    return G[y::d, x::d]


@functools.lru_cache(maxsize=None)
def operands(name, d):
    """The global operands of a form on a grid of side d, in [-1, 1]: (op(A), op(B), C0) for gemm, (op(T) with its other triangle zero -- and a
    unit diagonal where the form has one --, B, None) for trmm, (A, None, C0) for syrk."""
    f = FORMS[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    rnd = lambda r, c: rng.uniform(-1.0, 1.0, (r * d, c * d))
    if f["op"] == "gemm":
        M, N, K = f["dims"]
        return rnd(M, K), rnd(K, N), rnd(M, N)
    if f["op"] == "trmm":
        M, N = f["dims"]
        nt = M if f["side"] == "L" else N
        T = rnd(nt, nt)
        T = np.triu(T) if f["uplo"] == "U" else np.tril(T)         # the stored orientation
        if f["unit"]:
            np.fill_diagonal(T, 1.0)
        return (T.T.copy() if f["tr"] else T), rnd(M, N), None
    N, K = f["dims"]
    return (rnd(K, N) if f["tr"] else rnd(N, K)), None, rnd(N, N)


def local_inputs(name, x, y, d):
    """What rank (x, y) passes: a dict of its local blocks in the stored form (transposed, NaN where nothing may read, the sentinel where syrk
    must not write)."""
    f = FORMS[name]
    P, Q, C0 = operands(name, d)
    if f["op"] == "gemm":
        a, b = _block(P, x, y, d), _block(Q, x, y, d)
        c0 = np.full(_block(C0, x, y, d).shape, np.nan) if f["nan"] else _block(C0, x, y, d)
        return dict(A=a.T if f["ta"] else a, B=b.T if f["tb"] else b, C0=c0)
    if f["op"] == "trmm":
        t = _block(P, x, y, d)
        t = np.array(t.T if f["tr"] else t, order="F")               # the block as stored: its `uplo` triangle holds the data
        n = t.shape[0]
        i, j = np.indices((n, n))
        t[(i > j) if f["uplo"] == "U" else (i < j)] = np.nan
        if f["unit"] and x == y:
            t[i == j] = np.nan
        return dict(T=t, B=_block(Q, x, y, d), C0=np.full(f["dims"], np.nan))
    c0 = np.array(_block(C0, x, y, d), order="F")
    n = c0.shape[0]
    i, j = np.indices((n, n))
    wanted = (i <= j) if f["uplo"] == "U" else (i >= j)
    if f["nan"]:
        c0[wanted] = np.nan
    c0[~wanted] = SENTINEL
    return dict(A=_block(P, x, y, d), C0=c0)


def run_case(driver, case, rank, world):
    """One multiply on this rank; returns {tag + '.C': ..., tag + '.pad': ...} for the rank's result file."""
    x, y, z, d, c = coords(rank, world)
    f = FORMS[case["form"]]
    loc = local_inputs(case["form"], x, y, d)
    kw = dict(c=c, num_chunks=case["chunks"], pad=case["pad"])
    if f["op"] == "gemm":
        C, pad, where = driver.summa_gemm(loc["A"], loc["B"], loc["C0"], transA=f["ta"], transB=f["tb"], alpha=f["alpha"], beta=f["beta"], **kw)
    elif f["op"] == "trmm":
        C, pad, where = driver.summa_trmm(loc["T"], loc["B"], loc["C0"], side=f["side"], uplo=f["uplo"], trans=f["tr"], unit=f["unit"], alpha=f["alpha"], **kw)
    else:
        C, pad, where = driver.summa_syrk(loc["A"], loc["C0"], uplo=f["uplo"], trans=f["tr"], alpha=f["alpha"], beta=f["beta"], **kw)
    assert where == (x, y, z, d, c), f"the grid puts rank {rank} at {where}, the test at {(x, y, z, d, c)}"
    out = {case["tag"] + ".C": C}
    if pad is not None:
        out[case["tag"] + ".pad"] = pad
    return out


@functools.lru_cache(maxsize=None)
def reference(name, d):
    """(ref, S, Kg) of the global product in longdouble: ref = alpha op(A) op(B) + beta C0, S = |alpha| |op(A)| |op(B)| + |beta| |C0|"""
    f = FORMS[name]
    P, Q, C0 = operands(name, d)
    if f["op"] == "gemm":
        L, R = P, Q
    elif f["op"] == "trmm":
        L, R = (P, Q) if f["side"] == "L" else (Q, P)
    else:
        L, R = (P.T, P) if f["tr"] else (P, P.T)
    L, R = L.astype(LD), R.astype(LD)
    alpha, beta = LD(f["alpha"]), LD(f.get("beta", 0.0))
    ref, S = alpha * (L @ R), abs(alpha) * (np.abs(L) @ np.abs(R))
    if C0 is not None and not f.get("nan", False):
        ref, S = ref + beta * C0.astype(LD), S + abs(beta) * np.abs(C0).astype(LD)
    return ref, S, L.shape[1]


def check_case(case, world, results, fill):
    """results[rank] = that rank's result file (a mapping).  Returns (failures, worst): the list of what is wrong with this case on any rank, and the
    largest error in units of the bound."""
    f = FORMS[case["form"]]
    tag = case["tag"]
    bad, worst, replicas = [], 0.0, {}
    for rank in range(world):
        x, y, z, d, c = coords(rank, world)
        ref, S, Kg = reference(case["form"], d)
        ref, S = _block(ref, x, y, d), _block(S, x, y, d)
        got = results[rank][tag + ".C"]
        if got.shape != ref.shape:
            bad.append(f"{tag} rank {rank}: result {got.shape}, expected {ref.shape}")
            continue
        n0, n1 = got.shape
        i, j = np.indices((n0, n1))
        wanted = np.ones((n0, n1), bool) if f["op"] != "syrk" else ((i <= j) if f["uplo"] == "U" else (i >= j))
        if np.isnan(got).any():
            bad.append(f"{tag} rank {rank} ({x},{y},{z}): {int(np.isnan(got).sum())} NaN in the result, first at {tuple(np.argwhere(np.isnan(got))[0])}")
        err = np.abs(np.where(wanted, got, 0.0).astype(LD) - np.where(wanted, ref, LD(0)))
        bound = 2 * (Kg + 4) * LD(U) * np.where(wanted, S, LD(0))
        over = ~(err <= bound)                                           # (a NaN is over the bound too)
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0))) if not np.isnan(err.astype(float)).any() else float("inf")
        worst = max(worst, ratio)
        if over.any():
            k = tuple(np.argwhere(over)[0])
            bad.append(f"{tag} rank {rank} ({x},{y},{z}): {int(over.sum())} of {int(wanted.sum())} entries off the bound 2 (Kg + 4) u S, Kg = {Kg}; "
                       f"first at {k}: got {got[k]!r}, ref {float(ref[k])!r}, err / bound {float(err[k] / bound[k]) if bound[k] > 0 else float('inf'):.3g}; worst {ratio:.3g}")
        if f["op"] == "syrk" and not np.array_equal(got[~wanted].view(np.uint64), np.full(int((~wanted).sum()), SENTINEL).view(np.uint64)):
            bad.append(f"{tag} rank {rank} ({x},{y},{z}): the other triangle of the local block was written")
        if case["pad"] > 0:
            pad = results[rank][tag + ".pad"]
            if pad.shape != (case["pad"], n1) or not np.array_equal(pad.view(np.uint64), np.full(pad.shape, fill).view(np.uint64)):
                bad.append(f"{tag} rank {rank} ({x},{y},{z}): pad rows were written")
        replicas.setdefault((x, y), []).append((rank, got))
    for (x, y), blocks in replicas.items():
        for rank, other in blocks[1:]:
            if other.tobytes() != blocks[0][1].tobytes():
                bad.append(f"{tag}: depth replicas at ({x},{y}) differ in bits (ranks {blocks[0][0]} and {rank})")
    return bad, worst


def check_launch(world, directory, pattern, fill, only=None):
    """Every case of every rank of one launch: pattern.format(rank) names a rank's result file in `directory`.  Prints the largest error in units
    of the bound per operation and raises AssertionError with the list of what is wrong."""
    results = [np.load(os.path.join(directory, pattern.format(r))) for r in range(world)]
    bad, worst, todo = [], {}, cases(only)
    for case in todo:
        b, w = check_case(case, world, results, fill)
        bad += b
        op = case["form"].split("_")[0]
        worst[op] = max(worst.get(op, 0.0), w)
    print(f"[summa] world {world}: {len(todo)} multiplies, largest error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))
    forms = sorted({b.split("-")[0] for b in bad})
    assert not bad, f"{len(bad)} failures in the forms {forms}:\n" + "\n".join(bad[:40])
