"""The case table, the operand builders, the reference and the checker of tests/test_gpu_tile_kernels.py (and of its child process,
tests/_gpu_tile_main.py, and of the CPU test tests/test_tile_cases.py).  numpy only: no torch, no GPU.

A row is a plain dict (it travels to the child as JSON):
  tag            unique name; the operands are seeded by it
  fn             "gemm" | "syrk" | "gemmt" | "trmm_oop" (capi_dgemm, capi_dsyrk, capi_dgemmt, capi_dtrmm_oop)
  flags          gemm: ta, tb;  syrk: uplo, trans;  gemmt: uplo, ta (tb = 1 - ta);  trmm_oop: side, uplo, trans, diag
  m, n, k        logical extents (syrk / gemmt: m == n; trmm_oop: k is the order of T)
  alpha, beta
  padA, padB, padC   rows added to each leading dimension (padC is always 3)
  offA, offB     0 or 1 element of pointer offset into a larger allocation
  data           "exact" | "real"
  env            "ts64" | "ts128" | "free": the environment of the child that runs it (ENVS)
  ts             the tile size the row must run on (the forced one; for "free" rows the one a 256-CU device chooses)
  marks          plan properties the row is named for: "splitk", "share", "bands", "unvec_a", "unvec_b", "scale"

The table asks for 16-byte loads by parity: a row that wants them on an operand gets an even leading dimension (pad 2 on an even
row count, 1 on an odd one -- never 0, so there are always NaN rows between the extent and ld), a row that does not gets an odd one
(pad 1 / 2) or a pointer offset of one element.  The pads therefore differ between the four orientations of one shape.

exact data: entries are integers in [-4, 4], alpha and beta come from {0, +-0.5, +-1, 2}: every product and every partial sum is an
exact double (|sum| <= 16 K < 2^53), so float64 numpy gives THE result in any summation order and the check is np.array_equal.
real data: entries uniform in (-1, 1), reference in np.longdouble, componentwise bound
  |got - ref| <= 2 (K + splitk + 4) u (|alpha| |op A| |op B| + |beta| |C|),  u = 2^-53
-- the inner-product bound for any order of summation (K u), one rounding per split-K partial sum in the reduce (splitk u), alpha,
beta and the final sum (4 u), times 2 for the second-order terms; derived, not measured."""
import zlib

import numpy as np

U = 2.0 ** -53
LEFT, RIGHT, UPPER, LOWER = 0, 1, 1, 0
ENVS = {"ts64": {"CAPI_SMALL": "0", "CAPI_FORCE_TS": "64"}, "ts128": {"CAPI_SMALL": "0", "CAPI_FORCE_TS": "128"}, "free": {}}
FORCED = {"ts64": dict(force_small=0, force_ts=64), "ts128": dict(force_small=0, force_ts=128), "free": {}}
ORIENT = (("nn", 0, 0), ("nt", 0, 1), ("tn", 1, 0), ("tt", 1, 1))
EXACT_ALPHAS = (1.0, -1.0, 0.5, 2.0, -0.5)
REAL_LIMIT = 4e7          # m n k up to which a row may carry real data (the long-double product stays cheap) ...
# ... but for the one real split-K row of the 128-tile: its smallest split-K shape is 256 x 256 x 8192 (a few seconds of long double)


# ---- shapes as stored -----------------------------------------------------------------------------------------------------------------
def stored_shapes(row):
    """(rows, cols) of A and of B as they lie in memory (B: None for syrk) and of the logical C."""
    f, m, n, k = row["flags"], row["m"], row["n"], row["k"]
    if row["fn"] == "gemm":
        return ((k, m) if f["ta"] else (m, k)), ((n, k) if f["tb"] else (k, n)), (m, n)
    if row["fn"] == "syrk":
        return ((k, n) if f["trans"] else (n, k)), None, (n, n)
    if row["fn"] == "gemmt":
        s = (k, n) if f["ta"] else (n, k)
        return s, s, (n, n)
    nt = m if f["side"] == LEFT else n
    return (nt, nt), (m, n), (m, n)                          # T, B


def lds(row):
    sa, sb, sc = stored_shapes(row)
    return sa[0] + row["padA"], (sb[0] + row["padB"] if sb else sa[0] + row["padA"]), sc[0] + row["padC"]


def _pad_for(rows, vec):
    """None: tight (pad 0).  True: an even ld, False: an odd one -- with at least one padding row either way."""
    if vec is None:
        return 0
    even_pad = 2 if rows % 2 == 0 else 1
    return even_pad if vec else 3 - even_pad


def make_row(env, ts, tag, fn, flags, m, n, k, alpha, beta, data="exact", vec=(True, True), offA=0, offB=0, marks=()):
    row = dict(tag=tag, fn=fn, flags=dict(flags), m=m, n=n, k=k, alpha=alpha, beta=beta, padA=0, padB=0, padC=3, offA=offA, offB=offB,
               data=data, env=env, ts=ts, marks=list(marks))
    sa, sb, _ = stored_shapes(row)
    row["padA"] = _pad_for(sa[0], vec[0])
    row["padB"] = _pad_for(sb[0], vec[1]) if sb else row["padA"]
    if data == "exact":
        assert alpha in (0.0, 0.5, -0.5, 1.0, -1.0, 2.0) and beta in (0.0, 0.5, -0.5, 1.0, -1.0, 2.0), tag
    return row


# ---- what the planner is told about a row (gemm_f64.hip: capi_dgemm, capi_dgemmt, capi_dsyrk, trmm_launch, launch_gemm) ----------------
def product_of(row):
    """The gemm_plan::Product of the row's call, with the overrides of its environment: the input of tests/gemm_plan/gemm_plan_sim."""
    f, fn = row["flags"], row["fn"]
    lda, ldb, _ = lds(row)
    va, vb = row["offA"] == 0 and lda % 2 == 0, row["offB"] == 0 and ldb % 2 == 0
    p = dict(M=row["m"], N=row["n"], K=row["k"], alpha_zero=int(row["alpha"] == 0.0), beta=row["beta"])
    if fn == "gemm":
        p.update(ak=f["ta"], bkc=1 - f["tb"], a_vec=int(va), b_vec=int(vb), same_ld=int(lda == ldb))
    elif fn == "syrk":
        p.update(out_uplo=f["uplo"], ak=f["trans"], bkc=f["trans"], a_is_b=1, same_ld=1, a_vec=int(va), b_vec=int(va))
    elif fn == "gemmt":
        p.update(out_uplo=f["uplo"], ak=f["ta"], bkc=f["ta"], a_vec=int(va), b_vec=int(vb), same_ld=int(lda == ldb))
    else:                                                    # A is T, B is the dense operand; launch_gemm's A-operand is T only on the left
        eff_upper = int((f["uplo"] == UPPER) != (f["trans"] == 1))
        p.update(tri_side=f["side"], tri_eff_upper=eff_upper)
        if f["side"] == LEFT:
            p.update(ak=f["trans"], bkc=1, a_vec=int(va), b_vec=int(vb), same_ld=int(lda == ldb))
        else:
            p.update(ak=0, bkc=1 - f["trans"], a_vec=int(vb), b_vec=int(va), same_ld=int(lda == ldb))
    p.update(FORCED[row["env"]])
    return p


def plan_errors(row, p):
    """What is wrong with plan line `p` (product and plan fields, as strings) for this row; an empty list when it is the intended one."""
    bad = []
    seen = ("M", "N", "K", "ak", "bkc", "a_vec", "b_vec", "alpha_zero", "out_uplo", "tri_side", "tri_eff_upper", "a_is_b")
    want = {k: str(v) for k, v in product_of(row).items() if k in seen}
    for k, v in want.items():
        if p.get(k) != v:
            bad.append(f"{k}={p.get(k)} (the table says {v})")
    marks = row["marks"]
    if "scale" in marks:
        if p["path"] != "scale":
            bad.append(f"path={p['path']}, not scale")
        return bad
    if p["path"] != "tile" or int(p["ts"]) != row["ts"]:
        bad.append(f"path={p['path']} ts={p['ts']}, not tile / {row['ts']}")
    if "splitk" in marks:
        if not (int(p["splitk"]) > 1 and p["k_rotate"] == "1" and p["reduce"] == "narrow"):
            bad.append(f"splitk={p['splitk']} k_rotate={p['k_rotate']} reduce={p['reduce']}")
    elif int(p["splitk"]) != 1:
        bad.append(f"splitk={p['splitk']} on a row that is not named for it")
    if ("share" in marks) != (p["share_ab"] == "1"):
        bad.append(f"share_ab={p['share_ab']}")
    if ("bands" in marks) != (p["order"] == "1"):
        bad.append(f"order={p['order']}")
    if "unvec_a" in marks and (p["a_vec"], p["b_vec"]) != ("0", "1"):
        bad.append(f"a_vec={p['a_vec']} b_vec={p['b_vec']}")
    if "unvec_b" in marks and (p["a_vec"], p["b_vec"]) != ("1", "0"):
        bad.append(f"a_vec={p['a_vec']} b_vec={p['b_vec']}")
    return bad


def all_interior(row):
    """Every tile of the launch is whole and both operands take 16-byte loads: the kernel's `interior`."""
    p = product_of(row)
    return row["m"] % row["ts"] == 0 and row["n"] % row["ts"] == 0 and p["a_vec"] == 1 and p["b_vec"] == 1


def ragged(row):
    return row["m"] % row["ts"] != 0 and row["n"] % row["ts"] != 0 and row["k"] % 16 != 0


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
def _plain(env, ts):
    V, T = (True, True), (None, None)
    shapes = [((1, 1, 1), T, 0, ()), ((64, 64, 16), T, 0, ()), ((128, 128, 16), T, 0, ()),
              ((65, 63, 17), (False, True), 0, ("unvec_a",)), ((65, 63, 17), (True, False), 0, ("unvec_b",)),
              ((130, 67, 37), (False, True), 0, ("unvec_a",)), ((130, 67, 37), (True, False), 0, ("unvec_b",)),
              ((256, 256, 15), V, 0, ()), ((256, 256, 80), V, 0, ()), ((256, 256, 83), V, 0, ()),
              ((256, 256, 83), V, 1, ("unvec_b",)), ((256, 256, 83), (False, True), 0, ("unvec_a",)),
              ((384, 129, 200), V, 0, ()), ((129, 384, 200), V, 0, ())]
    rows = []
    for s, ((m, n, k), vec, offB, marks) in enumerate(shapes):
        for o, (oname, ta, tb) in enumerate(ORIENT):
            what = "_".join(marks) + ("_off" if offB else "")
            rows.append(make_row(env, ts, f"{env}_gemm_{oname}_{m}x{n}x{k}" + (f"_{what}" if what else ""), "gemm", dict(ta=ta, tb=tb), m, n, k,
                                 EXACT_ALPHAS[(s + 2 * o) % 5], (0.0, 1.0, -0.5)[(s + o) % 3], vec=vec, offB=offB, marks=marks))
    for s, (m, n, k) in enumerate([(130, 67, 37), (256, 256, 83), (384, 129, 200)]):
        for o, (oname, ta, tb) in enumerate(ORIENT):
            rows.append(make_row(env, ts, f"{env}_gemm_{oname}_{m}x{n}x{k}_real", "gemm", dict(ta=ta, tb=tb), m, n, k,
                                 1.7, (0.0, -0.6, 1.0)[(s + o) % 3], data="real"))
    # alpha == 0: neither A nor B is read (they hold NaN only), C is scaled
    rows.append(make_row(env, ts, f"{env}_gemm_nn_130x67x37_alpha0_scale", "gemm", dict(ta=0, tb=0), 130, 67, 37, 0.0, -0.5, marks=("scale",)))
    return rows


def _splitk(env, shapes, ts_of, real):
    rows = []
    for s, (m, n, k) in enumerate(shapes):
        for o, (oname, ta, tb) in enumerate(ORIENT):
            rows.append(make_row(env, ts_of[(m, n, k)], f"{env}_gemm_{oname}_{m}x{n}x{k}_splitk", "gemm", dict(ta=ta, tb=tb), m, n, k,
                                 EXACT_ALPHAS[(s + o) % 5], (0.0, -0.5)[(s + o) % 2], marks=("splitk",)))
    if real:
        (m, n, k), (oname, ta, tb) = real, ORIENT[2]
        rows.append(make_row(env, ts_of[real], f"{env}_gemm_{oname}_{m}x{n}x{k}_splitk_real", "gemm", dict(ta=ta, tb=tb), m, n, k, -1.3, 0.7,
                             data="real", marks=("splitk",)))
    return rows


def _tri_forms():
    for uplo in (UPPER, LOWER):
        for t in (1, 0):
            yield "syrk", dict(uplo=uplo, trans=t), f"syrk_{'ul'[uplo == LOWER]}{'nt'[t]}", ("share",)
            yield "gemmt", dict(uplo=uplo, ta=t), f"gemmt_{'ul'[uplo == LOWER]}{'nt'[t]}", ()


def _tri(env, ts):
    shapes = [((130, 37), ()), ((256, 83), ()), ((200, 16), ())]
    if ts == 128:
        shapes += [((256, 8197), ("splitk",)), ((2100, 40), ("bands",))]        # 3 tiles, split along k; 17 tile rows
    else:
        shapes += [((1000, 40), ("bands",))]                                    # 16 tile rows, the last band ragged
    rows = []
    for s, ((n, k), marks) in enumerate(shapes):
        for o, (fn, flags, name, fmarks) in enumerate(_tri_forms()):
            beta = (0.0, -0.5)[(s + o) % 2] if "splitk" in marks else (0.0, 1.0, -0.5)[(s + o) % 3]
            rows.append(make_row(env, ts, f"{env}_{name}_{n}x{k}" + "".join("_" + x for x in marks), fn, flags, n, n, k,
                                 EXACT_ALPHAS[(s + o) % 5], beta, marks=marks + fmarks))
    # A with an odd leading dimension: the shared panel of a diagonal tile through the 8-byte loads
    rows.append(make_row(env, ts, f"{env}_syrk_ut_130x37_oddld", "syrk", dict(uplo=UPPER, trans=1), 130, 130, 37, -1.0, -0.5,
                         vec=(False, False), marks=("share",)))
    return rows


def _trmm(env, ts):
    rows = []
    for s, (m, n) in enumerate([(200, 136), (136, 200)]):
        for o in range(16):
            side, uplo, trans, diag = o >> 3 & 1, o >> 2 & 1, o >> 1 & 1, o & 1
            rows.append(make_row(env, ts, f"{env}_trmm_{'LR'[side]}{'LU'[uplo]}{'NT'[trans]}{'NU'[diag]}_{m}x{n}", "trmm_oop",
                                 dict(side=side, uplo=uplo, trans=trans, diag=diag), m, n, m if side == LEFT else n,
                                 EXACT_ALPHAS[(s + o) % 5], 0.0))
    return rows


SPLITK_SHAPES = {"ts128": [(256, 256, 8192), (256, 256, 8197)], "ts64": [(129, 65, 4101), (129, 65, 600), (192, 192, 2053)],
                 "free": [(640, 640, 4101), (520, 130, 9000), (700, 300, 5000)]}
# the tile size a 256-CU device chooses for the unforced rows (tests/test_tile_cases.py holds the planner to it)
FREE_TS = {(640, 640, 4101): 64, (520, 130, 9000): 64, (700, 300, 5000): 64}


def _build():
    rows = []
    for env, ts in (("ts64", 64), ("ts128", 128)):
        fixed = {s: ts for s in SPLITK_SHAPES[env]}
        rows += _plain(env, ts) + _splitk(env, SPLITK_SHAPES[env], fixed, SPLITK_SHAPES[env][0] if ts == 128 else (129, 65, 600))
        rows += _tri(env, ts) + _trmm(env, ts)
    rows += _splitk("free", SPLITK_SHAPES["free"], FREE_TS, None)
    tags = [r["tag"] for r in rows]
    assert len(set(tags)) == len(tags)
    for r in rows:
        assert r["data"] == "exact" or float(r["m"]) * r["n"] * r["k"] <= REAL_LIMIT or r["tag"] == "ts128_gemm_tn_256x256x8192_splitk_real", r["tag"]
    return rows


ROWS = _build()


def rows_of(env):
    return [r for r in ROWS if r["env"] == env]


# ---- operands -----------------------------------------------------------------------------------------------------------------------------
def _place(mat, pad, off):
    """`mat` column-major in a flat buffer, `off` elements in, leading dimension rows + pad; NaN wherever `mat` is not."""
    rows, cols = mat.shape
    ld = rows + pad
    flat = np.full(off + ld * cols, np.nan)
    flat[off:].reshape(cols, ld).T[:rows] = mat
    return flat


def view(flat, ld, cols, off=0):
    """The (ld, cols) column-major matrix that starts `off` elements into `flat` (a view)."""
    return flat[off:off + ld * cols].reshape(cols, ld).T


def _draw(rng, shape, data):
    return rng.integers(-4, 5, size=shape).astype(np.float64) if data == "exact" else rng.uniform(-1.0, 1.0, size=shape)


def operands(row):
    """{"A", "B", "C"}: flat float64 buffers as the call sees them (the pointers are offA / offB elements in; B is None for syrk),
    and {"lda", "ldb", "ldc"}.  trmm_oop: A is T, with NaN in its other strict triangle and on a unit diagonal."""
    rng = np.random.default_rng(zlib.crc32(row["tag"].encode()))
    sa, sb, (m, n) = stored_shapes(row)
    f = row["flags"]
    A = _draw(rng, sa, row["data"])
    B = _draw(rng, sb, row["data"]) if sb else None
    if row["fn"] == "trmm_oop":
        i, j = np.indices(sa)
        dead = (i > j) if f["uplo"] == UPPER else (i < j)
        if f["diag"]:
            dead |= i == j
        A[dead] = np.nan
    if row["alpha"] == 0.0:
        A[:] = np.nan
        if B is not None:
            B[:] = np.nan
    lda, ldb, ldc = lds(row)
    Cm = _draw(rng, (ldc, n), row["data"])
    if row["beta"] == 0.0:
        Cm[:m] = np.nan
    return dict(A=_place(A, row["padA"], row["offA"]), B=None if B is None else _place(B, row["padB"], row["offB"]),
                C=np.ascontiguousarray(Cm.T).reshape(-1), lda=lda, ldb=ldb, ldc=ldc)


def logical(row, ops):
    """op(A) (m x k), op(B) (k x n) with the triangle of a trmm masked out explicitly, the input C (m x n), the wanted part (bool m x n)."""
    sa, sb, (m, n) = stored_shapes(row)
    f, fn = row["flags"], row["fn"]
    A = view(ops["A"], ops["lda"], sa[1], row["offA"])[:sa[0]]
    B = A if sb is None else view(ops["B"], ops["ldb"], sb[1], row["offB"])[:sb[0]]
    wanted = np.ones((m, n), dtype=bool)
    if fn == "gemm":
        opA, opB = (A.T if f["ta"] else A), (B.T if f["tb"] else B)
    elif fn in ("syrk", "gemmt"):
        t = f["trans"] if fn == "syrk" else f["ta"]
        opA, opB = (A.T, B) if t else (A, B.T)
        i, j = np.indices((m, n))
        wanted = (i <= j) if f["uplo"] == UPPER else (i >= j)
    else:
        T = np.where(np.isnan(A), 0.0, A)
        T = np.triu(T) if f["uplo"] == UPPER else np.tril(T)
        if f["diag"]:
            np.fill_diagonal(T, 1.0)
        opT = T.T if f["trans"] else T
        opA, opB = (opT, B) if f["side"] == LEFT else (B, opT)
    C0 = view(ops["C"], ops["ldc"], n)[:m]
    return opA, opB, C0, wanted


def reference(row, ops):
    """(ref, scale, wanted): alpha op(A) op(B) + beta C on the m x n block -- float64 (exact data: THE result) or np.longdouble (real
    data) -- and |alpha| |op A| |op B| + |beta| |C|, the matrix the real rows' bound is relative to (None for exact data)."""
    opA, opB, C0, wanted = logical(row, ops)
    alpha, beta = row["alpha"], row["beta"]
    ft = np.float64 if row["data"] == "exact" else np.longdouble
    ref = np.zeros(C0.shape, dtype=ft)
    if alpha != 0.0:
        ref += ft(alpha) * (opA.astype(ft) @ opB.astype(ft))
    if beta != 0.0:
        ref += ft(beta) * C0.astype(ft)
    scale = None
    if row["data"] == "real":
        scale = abs(alpha) * (np.abs(opA) @ np.abs(opB)) + (abs(beta) * np.abs(C0) if beta != 0.0 else 0.0)
    return ref, scale, wanted


def expected_output(row, ops, ref=None):
    """The flat C a correct call leaves behind: the reference (rounded to float64) in the wanted part, the input everywhere else."""
    ref, _, wanted = reference(row, ops) if ref is None else ref
    out = ops["C"].copy()
    blk = view(out, ops["ldc"], row["n"])[:row["m"]]
    blk[wanted] = ref[wanted].astype(np.float64)
    return out


def check(row, got, splitk, ops=None, ref=None):
    """AssertionError unless `got` (the flat C after the call) is right; returns the worst error / bound of the wanted part (0 for exact
    data).  `ops` and `ref`: operands(row) and reference(row, ops) when the caller has them already."""
    tag = row["tag"]
    ops = operands(row) if ops is None else ops
    ref, scale, wanted = reference(row, ops) if ref is None else ref
    m, n, ldc = row["m"], row["n"], ops["ldc"]
    got = np.ascontiguousarray(got, dtype=np.float64).reshape(-1)
    assert got.shape == ops["C"].shape, f"{tag}: C has {got.size} elements, expected {ops['C'].size}"
    live = np.zeros(got.size, dtype=bool)
    view(live, ldc, n)[:m] = wanted
    # everything outside the wanted part is the input, bit for bit: the other strict triangle, the rows m..ldc
    same = got.view(np.int64) == ops["C"].view(np.int64)
    if not same[~live].all():
        at = int(np.flatnonzero(~same & ~live)[0])
        raise AssertionError(f"{tag}: {int((~same & ~live).sum())} elements outside the wanted part were written, the first at "
                             f"(i, j) = ({at % ldc}, {at // ldc}) of the {m} x {n} block with ldc {ldc}: {ops['C'][at]!r} -> {got[at]!r}")
    g = view(got, ldc, n)[:m]
    assert not np.isnan(g[wanted]).any(), f"{tag}: {int(np.isnan(g[wanted]).sum())} NaN in the wanted part"
    if row["data"] == "exact":
        ne = (g != ref) & wanted
        if ne.any():
            i, j = (int(x[0]) for x in np.nonzero(ne))
            raise AssertionError(f"{tag}: {int(ne.sum())} of {int(wanted.sum())} elements differ from the exact result, the first at "
                                 f"({i}, {j}): got {g[i, j]!r}, exact {ref[i, j]!r}")
        return 0.0
    bound = 2.0 * (row["k"] + splitk + 4) * U * scale
    err = np.abs(g.astype(np.longdouble) - ref).astype(np.float64)
    over = (err > bound) & wanted
    if over.any():
        i, j = (int(x[0]) for x in np.nonzero(over))
        raise AssertionError(f"{tag}: {int(over.sum())} elements beyond the bound, the first at ({i}, {j}): err {err[i, j]:.3e} > "
                             f"{bound[i, j]:.3e}")
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(wanted & (bound > 0), err / bound, 0.0)
    return float(ratio.max())
