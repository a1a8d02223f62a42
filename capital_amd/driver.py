"""ctypes binding of libcapital_driver.so (capital_amd/drivers/capital_driver.cpp): the host-side C++ layer
(cholesky::cholinv<...>::factor, qr::cacqr<...>::factor, validators) behind plain C entry points.

One process per GPU.  `init()` binds the C++ layer to this process's device/stream and, for world_size > 1, builds the
RCCL world communicator from a unique id that rank 0 creates and torch.distributed ships to the other ranks.
No CPU fallback: everything here ends in libcapital_hip.so kernels.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import capi

_HERE = os.path.dirname(os.path.abspath(__file__))
DRV_PATH = os.environ.get("CAPITAL_DRIVER_LIB", os.path.join(_HERE, "libcapital_driver.so"))   # override: A/B builds of the same ABI
_i64, _dbl, _int, _vp = C.c_int64, C.c_double, C.c_int, C.c_void_p
_dp = C.POINTER(C.c_double)
_drv = None
_state = {"init": False, "rank": 0, "size": 1}


class DriverError(RuntimeError):
    pass


def load():
    global _drv
    if _drv is not None:
        return _drv
    capi.load()  # libcapital_hip.so first (RTLD_GLOBAL), so the driver resolves against it
    if not os.path.exists(DRV_PATH):
        raise DriverError(f"{DRV_PATH} is missing: run __graft_entry__.build() (there is no CPU fallback)")
    D = C.CDLL(DRV_PATH, mode=C.RTLD_GLOBAL)
    _drv = bind(D)
    return D


def bind(D):
    """Declare the driver's C signatures on a loaded library object."""
    D.capital_drv_last_error.restype = C.c_char_p
    D.capital_drv_init.argtypes = [_int, _int, _int, _vp, _vp]
    D.capital_drv_handle.restype = _vp
    D.capital_cholinv_create.argtypes = [_i64] + [_int] * 8
    D.capital_cholinv_create.restype = _vp
    for f in ("generate", "factor", "destroy"):
        getattr(D, f"capital_cholinv_{f}").argtypes = [_vp]
        getattr(D, f"capital_cacqr_{f}").argtypes = [_vp]
    D.capital_cholinv_set_A.argtypes = [_vp, _dp]
    D.capital_cholinv_residual.argtypes = [_vp, _dp]
    D.capital_cholinv_get.argtypes = [_vp, _int, _dp]
    D.capital_cholinv_get_rows.argtypes = [_vp, _int, _i64, C.POINTER(_i64), _dp]
    D.capital_cholinv_dims.argtypes = [_vp, C.POINTER(_i64)] + [C.POINTER(_int)] * 5
    D.capital_cholinv_stats.argtypes = [_vp] + [C.POINTER(_i64)] * 3
    D.capital_cholinv_set_trsm_mode.argtypes = [_vp, _int]
    D.capital_cholinv_set_solve_substitution.argtypes = [_vp, _int]
    D.capital_cholinv_solve.argtypes = [_vp, _i64, _dp, _dp, _dp, _int]
    D.capital_cholinv_rcond.argtypes = [_vp, _dp, _dp]
    D.capital_cholinv_rcond_applies.argtypes = [_vp, _dp, _dp, C.POINTER(_int)]
    D.capital_cholinv_error_bounds.argtypes = [_vp, _i64, _dp, _dp, _dp]
    D.capital_cholinv_solve_expert.argtypes = [_vp, _i64, _dp, _dp, _dp, _int, _dp, _dp]
    D.capital_cholinv_update.argtypes = [_vp, _i64, _dp, _int]
    D.capital_cholinv_factor_pivoted.argtypes = [_vp, _dbl, _i64, C.POINTER(_i64), _dp, _dp]
    D.capital_cholinv_get_pivoted.argtypes = [_vp, _dp, C.POINTER(_int), _dp]
    D.capital_cholinv_apply.argtypes = [_vp, _int, _i64, _dp, _dp]
    D.capital_cholinv_quadratic_forms.argtypes = [_vp, _i64, _dp, _dp]
    D.capital_cholinv_logdet.argtypes = [_vp, _dp]
    D.capital_cholinv_inverse_diagonal.argtypes = [_vp, _dp]
    D.capital_cholinv_equilibrate.argtypes = [_vp, _dbl, C.POINTER(_int), _dp, _dp, _dp]
    D.capital_cholinv_unequilibrate.argtypes = [_vp]
    D.capital_cholinv_lowrank_prepare.argtypes = [_vp, _dbl, _dp, _int, _dp, _dp]
    D.capital_cholinv_lowrank_solve.argtypes = [_vp, _i64, _dp, _dp, _dp]
    D.capital_cholinv_lowrank_quadratic_forms.argtypes = [_vp, _i64, _dp, _dp]
    D.capital_cacqr_create.argtypes = [_i64, _i64] + [_int] * 8
    D.capital_cacqr_create.restype = _vp
    D.capital_cacqr_set_A.argtypes = [_vp, _dp]
    D.capital_cacqr_residual.argtypes = [_vp, _dp]
    D.capital_cacqr_orthogonality.argtypes = [_vp, _dp]
    D.capital_cacqr_get.argtypes = [_vp, _int, _dp]
    D.capital_cacqr_dims.argtypes = [_vp, C.POINTER(_i64), C.POINTER(_i64)]
    D.capital_cacqr_get_rows.argtypes = [_vp, _int, _i64, _i64, _dp]
    D.capital_cacqr_set_shift.argtypes = [_vp, _int, _dbl]
    D.capital_cacqr_sweep_stats.argtypes = [_vp, _int, _dp]
    D.capital_cacqr_lstsq.argtypes = [_vp, _i64, _dp, _dp, _dp]
    D.capital_cacqr_svd.argtypes = [_vp, _int, _dp, _dp, _dp, C.POINTER(_int)]
    D.capital_cacqr_factor_pivoted.argtypes = [_vp, _dbl, _dbl, C.POINTER(_int)]
    D.capital_cacqr_get_piv.argtypes = [_vp, C.POINTER(_i64)]
    _tail = [_i64, _dbl, _dp, C.POINTER(_int)]             # pad, fill, pad rows out, (x, y, z, d, c) out
    D.capital_summa_gemm.argtypes = [_int] * 5 + [_i64] * 3 + [_dbl, _dbl, _dp, _dp, _dp] + _tail
    D.capital_summa_trmm.argtypes = [_int] * 7 + [_i64] * 2 + [_dbl, _dp, _dp, _dp] + _tail
    D.capital_summa_syrk.argtypes = [_int] * 5 + [_i64] * 2 + [_dbl, _dbl, _dp, _dp] + _tail
    return D


def _ck(rc, what):
    if rc != 0:
        raise DriverError(f"{what}: {load().capital_drv_last_error().decode()}")


def init(device=0, rank=0, size=1, unique_id=None, use_torch_stream=True):
    """Bind the C++ layer to `device`.  With size > 1 `unique_id` is the 128-byte RCCL id from rank 0."""
    D = load()
    if not torch.cuda.is_available():
        raise DriverError("capital_amd needs an AMD GPU; there is no CPU fallback")
    torch.cuda.set_device(device)
    stream = _vp(torch.cuda.current_stream(device).cuda_stream) if use_torch_stream else None
    if use_torch_stream and not stream.value:
        # torch's default stream is the NULL stream; give the layer its own stream instead and sync explicitly
        stream = None
    uid = (C.c_char * 128).from_buffer_copy(unique_id) if unique_id is not None else None
    _ck(D.capital_drv_init(device, rank, size, uid, stream), "capital_drv_init")
    _state.update(init=True, rank=rank, size=size)


def init_distributed(device):
    """torch.distributed must be initialised; ships the RCCL unique id from rank 0 and builds the world communicator."""
    import torch.distributed as dist
    rank, size = dist.get_rank(), dist.get_world_size()
    uid = None
    if size > 1 or os.environ.get("CAPI_RCCL_FORCE"):      # (CAPI_RCCL_FORCE: even a 1-rank communicator goes through RCCL)
        L = capi.load()
        torch_rccl = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        named = os.environ.get("CAPI_RCCL_LIB")          # an RCCL build of the caller's choosing (same ABI), e.g. a debug build
        if named:
            if L.capi_comm_load_rccl(named.encode()) != 0:
                raise DriverError(f"CAPI_RCCL_LIB={named} cannot be loaded as an RCCL library")
        elif os.path.exists(torch_rccl):
            L.capi_comm_load_rccl(torch_rccl.encode())   # one RCCL per process: the copy torch maps
        buf = (C.c_char * 128)()
        if rank == 0:
            rc = L.capi_comm_unique_id(buf)
            if rc != 0:
                raise DriverError(f"capi_comm_unique_id -> {rc}")
        obj = [bytes(buf)]
        dist.broadcast_object_list(obj, src=0)
        uid = obj[0]
    init(device, rank, size, uid, use_torch_stream=False)


def finalize():
    if _state["init"]:
        load().capital_drv_finalize()
        _state["init"] = False


def sync():
    _ck(load().capital_drv_sync(), "sync")


def handle_ptr():
    return load().capital_drv_handle()


def world_query():
    """(rank, size) of the world communicator as RCCL reports them."""
    r, s = _int(), _int()
    _ck(load().capital_drv_world_query(C.byref(r), C.byref(s)), "world_query")
    return r.value, s.value


SUMMA_FILL = -1.2345678901234567e+100      # what the pad rows of a view-mode block hold before a summa_* call


def _summa_block(a):
    a = np.asfortranarray(a, dtype=np.float64)
    if a.ndim != 2 or a.size == 0:
        raise DriverError(f"summa: a non-empty two-dimensional local block expected, got shape {a.shape}")
    return a


def _summa_tail(pad, cols, fill):
    rows = np.zeros((pad, cols), order="F") if pad > 0 else None
    return rows, (_int * 5)(), [int(pad), float(fill), rows.ctypes.data_as(_dp) if pad > 0 else None]


def summa_gemm(A, B, C0, transA=False, transB=False, alpha=1.0, beta=0.0, c=1, layout=0, num_chunks=0, pad=0, fill=SUMMA_FILL):
    """One matmult::summa gemm on the d x d x c grid over the current world: alpha op(A) op(B) + beta C0 on this rank's LOCAL blocks (INTEGRATION.md,
    "SUMMA on a grid": which block of a global operand a rank holds).  Every rank calls.  pad=0: the public summa::invoke overload on matrix<>
    objects; pad>0: the view-level engine on device blocks of leading dimension rows + pad whose pad rows hold `fill`.  Returns (C, pad_rows,
    (x, y, z, d, c)): pad_rows are C's pad rows after the call (pad x N), None with pad=0."""
    a, b, c0 = _summa_block(A), _summa_block(B), _summa_block(C0)
    M, N = c0.shape
    K = a.shape[0] if transA else a.shape[1]
    if a.shape != ((K, M) if transA else (M, K)) or b.shape != ((N, K) if transB else (K, N)):
        raise DriverError(f"summa_gemm: blocks {a.shape}, {b.shape}, {c0.shape} do not fit transA={transA}, transB={transB}")
    out = c0.copy(order="F")
    rows, where, tail = _summa_tail(pad, N, fill)
    _ck(load().capital_summa_gemm(c, layout, num_chunks, int(bool(transA)), int(bool(transB)), M, N, K, float(alpha), float(beta),
                                  a.ctypes.data_as(_dp), b.ctypes.data_as(_dp), out.ctypes.data_as(_dp), *tail, where), "summa_gemm")
    return out, rows, tuple(where)


def summa_trmm(T, B, C0=None, side="L", uplo="U", trans=False, unit=False, alpha=1.0, c=1, layout=0, num_chunks=0, pad=0, fill=SUMMA_FILL):
    """One matmult::summa trmm: alpha op(T) B (side "L") or alpha B op(T) ("R") with this rank's block T of a triangular matrix, of which only
    the `uplo` triangle is read (and not the diagonal where unit=True and the block is a diagonal one).  C0: what the output block holds before a
    view-mode call (default zeros; the public overload multiplies in place).  Returns (C, pad_rows, (x, y, z, d, c)); pad_rows are B's."""
    t, b = _summa_block(T), _summa_block(B)
    M, N = b.shape
    nt = M if side == "L" else N
    if side not in ("L", "R") or uplo not in ("U", "L") or t.shape != (nt, nt):
        raise DriverError(f"summa_trmm: side L or R, uplo U or L and a T of order {nt} expected, got {side!r}, {uplo!r}, {t.shape}")
    out = np.zeros((M, N), order="F") if C0 is None else _summa_block(C0).copy(order="F")
    if out.shape != (M, N):
        raise DriverError(f"summa_trmm: C0 must be {M} x {N}, got {out.shape}")
    rows, where, tail = _summa_tail(pad, N, fill)
    _ck(load().capital_summa_trmm(c, layout, num_chunks, capi.LEFT if side == "L" else capi.RIGHT, capi.UPPER if uplo == "U" else capi.LOWER,
                                  int(bool(trans)), capi.UNIT if unit else capi.NONUNIT, M, N, float(alpha), t.ctypes.data_as(_dp),
                                  b.ctypes.data_as(_dp), out.ctypes.data_as(_dp), *tail, where), "summa_trmm")
    return out, rows, tuple(where)


def summa_syrk(A, C0, uplo="U", trans=True, alpha=1.0, beta=0.0, c=1, layout=0, num_chunks=0, pad=0, fill=SUMMA_FILL):
    """One matmult::summa syrk: the `uplo` triangle of this rank's block of alpha A^T A + beta C0 (trans=True, A K x N) or alpha A A^T + beta C0
    (A N x K); the rest of the block comes back as it went in.  Returns (C, pad_rows, (x, y, z, d, c)); pad_rows are C's."""
    a, c0 = _summa_block(A), _summa_block(C0)
    N = c0.shape[0]
    K = a.shape[0] if trans else a.shape[1]
    if uplo not in ("U", "L") or c0.shape != (N, N) or a.shape != ((K, N) if trans else (N, K)):
        raise DriverError(f"summa_syrk: blocks {a.shape}, {c0.shape} do not fit trans={trans}, or uplo {uplo!r} is neither U nor L")
    out = c0.copy(order="F")
    rows, where, tail = _summa_tail(pad, N, fill)
    _ck(load().capital_summa_syrk(c, layout, num_chunks, capi.UPPER if uplo == "U" else capi.LOWER, int(bool(trans)), N, K, float(alpha), float(beta),
                                  a.ctypes.data_as(_dp), out.ctypes.data_as(_dp), *tail, where), "summa_syrk")
    return out, rows, tuple(where)


class Cholinv:
    """cholesky::cholinv<SP,SaveIntermediates,BP>::factor on this process's block of an n x n SPD matrix.
    Arguments in the order of the reference bench (bench/cholesky/cholinv.cpp:15-22)."""

    def __init__(self, n, c=1, complete_inv=0, split=1, bc_mult=0, layout=0, num_chunks=0, serialize=True, bc_policy=2, trsm_mode=False,
                 flush_intermediates=False, substitution=False):
        self.D = load()
        self.p = self.D.capital_cholinv_create(n, c, layout, num_chunks, int(complete_inv), split, bc_mult,
                                               int(bool(serialize)) + (2 if flush_intermediates else 0), bc_policy)
        if not self.p:
            raise DriverError("capital_cholinv_create: " + self.D.capital_drv_last_error().decode())
        if trsm_mode:      # info::solve_with_trsm: potrf + block TRSM + SYRK, no inverse formed (not the reference's schedule)
            _ck(self.D.capital_cholinv_set_trsm_mode(self.p, 1), "set_trsm_mode")
        if substitution:   # info::solve_by_substitution: solve() by two capi_dtrsm_thin calls on R, in either mode
            self.set_solve_substitution(True)
        nloc, x, y, z, d, cc = _i64(), _int(), _int(), _int(), _int(), _int()
        _ck(self.D.capital_cholinv_dims(self.p, C.byref(nloc), C.byref(x), C.byref(y), C.byref(z), C.byref(d), C.byref(cc)), "dims")
        self.n, self.n_loc, self.x, self.y, self.z, self.d, self.c = n, nloc.value, x.value, y.value, z.value, d.value, cc.value
        self._dscale = None

    def generate(self):
        _ck(self.D.capital_cholinv_generate(self.p), "generate")
        self._dscale = None

    def set_A(self, A_local):
        a = np.asfortranarray(A_local, dtype=np.float64)
        assert a.shape == (self.n_loc, self.n_loc)
        _ck(self.D.capital_cholinv_set_A(self.p, a.ctypes.data_as(_dp)), "set_A")
        self._dscale = None

    def equilibrate(self, thresh=0.1):
        """Power-of-two equilibration of a badly scaled SPD matrix (cholesky::cholinv::equilibrate, one rank; LAPACK's dpoequb + dlaqsy): with
        d_j = 2^e_j, e_j = floor(ex_j / 2) for a_jj = f 2^ex_j, A's upper triangle becomes that of A_s = D^-1 A D^-1 (diagonal in [0.5, 2)) iff
        scond = min d / max d < thresh, or amax = max a_jj lies outside [DBL_MIN / eps, eps / DBL_MIN]; thresh > 1 forces it.  Returns
        (scaled, scond, amax).  scaled=True: factor() again -- it factors A_s -- and solve, solve_expert, update, apply, quadratic_forms, logdet and
        inverse_diagonal then answer for the ORIGINAL matrix, bit for bit as without equilibration where nothing over- or underflows; rcond() is that of
        A_s and ferr bounds the error in the scaled unknowns, ||D (x - x_true)||_inf / ||D x||_inf.  A(), R() and Rinv() show what lies on the device:
        A_s and its factors.  scaled=False: nothing changed, valid factors stay valid.  Raises DriverError when a diagonal entry is not a positive
        finite number (A is unchanged) and when A is already equilibrated."""
        scaled, scond, amax = _int(0), _dbl(0.0), _dbl(0.0)
        d = np.ones(self.n_loc)
        _ck(self.D.capital_cholinv_equilibrate(self.p, float(thresh), C.byref(scaled), C.byref(scond), C.byref(amax), d.ctypes.data_as(_dp)), "equilibrate")
        self._dscale = d if scaled.value else None
        return bool(scaled.value), scond.value, amax.value

    def scale(self):
        """the scale factors in force, n powers of two: D's diagonal while A is equilibrated, ones otherwise"""
        return np.ones(self.n_loc) if self._dscale is None else self._dscale.copy()

    def unequilibrate(self):
        """A's upper triangle <- that of D A_s D, every bit as before equilibrate() (cholesky::cholinv::unequilibrate); factor() again afterwards"""
        _ck(self.D.capital_cholinv_unequilibrate(self.p), "unequilibrate")
        self._dscale = None

    def factor(self):
        _ck(self.D.capital_cholinv_factor(self.p), "factor")

    def set_solve_substitution(self, on):
        """info::solve_by_substitution for the solves that follow; the factors stay as they are (no new factor() is needed)."""
        _ck(self.D.capital_cholinv_set_solve_substitution(self.p, int(bool(on))), "set_solve_substitution")

    def residual(self):
        v = _dbl()
        _ck(self.D.capital_cholinv_residual(self.p, C.byref(v)), "residual")
        return v.value

    def solve(self, B, refine=1, residual=True):
        """A X = B on the factors of the last factor() (cholesky::cholinv::solve, one rank): products with the resident R^-1 -- block-wise with
        R^-1_11, R^-1_22 and R_12 where complete_inv=0 skipped R^-1_12 -- or capi_dtrsm on R in TRSM mode, or, with substitution=True, two
        thin triangular solves on R (capi_dtrsm_thin: either mode, packed or not, no inverse), then `refine` steps of fixed-precision refinement.  B: n x r.  Returns (X, resnorms): X n x r; resnorms[j] = ||b_j - A x_j||_2, or None with residual=False.
        Like factor(), the refinement and the residual norms read A's upper triangle alone (capi_dresid_sym): what set_A left below the diagonal is
        never used."""
        b = np.asfortranarray(B, dtype=np.float64)
        if b.ndim == 1:
            b = np.asfortranarray(b[:, None])
        if b.ndim != 2 or b.shape[0] != self.n or b.shape[1] < 1:
            raise DriverError(f"Cholinv.solve: B must be {self.n} x r with r >= 1, got {b.shape}")
        r = b.shape[1]
        X = np.zeros((self.n, r), order="F")
        res = np.zeros(r) if residual else None
        _ck(self.D.capital_cholinv_solve(self.p, r, b.ctypes.data_as(_dp), X.ctypes.data_as(_dp), res.ctypes.data_as(_dp) if residual else None,
                                         int(refine)), "solve")
        return X, res

    def rcond(self, details=False):
        """The reciprocal condition number 1 / (||A||_1 ||A^-1||_1) of the factored A as LAPACK's dpocon estimates it (cholesky::cholinv::condition,
        one rank): ||A||_1 from one pass over A's upper triangle, ||A^-1||_1 by the Hager-Higham estimator over the operator of solve() -- at most 11
        products with A^-1 on one column.  The estimate of ||A^-1||_1 is a lower bound, so rcond errs on the large side (rarely by more than 3).
        0.0: singular to working precision (the estimate overflowed).  details=True returns (rcond, ||A||_1, products)."""
        v, a, k = _dbl(), _dbl(), _int()
        _ck(self.D.capital_cholinv_rcond_applies(self.p, C.byref(v), C.byref(a), C.byref(k)), "rcond")
        return (v.value, a.value, k.value) if details else v.value

    def solve_expert(self, B, refine=1, residual=True):
        """solve(B, refine, residual), then dporfs's bounds for its X (cholesky::cholinv::error_bounds).  Returns (X, resnorms, ferr, berr):
        berr[j] is the componentwise backward error of x_j (the smallest e with (A + dA) x_j = b_j + db_j, |dA| <= e |A|, |db_j| <= e |b_j|),
        ferr[j] an estimated bound on ||x_j - x_true,j||_inf / ||x_j||_inf.  Per block of 32 columns the bounds cost three passes over A's upper
        triangle and at most 11 products with A^-1 (an unrefined solve of the block each).  X and resnorms are solve()'s, bit for bit."""
        b = np.asfortranarray(B, dtype=np.float64)
        if b.ndim == 1:
            b = np.asfortranarray(b[:, None])
        if b.ndim != 2 or b.shape[0] != self.n or b.shape[1] < 1:
            raise DriverError(f"Cholinv.solve_expert: B must be {self.n} x r with r >= 1, got {b.shape}")
        r = b.shape[1]
        X = np.zeros((self.n, r), order="F")
        res = np.zeros(r) if residual else None
        ferr, berr = np.zeros(r), np.zeros(r)
        _ck(self.D.capital_cholinv_solve_expert(self.p, r, b.ctypes.data_as(_dp), X.ctypes.data_as(_dp), res.ctypes.data_as(_dp) if residual else None,
                                                int(refine), ferr.ctypes.data_as(_dp), berr.ctypes.data_as(_dp)), "solve_expert")
        return X, res, ferr, berr

    def update(self, V, downdate=False):
        """A <- A + V V^T (downdate=True: A - V V^T) on the factors of the last factor(), without a new factorisation (cholesky::cholinv::update, one
        rank): R, R^-1 where one exists and A's upper triangle are updated on the device in O(n^2 r).  V: n x r, any r >= 1 (blocks of 32 columns).
        Every form of solve(), rcond() and solve_expert() then works on the updated matrix.  Raises DriverError when a downdate leaves the matrix not
        positive definite: A is then unchanged, and solve() refuses until the next factor()."""
        v = np.asfortranarray(V, dtype=np.float64)
        if v.ndim == 1:
            v = np.asfortranarray(v[:, None])
        if v.ndim != 2 or v.shape[0] != self.n or v.shape[1] < 1:
            raise DriverError(f"Cholinv.update: V must be {self.n} x r with r >= 1, got {v.shape}")
        _ck(self.D.capital_cholinv_update(self.p, v.shape[1], v.ctypes.data_as(_dp), -1 if downdate else 1), "update")

    def _thin_block(self, B, who):
        b = np.asfortranarray(B, dtype=np.float64)
        if b.ndim == 1:
            b = np.asfortranarray(b[:, None])
        if b.ndim != 2 or b.shape[0] != self.n or b.shape[1] < 1:
            raise DriverError(f"Cholinv.{who}: B must be {self.n} x r with r >= 1, got {b.shape}")
        return b

    _FACTOR_OPS = {"R": 0, "RT": 1, "Rinv": 2, "RinvT": 3}

    def apply(self, B, op):
        """op B for one of the four triangular operators of A = R^T R, on the factors of the last factor() or update() (cholesky::cholinv::apply, one
        rank): op = "R", "RT" (R^T z samples N(0, A)), "Rinv" (R^-1 z samples N(0, A^-1)) or "RinvT" (R^-T b whitens b).  B: n x r, any r >= 1.
        "R" and "RT" are one thin product with R as it lies, in every mode; the inverses are one half of solve()'s operator in the form the flags
        select, so apply(apply(B, "RinvT"), "Rinv") is solve(B, refine=0)[0] bit for bit.  The X of the last solve stays as it is.  Returns n x r."""
        if op not in self._FACTOR_OPS:
            raise DriverError(f"Cholinv.apply: op must be one of {sorted(self._FACTOR_OPS)}, got {op!r}")
        b = self._thin_block(B, "apply")
        Y = np.zeros(b.shape, order="F")
        _ck(self.D.capital_cholinv_apply(self.p, self._FACTOR_OPS[op], b.shape[1], b.ctypes.data_as(_dp), Y.ctypes.data_as(_dp)), "apply")
        return Y

    def quadratic_forms(self, B):
        """q[j] = b_j^T A^-1 b_j = ||R^-T b_j||^2, the squared Mahalanobis lengths of B's columns (cholesky::cholinv::quadratic_forms, one rank): half
        a solve and a column norm; the half-solve is not kept.  B: n x r.  Returns r values."""
        b = self._thin_block(B, "quadratic_forms")
        q = np.zeros(b.shape[1])
        _ck(self.D.capital_cholinv_quadratic_forms(self.p, b.shape[1], b.ctypes.data_as(_dp), q.ctypes.data_as(_dp)), "quadratic_forms")
        return q

    def logdet(self):
        """log det A = 2 sum_i log r_ii from the resident R (cholesky::cholinv::log_determinant, one rank), in every mode"""
        v = _dbl()
        _ck(self.D.capital_cholinv_logdet(self.p, C.byref(v)), "logdet")
        return v.value

    def inverse_diagonal(self):
        """diag(A^-1): the sums of squares of the rows of the resident R^-1 (cholesky::cholinv::inverse_diagonal, one rank), one pass over the
        triangle.  With complete_inv=0 and a split top level the block R^-1_12 that factor() skipped is formed for the call (its two triangular
        products and n^2 / 4 doubles of work) and released.  Raises DriverError in TRSM mode, which has no inverse.  Returns n values."""
        d = np.zeros(self.n)
        _ck(self.D.capital_cholinv_inverse_diagonal(self.p, d.ctypes.data_as(_dp)), "inverse_diagonal")
        return d

    def factor_pivoted(self, rtol=0.0, max_rank=None):
        """A ~= L L^T with L n x rank by a diagonally pivoted, partial Cholesky (cholesky::cholinv::factor_pivoted, one rank): for a symmetric matrix
        that is only positive semidefinite or numerically low-rank -- where factor() raises -- or of which few columns are wanted; O(n rank^2).  It
        stops where the largest remaining Schur diagonal entry is <= rtol trace(A) (rtol=0: LAPACK dpstrf's default n u max a_ii) or at max_rank
        columns (None: min(n, 4096)).  Only A's upper triangle is read.  Returns (rank, resid_trace, thresh): resid_trace is the trace of A - L L^T,
        its trace-norm error for a PSD A.  Afterwards L_pivoted(), piv() and schur_diagonal().  The factors of factor() are not touched.  Raises
        DriverError at rank 0 (A is zero or not finite)."""
        rk, tr, th = _i64(0), _dbl(0.0), _dbl(0.0)
        self.pivot_rank = 0
        self._lowrank = None       # (what lowrank_prepare() left belonged to the factor before this one)
        _ck(self.D.capital_cholinv_factor_pivoted(self.p, float(rtol), 0 if max_rank is None else int(max_rank), C.byref(rk), C.byref(tr), C.byref(th)),
            "factor_pivoted")
        self.pivot_rank = rk.value
        return rk.value, tr.value, th.value

    def _get_pivoted(self, what):
        rank = getattr(self, "pivot_rank", 0)
        if rank < 1:
            raise DriverError("Cholinv: factor_pivoted() has not run or did not succeed")
        out = {"L": np.zeros((self.n, rank), order="F"), "piv": np.zeros(self.n, dtype=np.int32), "d": np.zeros(self.n)}[what]
        _ck(self.D.capital_cholinv_get_pivoted(self.p, out.ctypes.data_as(_dp) if what == "L" else None,
                                               out.ctypes.data_as(C.POINTER(_int)) if what == "piv" else None,
                                               out.ctypes.data_as(_dp) if what == "d" else None), "get_pivoted")
        return out

    def L_pivoted(self):
        """L of the last factor_pivoted(), n x rank, in A's own row ordering: column j belongs to row piv()[j], rows chosen before it are zero there"""
        return self._get_pivoted("L")

    def piv(self):
        """the rows factor_pivoted() chose, in order, then the others ascending: a permutation of 0 .. n - 1"""
        return self._get_pivoted("piv").astype(np.int64)

    def schur_diagonal(self):
        """diag(A - L L^T) as factor_pivoted() carried it: the remaining Schur diagonal of the rows not chosen, 0 for the chosen ones"""
        return self._get_pivoted("d")

    def lowrank_prepare(self, shift=0.0, diag=None, schur=False):
        """Prepare solves with M = L L^T + D on the L of the last factor_pivoted() (cholesky::cholinv::lowrank_prepare, one rank), D the positive
        diagonal d = shift + diag + (schur: schur_diagonal()): shift alone is Nystroem / subset-of-regressors regression with noise sigma^2 = shift,
        schur=True adds diag(A - L L^T) and gives FITC.  diag: None or n values.  Forms and factors the rank x rank matrix C = I + L^T D^-1 L in
        O(n rank^2); a uniform d (diag=None, schur=False) uses G = L^T L, which is kept, so that a sweep over shift on one factor pays the pass over L
        once.  Returns {"logdet": log det M, "cnorm1": ||C||_1, "rank": rank}.  The Woodbury form is not backward stable: lowrank_solve,
        lowrank_quadratic_forms and logdet carry errors of about cnorm1 * 2^-53, whatever kappa(C) is.  Neither A nor the factors of factor() are
        touched.  Raises DriverError without a successful factor_pivoted(), for a shift that is negative or not finite, a diag of another length, and
        when some d_i is not a finite number > 0 (a chosen row has Schur diagonal 0, so schur=True needs shift > 0); after a prepare that the device
        layer refused lowrank_solve refuses until one succeeds, and after a new factor_pivoted() as well."""
        self._lowrank = None
        dv = None
        if diag is not None:
            dv = np.ascontiguousarray(diag, dtype=np.float64)
            if dv.shape != (self.n,):
                raise DriverError(f"Cholinv.lowrank_prepare: diag must have {self.n} entries, got shape {dv.shape}")
        ld, cn = _dbl(0.0), _dbl(0.0)
        _ck(self.D.capital_cholinv_lowrank_prepare(self.p, float(shift), dv.ctypes.data_as(_dp) if dv is not None else None, int(bool(schur)),
                                                   C.byref(ld), C.byref(cn)), "lowrank_prepare")
        self._lowrank = {"logdet": ld.value, "cnorm1": cn.value, "rank": getattr(self, "pivot_rank", 0)}
        return dict(self._lowrank)

    def lowrank_solve(self, B, residual=True):
        """X = M^-1 B with the M = L L^T + D of the last lowrank_prepare() (cholesky::cholinv::lowrank_solve, one rank): X = D^-1 (B - L T),
        T = C^-1 (L^T (D^-1 B)), in blocks of 32 columns; L is read twice per block as it lies, the rank x rank substitutions are capi_dtrsm_thin's.
        B: n x r.  Returns (X, resnorms): resnorms[j] = ||b_j - M x_j||_2 with M x = L (L^T x) + D x, from L and d alone, or None with
        residual=False.  The X of solve() stays as it is."""
        b = self._thin_block(B, "lowrank_solve")
        r = b.shape[1]
        X = np.zeros((self.n, r), order="F")
        res = np.zeros(r) if residual else None
        _ck(self.D.capital_cholinv_lowrank_solve(self.p, r, b.ctypes.data_as(_dp), X.ctypes.data_as(_dp), res.ctypes.data_as(_dp) if residual else None),
            "lowrank_solve")
        return X, res

    def lowrank_quadratic_forms(self, B):
        """q[j] = b_j^T M^-1 b_j = sum_i b_ij^2 / d_i - ||R_c^-T L^T D^-1 b_j||^2 with the M of the last lowrank_prepare()
        (cholesky::cholinv::lowrank_quadratic_forms, one rank): half a lowrank_solve -- one pass over L and one substitution.  B: n x r.  Returns r values."""
        b = self._thin_block(B, "lowrank_quadratic_forms")
        q = np.zeros(b.shape[1])
        _ck(self.D.capital_cholinv_lowrank_quadratic_forms(self.p, b.shape[1], b.ctypes.data_as(_dp), q.ctypes.data_as(_dp)), "lowrank_quadratic_forms")
        return q

    def lowrank_logdet(self):
        """log det (L L^T + D) = sum_i log d_i + 2 sum_i log (R_c)_ii as the last lowrank_prepare() found it"""
        if getattr(self, "_lowrank", None) is None:
            raise DriverError("Cholinv.lowrank_logdet: lowrank_prepare() has not run or did not succeed")
        return self._lowrank["logdet"]

    def _get(self, which):
        out = np.zeros((self.n_loc, self.n_loc), order="F")
        _ck(self.D.capital_cholinv_get(self.p, which, out.ctypes.data_as(_dp)), "get")
        return out

    def A(self):
        return self._get(0)

    def R(self):
        return self._get(1)

    def Rinv(self):
        return self._get(2)

    def rows(self, which, rows):
        """Local rows `rows` of R (which = 'R') or R^-1 ('Rinv') as a len(rows) x n_loc array -- a sample of a factor too large to fetch whole."""
        idx = np.ascontiguousarray(rows, dtype=np.int64)
        out = np.zeros((len(idx), self.n_loc), order="F")
        _ck(self.D.capital_cholinv_get_rows(self.p, {"R": 1, "Rinv": 2}[which], len(idx), idx.ctypes.data_as(C.POINTER(_i64)),
                                            out.ctypes.data_as(_dp)), "get_rows")
        return out

    def stats(self):
        a, b, c_ = _i64(), _i64(), _i64()
        _ck(self.D.capital_cholinv_stats(self.p, C.byref(a), C.byref(b), C.byref(c_)), "stats")
        return {"base_cases": a.value, "levels": b.value, "bc_dimension": c_.value}

    def close(self):
        if self.p:
            self.D.capital_cholinv_destroy(self.p)
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Cacqr:
    """qr::cacqr<SP,SaveIntermediates>::factor on this process's row-cyclic block of an m x n matrix
    (bench/qr/cacqr.cpp:14-25: variant 1 = CholeskyQR, 2 = CholeskyQR2; up to 4 sweeps).  shifted: the first `shifted` of the `variant`
    sweeps are shifted CholeskyQR sweeps (kappa(A) beyond 1e8: variant=3, shifted=1 up to ~1e10, variant=4, shifted=2 up to ~1e12; c = 1);
    shift_scale multiplies the published shift."""

    def __init__(self, m, n, c=1, variant=2, complete_inv=0, split=1, bc_mult=0, layout=0, num_chunks=0, serialize=True, shifted=0,
                 shift_scale=1.0):
        self.D = load()
        self.p = self.D.capital_cacqr_create(m, n, c, variant, layout, num_chunks, int(complete_inv), split, bc_mult, int(serialize))
        if not self.p:
            raise DriverError("capital_cacqr_create: " + self.D.capital_drv_last_error().decode())
        self.variant, self.shifted = variant, shifted
        self.rank, self.piv = 0, None
        if shifted or shift_scale != 1.0:
            _ck(self.D.capital_cacqr_set_shift(self.p, shifted, shift_scale), "set_shift")
        ml, nn = _i64(), _i64()
        _ck(self.D.capital_cacqr_dims(self.p, C.byref(ml), C.byref(nn)), "dims")
        self.m, self.n, self.m_loc = m, nn.value, ml.value

    def generate(self):
        _ck(self.D.capital_cacqr_generate(self.p), "generate")

    def set_A(self, A_local):
        a = np.asfortranarray(A_local, dtype=np.float64)
        assert a.shape == (self.m_loc, self.n)
        _ck(self.D.capital_cacqr_set_A(self.p, a.ctypes.data_as(_dp)), "set_A")

    def factor(self):
        _ck(self.D.capital_cacqr_factor(self.p), "factor")

    def factor_pivoted(self, rtol=0.0, tol_scale=1.0):
        """Column-pivoted CholeskyQR for a panel whose columns may be linearly dependent (qr::cacqr::factor_pivoted, 1-D variant): A[:, piv] = Q R with Q
        m x rank orthonormal and R rank x n upper trapezoidal.  A column is dropped when, after projecting out the accepted ones, its squared norm is at
        most tol trace(A^T A), tol = tol_scale max(rtol^2, 11 (m n + n (n + 1)) u): relative to ||A||_F the rank threshold is sqrt(tol), the Gram matrix's
        own noise level (about 1e-5 at 2048 x 32) -- rtol above it gives a truncated pivoted QR.  Returns the numerical rank; afterwards .rank, .piv,
        R_pivoted(), Q_pivoted(), and lstsq() gives the basic solution (zeros in the dropped columns)."""
        rk = _int(0)
        self.rank, self.piv = 0, None
        _ck(self.D.capital_cacqr_factor_pivoted(self.p, float(rtol), float(tol_scale), C.byref(rk)), "factor_pivoted")
        piv = np.zeros(self.n, dtype=np.int64)
        _ck(self.D.capital_cacqr_get_piv(self.p, piv.ctypes.data_as(C.POINTER(_i64))), "get_piv")
        self.rank, self.piv = rk.value, piv
        return self.rank

    def R_pivoted(self):
        """R of the last factor_pivoted(), rank x n upper trapezoidal: A[:, piv] = Q_pivoted() @ R_pivoted(); the same bits on every rank"""
        return np.asfortranarray(self._get(4, (self.n, self.n))[:self.rank])

    def Q_pivoted(self):
        """this rank's rows of the orthonormal factor of the last factor_pivoted(), m_loc x rank"""
        return np.asfortranarray(self._get(1, (self.m_loc, self.n))[:, :self.rank])

    def sweep_stats(self):
        """Per sweep of the last factor() of a run with shifted sweeps: the shift s, the trace of the equilibrated Gram matrix (both 0
        for a plain sweep) and cond_bound = ||R'||_1 ||R'||_inf ||R'^-1||_1 ||R'^-1||_inf of the sweep's Gram matrix G' = R'^T R'
        (cond_2(G') <= cond_bound <= n^2 cond_2(G'); 1 for an orthonormal panel).  Watch the first plain sweep: below ~1e15 it is
        safe, above ~1e16 n^2 a further shifted sweep is needed."""
        out = []
        for k in range(max(1, self.variant)):
            v = (_dbl * 3)()
            _ck(self.D.capital_cacqr_sweep_stats(self.p, k, v), "sweep_stats")
            out.append({"shift": v[0], "trace": v[1], "cond_bound": v[2]})
        return out

    def lstsq(self, B_local, residual=True):
        """min ||A X - B||_F on the factors of the last factor() (qr::cacqr::least_squares, 1-D variant): X = R^-1 (Q^T B) on the device.
        B_local: this rank's m_loc x r block of the right-hand sides, rows dealt as A's.  Returns (X, resnorms): X n x r, the same bits
        on every rank; resnorms[j] = ||b_j - A x_j||_2 over all ranks, or None with residual=False."""
        b = np.asfortranarray(B_local, dtype=np.float64)
        if b.ndim == 1:
            b = np.asfortranarray(b[:, None])
        assert b.ndim == 2 and b.shape[0] == self.m_loc and b.shape[1] >= 1
        r = b.shape[1]
        X = np.zeros((self.n, r), order="F")
        res = np.zeros(r) if residual else None
        _ck(self.D.capital_cacqr_lstsq(self.p, r, b.ctypes.data_as(_dp), X.ctypes.data_as(_dp), res.ctypes.data_as(_dp) if residual else None), "lstsq")
        return X, res

    def svd(self, left=True):
        """The singular value decomposition of A on the factors of the last factor() (qr::cacqr::svd, 1-D variant): R = U_R diag(s) V^T by one-sided
        Jacobi on the device (capi_dgesvj), then U = Q U_R on this rank's rows.  Returns (U_local or None, s, V) with A = U diag(s) V^T: U_local
        m_loc x n (None with left=False, which touches no m x n memory), s the n singular values, descending, V n x n -- s and V the same bits on
        every rank.  self.svd_sweeps: the Jacobi sweeps the call took."""
        U = np.zeros((self.m_loc, self.n), order="F") if left else None
        s = np.zeros(self.n)
        V = np.zeros((self.n, self.n), order="F")
        sw = _int()
        _ck(self.D.capital_cacqr_svd(self.p, int(bool(left)), U.ctypes.data_as(_dp) if left else None, s.ctypes.data_as(_dp), V.ctypes.data_as(_dp),
                                     C.byref(sw)), "svd")
        self.svd_sweeps = sw.value
        return U, s, V

    def residual(self):
        v = _dbl()
        _ck(self.D.capital_cacqr_residual(self.p, C.byref(v)), "residual")
        return v.value

    def orthogonality(self):
        v = _dbl()
        _ck(self.D.capital_cacqr_orthogonality(self.p, C.byref(v)), "orthogonality")
        return v.value

    def _get(self, which, shape):
        out = np.zeros(shape, order="F")
        _ck(self.D.capital_cacqr_get(self.p, which, out.ctypes.data_as(_dp)), "get")
        return out

    def A(self):
        return self._get(0, (self.m_loc, self.n))

    def Q(self):
        return self._get(1, (self.m_loc, self.n))

    def R(self):
        return self._get(2, (self.n, self.n))

    def gram_of_Q(self):
        """Q^T Q summed over the ranks (n x n): what the orthogonality validator measures against I."""
        return self._get(3, (self.n, self.n))

    def rows(self, which, row0, nrows):
        """Local rows [row0, row0 + nrows) of A (which = 'A') or Q ('Q') -- a bounded window of a panel too large to fetch whole."""
        out = np.zeros((nrows, self.n), order="F")
        _ck(self.D.capital_cacqr_get_rows(self.p, {"A": 0, "Q": 1}[which], row0, nrows, out.ctypes.data_as(_dp)), "get_rows")
        return out

    def close(self):
        if self.p:
            self.D.capital_cacqr_destroy(self.p)
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
