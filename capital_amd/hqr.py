"""Householder QR on the C-ABI: capi_dgeqrf, capi_dormqr, capi_dgels and capi_dtrsm_thin behind one object, numpy in and numpy out as the driver
classes are.  The unconditionally stable route for least squares: kappa(A) up to 1 / u, or unknown ("Householder least squares").

    h = capi.Handle()
    q = Hqr(h, A)                 # A: m x n, m >= n
    X, res = q.lstsq(B)           # factors on the first call; later calls reuse the factors
    QtB = q.apply_qt(B); B2 = q.apply_q(QtB)
    q.close()

Rank-deficient or numerically rank-deficient A ("Rank-deficient Householder least squares"): capi_dgeqp3 and capi_dgelsy.

    q = Hqr(h, A)
    X, res, k = q.lstsq_pivoted(B, rcond=1e-13)          # the minimum-norm solution; min_norm=False: the basic one
    k = q.factor_pivoted(rcond=1e-10)                    # another threshold: only the n x n triangle is pivoted again; q.rank, q.jpvt
"""
import ctypes as C

import numpy as np
import torch

from . import capi


class Hqr:
    def __init__(self, handle, A):
        A = np.asarray(A, dtype=np.float64)
        if A.ndim != 2 or A.shape[0] < A.shape[1] or A.shape[1] < 1:
            raise ValueError("Hqr: A must be m x n with m >= n >= 1")
        self.hip = handle
        self.m, self.n = A.shape
        self.dA = capi.to_device(A, handle.device)
        self.dtau = torch.zeros(self.n, dtype=torch.float64, device=f"cuda:{handle.device}")
        self.factored = False
        # the pivoted factors of R1 (factor_pivoted / lstsq_pivoted): F, tauf, jpvt as capi_dgeqp3 leaves them, Z, tauz of [R11 R12]^T
        self.rank = None
        self.jpvt = None
        self.dF = self.dtauf = self.djpvt = self.dZ = self.dtauz = None
        self._rcond = None
        self._have_z = False

    def _need(self):
        if self.dA is None:
            raise capi.CapiError("Hqr: closed")

    def factor(self):
        """A <- capi_dgeqrf's image (R above, the reflectors below), tau"""
        self._need()
        if not self.factored:
            torch.cuda.synchronize()
            self.hip.call("capi_dgeqrf", self.m, self.n, capi.ptr(self.dA), self.m, capi.ptr(self.dtau))
            self.factored = True
        return self

    def R(self):
        self.factor()
        self.hip.sync()
        return np.triu(capi.to_host(self.dA)[:self.n])

    def _block(self, B):
        B = np.asarray(B, dtype=np.float64)
        one = B.ndim == 1
        B = B.reshape(self.m, -1) if one else B
        if B.ndim != 2 or B.shape[0] != self.m or B.shape[1] < 1:
            raise ValueError(f"Hqr: B must have {self.m} rows and at least one column")
        return capi.to_device(B, self.hip.device), one

    def _apply(self, B, trans):
        self.factor()
        dB, one = self._block(B)
        torch.cuda.synchronize()
        self.hip.call("capi_dormqr", capi.LEFT, trans, self.m, dB.shape[0], self.n, capi.ptr(self.dA), self.m, capi.ptr(self.dtau), capi.ptr(dB),
                      self.m)
        self.hip.sync()
        out = capi.to_host(dB)
        return out[:, 0] if one else out

    def apply_qt(self, B):
        """Q^T B (m x r), Q the full m x m orthogonal factor"""
        return self._apply(B, capi.TRANS)

    def apply_q(self, B):
        """Q B (m x r)"""
        return self._apply(B, capi.NOTRANS)

    def lstsq(self, B, residual=True):
        """(X, resnorms): X (n x r) minimises ||A X - B||_F column by column; resnorms[j] = ||b_j - A x_j||_2, or None with residual=False.
        Raises capi.CapiError naming the column of R whose diagonal entry is zero or not finite."""
        self._need()
        dB, one = self._block(B)
        r = dB.shape[0]
        dev = f"cuda:{self.hip.device}"
        torch.cuda.synchronize()
        if not self.factored:                                   # the first solve factors: capi_dgels
            dn = torch.zeros(r, dtype=torch.float64, device=dev) if residual else None
            info = C.c_int(0)
            self.hip.call("capi_dgels", self.m, self.n, r, capi.ptr(self.dA), self.m, capi.ptr(self.dtau), capi.ptr(dB), self.m, capi.ptr(dn),
                          C.byref(info))
            self.factored = True
            if info.value != 0:
                raise capi.CapiError(f"Hqr.lstsq: R({info.value}, {info.value}) is zero or not finite (column {info.value}): A is rank deficient")
            self.hip.sync()
            norms = None if dn is None else np.sqrt(dn.cpu().numpy())
        else:                                                   # further right-hand sides on the factors
            d = torch.diagonal(self.dA[:, :self.n])
            bad = torch.nonzero((d == 0) | ~torch.isfinite(d))
            if bad.numel():
                j = int(bad[0]) + 1
                raise capi.CapiError(f"Hqr.lstsq: R({j}, {j}) is zero or not finite (column {j}): A is rank deficient")
            self.hip.call("capi_dormqr", capi.LEFT, capi.TRANS, self.m, r, self.n, capi.ptr(self.dA), self.m, capi.ptr(self.dtau), capi.ptr(dB), self.m)
            norms = np.empty(r) if residual else None
            for j in range(0, r, 32):
                rb = min(32, r - j)
                blk = dB[j:j + rb]
                self.hip.call("capi_dtrsm_thin", capi.NOTRANS, self.n, rb, capi.ptr(self.dA), self.m, 0, capi.ptr(blk), self.m)
                if residual:
                    dn = torch.zeros(rb, dtype=torch.float64, device=dev)
                    self.hip.call("capi_dcolnorm2", self.m - self.n, rb, capi.ptr(blk) + 8 * self.n, self.m, capi.ptr(dn))
                    self.hip.sync()
                    norms[j:j + rb] = np.sqrt(dn.cpu().numpy())
            self.hip.sync()
        X = capi.to_host(dB)[:self.n]
        if one:
            return X[:, 0], (None if norms is None else norms[0])
        return X, norms

    def _pivoted_buffers(self):
        if self.dF is None:
            dev = f"cuda:{self.hip.device}"
            n = self.n
            self.dF = torch.zeros((n, n), dtype=torch.float64, device=dev)
            self.dZ = torch.zeros((n, n), dtype=torch.float64, device=dev)
            self.dtauf = torch.zeros(n, dtype=torch.float64, device=dev)
            self.dtauz = torch.zeros(n, dtype=torch.float64, device=dev)
            self.djpvt = torch.zeros(n, dtype=torch.int32, device=dev)

    def _pivoted_done(self, k, rcond):
        self.hip.sync()
        self.rank = k
        self.jpvt = self.djpvt.cpu().numpy().copy()
        self._rcond = rcond

    def _factor_z(self):
        """Z <- [R11 R12]^T from F's upper trapezoid (a copy: zeros where F holds its reflectors), then capi_dgeqrf(n, k, Z, tauz)"""
        n, k = self.n, self.rank
        if not self._have_z and 0 < k < n:
            self.dZ[:k] = torch.triu(self.dF[:, :k].T)
            torch.cuda.synchronize()
            self.hip.call("capi_dgeqrf", n, k, capi.ptr(self.dZ), n, capi.ptr(self.dtauz))
        self._have_z = True

    def factor_pivoted(self, rcond=None):
        """k = the numerical rank of A at rcond (None: max(m, n) 2^-52): capi_dgeqrf once, then capi_dgeqp3 on triu(R1); sets .rank and .jpvt (column j
        of A P is column jpvt[j] of A).  A call with another rcond pivots the n x n triangle again: R1 is still in the image, A is not factored again."""
        self._need()
        rc = -1.0 if rcond is None else float(rcond)
        if self.rank is not None and rc == self._rcond:
            return self.rank
        self.factor()
        self._pivoted_buffers()
        n = self.n
        torch.cuda.synchronize()
        self.hip.call("capi_dlacpy", 1, n, n, capi.ptr(self.dA), self.m, capi.ptr(self.dF), n)
        self.hip.call("capi_dtrizero", capi.UPPER, n, capi.ptr(self.dF), n)
        k = C.c_int(0)
        self.hip.call("capi_dgeqp3", n, n, capi.ptr(self.dF), n, capi.ptr(self.djpvt), capi.ptr(self.dtauf),
                      self.m * 2.0 ** -52 if rc < 0 else rc, C.byref(k))
        self._have_z = False
        self._pivoted_done(k.value, rc)
        return self.rank

    def lstsq_pivoted(self, B, rcond=None, min_norm=True, residual=True):
        """(X, resnorms, rank): X (n x r) minimises ||A X - B||_F column by column for A of any rank -- with min_norm the solution of least norm, without
        the basic one (nonzeros in rows jpvt[:rank] only); resnorms[j] = ||b_j - A x_j||_2, or None with residual=False.  The first call runs
        capi_dgelsy; later calls run on the factors (capi_dgelsy's header comment gives the sequence)."""
        self._need()
        dB, one = self._block(B)
        r = dB.shape[0]
        m, n = self.m, self.n
        dev = f"cuda:{self.hip.device}"
        rc = -1.0 if rcond is None else float(rcond)
        dn = torch.zeros(r, dtype=torch.float64, device=dev) if residual else None
        torch.cuda.synchronize()
        if not self.factored and self.rank is None:             # the first solve factors: capi_dgelsy
            self._pivoted_buffers()
            k = C.c_int(0)
            self.hip.call("capi_dgelsy", m, n, r, capi.ptr(self.dA), m, capi.ptr(self.dtau), capi.ptr(self.dF), n, capi.ptr(self.dtauf),
                          capi.ptr(self.djpvt), capi.ptr(self.dZ) if min_norm else None, n, capi.ptr(self.dtauz) if min_norm else None, capi.ptr(dB), m,
                          rc, 1 if min_norm else 0, capi.ptr(dn), C.byref(k))
            self.factored = True
            self._have_z = bool(min_norm)
            self._pivoted_done(k.value, rc)
            X = capi.to_host(dB)[:n]
        else:                                                   # further right-hand sides on the factors
            k = self.factor_pivoted(rcond)
            mn = bool(min_norm) and 0 < k < n
            if mn:
                self._factor_z()
            self.hip.call("capi_dormqr", capi.LEFT, capi.TRANS, m, r, n, capi.ptr(self.dA), m, capi.ptr(self.dtau), capi.ptr(dB), m)
            self.hip.call("capi_dormqr", capi.LEFT, capi.TRANS, n, r, k, capi.ptr(self.dF), n, capi.ptr(self.dtauf), capi.ptr(dB), m)
            for j in range(0, r, 32):
                rb = min(32, r - j)
                pj = capi.ptr(dB[j:j + rb])
                if residual:
                    self.hip.call("capi_dcolnorm2", m - k, rb, pj + 8 * k, m, capi.ptr(dn[j:j + rb]))
                if k > 0:
                    self.hip.call("capi_dtrsm_thin", capi.TRANS if mn else capi.NOTRANS, k, rb, capi.ptr(self.dZ if mn else self.dF), n, 0, pj, m)
            if mn:
                dB[:, k:n] = 0.0
                torch.cuda.synchronize()
                self.hip.call("capi_dormqr", capi.LEFT, capi.NOTRANS, n, r, k, capi.ptr(self.dZ), n, capi.ptr(self.dtauz), capi.ptr(dB), m)
            dX = torch.empty((r, n), dtype=torch.float64, device=dev)
            self.hip.call("capi_drow_scatter", 0, n if mn else k, r, n, capi.ptr(dB), m, capi.ptr(self.djpvt), capi.ptr(dX), n)
            self.hip.sync()
            X = capi.to_host(dX)
        norms = None if dn is None else np.sqrt(dn.cpu().numpy())
        if one:
            return X[:, 0], (None if norms is None else norms[0]), self.rank
        return X, norms, self.rank

    def close(self):
        self.dA = None
        self.dtau = None
        self.dF = self.dtauf = self.djpvt = self.dZ = self.dtauz = None
