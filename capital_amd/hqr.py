"""Householder QR on the C-ABI: capi_dgeqrf, capi_dormqr, capi_dgels and capi_dtrsm_thin behind one object, numpy in and numpy out as the driver
classes are.  The unconditionally stable route for least squares: kappa(A) up to 1 / u, or unknown ("Householder least squares").

    h = capi.Handle()
    q = Hqr(h, A)                 # A: m x n, m >= n
    X, res = q.lstsq(B)           # factors on the first call; later calls reuse the factors
    QtB = q.apply_qt(B); B2 = q.apply_q(QtB)
    q.close()
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

    def close(self):
        self.dA = None
        self.dtau = None
