"""One SHA-256 per output array of the thin kernels (capi_dgemtn_ts, capi_dresid_ts, capi_dtrmm_thin, capi_dresid_sym) on a fixed list of cases with
fixed seeds: run it under two builds of the library (CAPITAL_HIP_LIB) and diff the two outputs -- a refactor of these kernels leaves every line as
it is.  The shapes are the GPU tests' small ones: ragged tiles, the diagonal's tiles, r <= 16 and r > 16, both routes of capi_dresid_sym, the edge
loaders (odd and padded leading dimensions, an unaligned base, packed storage at an odd col0).  Every output buffer is hashed whole, padding rows
included, so a stray write shows too.

    python tools/thin_bits.py > bits.txt"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RECT, UPPERTRI = 0, 1


def main():
    import torch
    from capital_amd import capi
    h = capi.Handle(0)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def colmajor(rng, m, n, ld, off=0):
        """an m x n standard-normal matrix with leading dimension ld, `off` doubles into its buffer (off = 1: an 8-byte-aligned base); the padding
        holds values too.  Returns the tensor and the device pointer of element (0, 0)"""
        t = dev(rng.standard_normal(off + ld * max(n, 1)))
        return t, t.data_ptr() + 8 * off

    def sha(t):
        h.sync()
        return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()

    def out(rng, ld, r, nan=False):
        return dev(np.full(ld * r, np.nan) if nan else rng.standard_normal(ld * r))

    # ---- capi_dgemtn_ts, capi_dresid_ts ----
    for m in (777, 4099):
        for n in (5, 33, 300):
            for r in (1, 16, 17, 32):
                # (lda, ldb, unaligned base of A): padded and even, odd, and the aligned even ld behind an 8-byte-aligned base
                for lda, ldb, off in ((m + (m & 1) + 2, m + (m & 1), 0), (m + 1 - (m & 1), m + 3 - (m & 1), 0), (m + (m & 1), m + (m & 1), 1)):
                    rng = np.random.default_rng([1, m, n, r, lda, off])
                    tA, pA = colmajor(rng, m, n, lda, off)
                    tB, pB = colmajor(rng, m, r, ldb)
                    tX, pX = colmajor(rng, n, r, n + 1)
                    C = out(rng, (n + 2) * r, 1)
                    tag = f"m{m} n{n} r{r} lda{lda} ldb{ldb} off{off}"
                    h.call("capi_dgemtn_ts", m, n, r, 1.0, pA, lda, pB, ldb, 0.0, C.data_ptr(), n + 2)
                    print(f"dgemtn_ts {tag} beta0 C {sha(C)}")
                    h.call("capi_dgemtn_ts", m, n, r, -0.5, pA, lda, pB, ldb, 2.0, C.data_ptr(), n + 2)
                    print(f"dgemtn_ts {tag} beta2 C {sha(C)}")
                    R, nrm = out(rng, ldb, r), out(rng, r, 1)
                    h.call("capi_dresid_ts", m, n, r, pA, lda, pX, n + 1, pB, ldb, R.data_ptr(), ldb, nrm.data_ptr())
                    print(f"dresid_ts {tag} Rout {sha(R)} colnorm2 {sha(nrm)}")
                    h.call("capi_dresid_ts", m, n, r, pA, lda, pX, n + 1, pB, ldb, None, 0, nrm.data_ptr())
                    print(f"dresid_ts {tag} norms-only colnorm2 {sha(nrm)}")
                    del tA, tB, tX

    # ---- capi_dtrmm_thin ----
    def pstart(x):
        return x * (x + 1) // 2

    for n in (300, 1000, 2100):
        rng = np.random.default_rng([2, n])
        col0 = 129                                                        # the triangle is a view at an odd col0 of a larger packed one
        big = dev(rng.standard_normal(pstart(col0 + n)))
        p_packed = big.data_ptr() + 8 * (pstart(col0) + col0)
        ld = n + 3
        full = dev(rng.standard_normal(ld * n))
        for r in (1, 17, 32):
            for trans in (0, 1):
                for store, pT, ldt, c0 in (("packed", p_packed, 0, col0), ("full", full.data_ptr(), ld, 0)):
                    rng = np.random.default_rng([3, n, r, trans, ldt])
                    B = dev(rng.standard_normal((n + 1) * r))
                    C = out(rng, (n + 5) * r, 1)
                    tag = f"tri n{n} r{r} t{trans} {store}"
                    h.call("capi_dtrmm_thin", UPPERTRI, trans, n, n, r, 1.0, pT, ldt, c0, B.data_ptr(), n + 1, 0.0, C.data_ptr(), n + 5)
                    print(f"dtrmm_thin {tag} a1b0 C {sha(C)}")
                    h.call("capi_dtrmm_thin", UPPERTRI, trans, n, n, r, -0.5, pT, ldt, c0, B.data_ptr(), n + 1, 2.0, C.data_ptr(), n + 5)
                    print(f"dtrmm_thin {tag} a-0.5b2 C {sha(C)}")
    for m, n in ((5, 300), (1000, 129)):
        for r in (1, 17, 32):
            for trans in (0, 1):
                rng = np.random.default_rng([4, m, n, r, trans])
                ld = m + 1
                T = dev(rng.standard_normal(ld * n))
                lines, depth = (n, m) if trans else (m, n)
                B = dev(rng.standard_normal(depth * r))
                C = out(rng, (lines + 2) * r, 1)
                tag = f"rect {m}x{n} r{r} t{trans} full"
                h.call("capi_dtrmm_thin", RECT, trans, m, n, r, 1.0, T.data_ptr(), ld, 0, B.data_ptr(), depth, 0.0, C.data_ptr(), lines + 2)
                print(f"dtrmm_thin {tag} a1b0 C {sha(C)}")
                h.call("capi_dtrmm_thin", RECT, trans, m, n, r, 0.5, T.data_ptr(), ld, 0, B.data_ptr(), depth, -1.0, C.data_ptr(), lines + 2)
                print(f"dtrmm_thin {tag} a0.5b-1 C {sha(C)}")

    # ---- capi_dresid_sym ----
    for n in (300, 1100, 2100):
        for lda in (n, n + 3):
            rng = np.random.default_rng([5, n, lda])
            A = dev(rng.standard_normal(lda * n))                         # the lower triangle and the padding hold values: they take no part
            for r in (1, 7, 8, 32):
                rng = np.random.default_rng([6, n, lda, r])
                X, B = dev(rng.standard_normal((n + 1) * r)), dev(rng.standard_normal((n + 2) * r))
                tag = f"n{n} lda{lda} r{r}"
                R, nrm = out(rng, (n + 4) * r, 1), out(rng, r, 1)
                h.call("capi_dresid_sym", n, r, A.data_ptr(), lda, X.data_ptr(), n + 1, B.data_ptr(), n + 2, R.data_ptr(), n + 4, nrm.data_ptr())
                print(f"dresid_sym {tag} Rout {sha(R)} colnorm2 {sha(nrm)}")
                h.call("capi_dresid_sym", n, r, A.data_ptr(), lda, X.data_ptr(), n + 1, B.data_ptr(), n + 2, R.data_ptr(), n + 4, None)
                print(f"dresid_sym {tag} Rout-only Rout {sha(R)}")
                h.call("capi_dresid_sym", n, r, A.data_ptr(), lda, X.data_ptr(), n + 1, B.data_ptr(), n + 2, None, 0, nrm.data_ptr())
                print(f"dresid_sym {tag} norms-only colnorm2 {sha(nrm)}")
    h.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
