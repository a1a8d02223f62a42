"""One SHA-256 per output array of the thin kernels (capi_dgemtn_ts, capi_dresid_ts, capi_dtrmm_thin, capi_dresid_sym, capi_dtri_rownorm2,
capi_dtri_logdiag, capi_dtrsm_thin, capi_dchud + capi_dchud_inv, capi_dsym_abs) on a fixed list of cases with fixed seeds: run it under two builds of the library (CAPITAL_HIP_LIB) and diff the two outputs -- a refactor of these kernels leaves every line as
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

    # ---- the triangles of the cases below: order n with a dominant positive diagonal, as a view at an odd col0 of a larger packed triangle whose other
    # words hold values too, and column-major with a padded ld (values below the diagonal and in the padding).  Returns host arrays and view offsets ----
    COL0 = 129

    def packed_host(rng, n, scale=1.0):
        a = scale * rng.standard_normal(pstart(COL0 + n))
        for j in range(n):
            e = pstart(COL0 + j) + COL0 + j
            a[e] = 4.0 * np.sqrt(n) + abs(a[e])
        return a, pstart(COL0) + COL0

    def full_host(rng, n, ld, scale=1.0):
        a = scale * rng.standard_normal(ld * n)
        d = np.arange(n) * (ld + 1)
        a[d] = 4.0 * np.sqrt(n) + np.abs(a[d])
        return a, 0

    def triangles(seed, n, scale=1.0):
        """[(name, host array, offset of the view's first element, ldt, col0)]"""
        hp, op = packed_host(np.random.default_rng(seed + [0]), n, scale)
        hf, of = full_host(np.random.default_rng(seed + [1]), n, n + 3, scale)
        return (("packed", hp, op, 0, COL0), ("full", hf, of, n + 3, 0))

    # ---- capi_dtri_rownorm2, capi_dtri_logdiag ----
    for n in (300, 777):
        for store, host, off, ldt, c0 in triangles([7, n], n):
            T = dev(host)
            pT = T.data_ptr() + 8 * off
            rng = np.random.default_rng([8, n, ldt])
            o = out(rng, n + 2, 1)
            h.call("capi_dtri_rownorm2", UPPERTRI, n, n, pT, ldt, c0, 0.0, o.data_ptr())
            print(f"dtri_rownorm2 tri n{n} {store} beta0 out {sha(o)}")
            h.call("capi_dtri_rownorm2", UPPERTRI, n, n, pT, ldt, c0, 1.0, o.data_ptr())
            print(f"dtri_rownorm2 tri n{n} {store} beta1 out {sha(o)}")
            ld1 = out(rng, 3, 1)
            h.call("capi_dtri_logdiag", n, pT, ldt, c0, ld1.data_ptr())
            print(f"dtri_logdiag n{n} {store} out {sha(ld1)}")
            if store == "packed":
                # a rectangle inside the packed triangle: rows 0 .. m - 1 of its columns col0 .., m <= col0
                m = 100
                pR = T.data_ptr() + 8 * pstart(c0)
                o = out(rng, m + 2, 1)
                h.call("capi_dtri_rownorm2", RECT, m, n, pR, 0, c0, 0.0, o.data_ptr())
                print(f"dtri_rownorm2 rect {m}x{n} packed beta0 out {sha(o)}")
                h.call("capi_dtri_rownorm2", RECT, m, n, pR, 0, c0, 1.0, o.data_ptr())
                print(f"dtri_rownorm2 rect {m}x{n} packed beta1 out {sha(o)}")
    for m, n in ((5, 300), (777, 129)):
        rng = np.random.default_rng([9, m, n])
        ld = m + 1
        T = dev(rng.standard_normal(ld * n))
        o = out(rng, m + 2, 1)
        h.call("capi_dtri_rownorm2", RECT, m, n, T.data_ptr(), ld, 0, 0.0, o.data_ptr())
        print(f"dtri_rownorm2 rect {m}x{n} full beta0 out {sha(o)}")
        h.call("capi_dtri_rownorm2", RECT, m, n, T.data_ptr(), ld, 0, 1.0, o.data_ptr())
        print(f"dtri_rownorm2 rect {m}x{n} full beta1 out {sha(o)}")

    # ---- capi_dtrsm_thin (n = 777: two leaves and a rectangular product between them) ----
    for n in (300, 777):
        for store, host, off, ldt, c0 in triangles([10, n], n):
            T = dev(host)
            pT = T.data_ptr() + 8 * off
            for r in (1, 5, 32):
                for trans in (0, 1):
                    rng = np.random.default_rng([11, n, r, trans, ldt])
                    B = out(rng, (n + 3) * r, 1)
                    h.call("capi_dtrsm_thin", trans, n, r, pT, ldt, c0, B.data_ptr(), n + 3)
                    print(f"dtrsm_thin n{n} r{r} t{trans} {store} B {sha(B)}")

    # ---- capi_dchud, capi_dchud_inv: T, V and the log of the factor; the inverse in one range and in two ----
    import ctypes as C
    for n in (300, 777):
        for r in (1, 17, 32):
            for sign in (1, -1):
                for store, host, off, ldt, c0 in triangles([12, n], n):
                    rng = np.random.default_rng([13, n, r, sign + 1, ldt])
                    T = dev(host)
                    V = dev(0.05 * rng.standard_normal((n + 2) * r))
                    lg = dev(np.zeros(h.L.capi_dchud_log_bytes(n, r) // 8 + 3))
                    info = C.c_int(-99)
                    h.call("capi_dchud", sign, n, r, T.data_ptr() + 8 * off, ldt, c0, V.data_ptr(), n + 2, lg.data_ptr(), C.byref(info))
                    tag = f"n{n} r{r} s{sign:+d} {store}"
                    print(f"dchud {tag} info {info.value} T {sha(T)} V {sha(V)} log {sha(lg)}")
                    ihost = triangles([14, n], n, 0.01)[0 if ldt == 0 else 1][1]
                    Ti = dev(ihost)
                    h.call("capi_dchud_inv", sign, n, r, Ti.data_ptr() + 8 * off, ldt, c0, lg.data_ptr(), 0, n)
                    print(f"dchud_inv {tag} [0,{n}) Tinv {sha(Ti)}")
                    Ti = dev(ihost)
                    h1 = n // 2 + 1
                    h.call("capi_dchud_inv", sign, n, r, Ti.data_ptr() + 8 * off, ldt, c0, lg.data_ptr(), 0, h1)
                    h.call("capi_dchud_inv", sign, n, r, Ti.data_ptr() + 8 * off, ldt, c0, lg.data_ptr(), h1, n)
                    print(f"dchud_inv {tag} [0,{h1})+[{h1},{n}) Tinv {sha(Ti)}")

    # ---- capi_dsym_abs ----
    for n in (300, 777):
        for lda in (n, n + 3):
            rng = np.random.default_rng([15, n, lda])
            A = dev(rng.standard_normal(lda * n))                         # the lower triangle and the padding hold values: they take no part
            for r in (5, 20):
                rng = np.random.default_rng([16, n, lda, r])
                X, B = dev(rng.standard_normal((n + 1) * r)), dev(rng.standard_normal((n + 2) * r))
                tag = f"n{n} lda{lda} r{r}"
                W, cm = out(rng, (n + 4) * r, 1), out(rng, r + 1, 1)
                h.call("capi_dsym_abs", n, r, A.data_ptr(), lda, X.data_ptr(), n + 1, B.data_ptr(), n + 2, W.data_ptr(), n + 4, cm.data_ptr())
                print(f"dsym_abs {tag} B W {sha(W)} colmax {sha(cm)}")
                h.call("capi_dsym_abs", n, r, A.data_ptr(), lda, X.data_ptr(), n + 1, None, 0, W.data_ptr(), n + 4, cm.data_ptr())
                print(f"dsym_abs {tag} no-B W {sha(W)} colmax {sha(cm)}")
                h.call("capi_dsym_abs", n, r, A.data_ptr(), lda, X.data_ptr(), n + 1, B.data_ptr(), n + 2, None, 0, cm.data_ptr())
                print(f"dsym_abs {tag} B no-W colmax {sha(cm)}")
                h.call("capi_dsym_abs", n, r, A.data_ptr(), lda, X.data_ptr(), n + 1, None, 0, W.data_ptr(), n + 4, None)
                print(f"dsym_abs {tag} no-B W-only W {sha(W)}")
    h.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
