"""capi_dgemtn_ts (C <- alpha A^T B + beta C) and capi_dresid_ts (Rout <- B - A X with its squared column norms), the streaming
tall-skinny kernels of capital_amd/csrc/ts_apply_f64.hip, against long double on the host.

The bounds are derived, not measured.  For any summation order |fl(a^T b) - a^T b| <= gamma_k |a|^T |b|, gamma_k = k u / (1 - k u),
u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1), so elementwise
    |C - C_ld|              <= gamma_(m+2) (|alpha| |A|^T |B| + |beta| |C0|)
    |Rout - (B - A X)_ld|   <= gamma_(n+2) (|B| + |A| |X|)
    |colnorm2 - sum Rout^2| <= gamma_(m+1) colnorm2          (the sum of the squares of the GPU's own Rout, in long double)
A kernel that drops a row tile, a column strip or a tail misses these by many orders."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SENTINEL = -7777.25          # guard rows between the columns of every output, and in front of offset pointers
LD = np.longdouble


def gamma(k):
    return k * U / (1.0 - k * U)


# (m, n, r, pad, off): a thinned product of m in {0, 1, 31, 4113, 65536}, n in {1, 16, 130, 256, 1000, 1024}, r in {1, 3, 8, 17, 32}; pad is added
# to every leading dimension (an odd leading dimension or off = 1, a pointer one double into its buffer, leaves 8-byte alignment only);
# (alpha, beta) alternate along the list
SHAPES = [(0, 16, 3, 0, 0), (0, 256, 32, 3, 1), (1, 1, 1, 0, 0), (1, 130, 17, 2, 1), (31, 16, 8, 1, 0), (31, 1000, 3, 0, 1), (31, 256, 32, 3, 0),
          (4113, 1, 1, 0, 0), (4113, 16, 17, 3, 0), (4113, 130, 3, 3, 0), (4113, 256, 8, 1, 1), (4113, 1000, 32, 0, 0), (4113, 1024, 1, 2, 1),
          (4113, 1024, 32, 1, 0), (65536, 16, 8, 0, 1), (65536, 130, 1, 2, 0), (65536, 256, 32, 0, 0), (65536, 1000, 3, 3, 0),
          (65536, 1024, 17, 0, 0), (65536, 256, 1, 1, 1)]
CASES = [(m, n, r, pad, off, ((1.0, 0.0), (-0.5, 2.0))[k % 2]) for k, (m, n, r, pad, off) in enumerate(SHAPES)]
IDS = [f"{m}x{n}-r{r}-pad{pad}-off{off}-a{ab[0]}b{ab[1]}" for m, n, r, pad, off, ab in CASES]


class Dev:
    """a column-major rows x cols window with leading dimension rows + pad, `off` doubles into a device buffer filled with SENTINEL"""

    def __init__(self, M, pad, off, fill=SENTINEL):
        import torch
        rows, cols = M.shape
        self.rows, self.cols, self.ld, self.off = rows, cols, max(1, rows + pad), off
        host = np.full(off + self.ld * cols + 2, fill)
        self._view(host)[:, :] = M
        self.t = torch.from_numpy(host).cuda()

    def _view(self, host):
        return host[self.off:self.off + self.ld * self.cols].reshape(self.cols, self.ld).T[:self.rows]

    @property
    def ptr(self):
        return self.t.data_ptr() + 8 * self.off

    def get(self):
        """(the window, whether everything outside it still holds the fill value)"""
        host = self.t.cpu().numpy()
        win = np.array(self._view(host), order="F")
        mask = np.ones(host.shape, bool)
        self._view(mask.view())[:, :] = False
        return win, host[mask]


def _inputs(m, n, r, seed):
    rng = np.random.default_rng(seed)
    return (np.asfortranarray(rng.standard_normal((m, n))), np.asfortranarray(rng.standard_normal((m, r))),
            np.asfortranarray(rng.standard_normal((n, r))))


def _gemtn(hip, dA, dB, dC, alpha, beta):
    hip.call("capi_dgemtn_ts", dA.rows, dA.cols, dB.cols, alpha, dA.ptr, dA.ld, dB.ptr, dB.ld, beta, dC.ptr, dC.ld)
    hip.sync()


def _resid(hip, dA, dX, dB, dR, norms):
    from capital_amd import capi
    hip.call("capi_dresid_ts", dA.rows, dA.cols, dX.cols, dA.ptr, dA.ld, dX.ptr, dX.ld, dB.ptr, dB.ld, dR.ptr if dR is not None else None,
             dR.ld if dR is not None else 0, capi.ptr(norms))
    hip.sync()


@pytest.mark.parametrize("m,n,r,pad,off,ab", CASES, ids=IDS)
def test_gemtn_against_long_double(hip, m, n, r, pad, off, ab):
    alpha, beta = ab
    A, B, C0 = _inputs(m, n, r, seed=m + n + r)
    dA, dB, dC = Dev(A, pad, off), Dev(B, pad + 1, off), Dev(C0, pad, off)
    _gemtn(hip, dA, dB, dC, alpha, beta)
    got, guard = dC.get()
    ref = LD(alpha) * (A.T.astype(LD) @ B.astype(LD)) + LD(beta) * C0.astype(LD)
    bound = gamma(m + 2) * (abs(alpha) * (np.abs(A).T @ np.abs(B)) + abs(beta) * np.abs(C0))
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    ratio = err / np.maximum(bound, 1e-300)
    print(f"gemtn {m}x{n} r={r}: max err / bound = {np.max(ratio):.3e}")
    assert np.all(err <= bound), (np.max(ratio), np.unravel_index(np.argmax(ratio), err.shape))
    assert np.all(guard == SENTINEL)                                        # nothing lands outside the n x r window
    dC2 = Dev(C0, pad, off)
    _gemtn(hip, dA, dB, dC2, alpha, beta)
    np.testing.assert_array_equal(dC2.get()[0], got)                       # bit-identical from run to run


@pytest.mark.parametrize("m,n,r,pad,off,ab", CASES, ids=IDS)
def test_resid_against_long_double(hip, m, n, r, pad, off, ab):
    import torch
    A, B, X = _inputs(m, n, r, seed=m + n + r + 1)
    dA, dB, dX = Dev(A, pad, off), Dev(B, pad + 1, off), Dev(X, pad + 2, off)
    dR = Dev(np.full((m, r), np.nan), pad + 3, off)
    norms = torch.full((r + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    _resid(hip, dA, dX, dB, dR, norms)
    got, guard = dR.get()
    ref = B.astype(LD) - A.astype(LD) @ X.astype(LD)
    bound = gamma(n + 2) * (np.abs(B) + np.abs(A) @ np.abs(X))
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    ratio = np.max(err / bound) if m else 0.0
    assert np.all(err <= bound), ratio
    assert np.all(guard == SENTINEL)
    nr = norms.cpu().numpy()
    own = np.sum(got.astype(LD) ** 2, axis=0).astype(np.float64)
    print(f"resid {m}x{n} r={r}: max err / bound = {ratio:.3e}, norms rel {np.max(np.abs(nr[:r] - own) / np.maximum(own, 1e-300)):.3e}")
    assert np.all(np.abs(nr[:r] - own) <= gamma(m + 1) * own), (nr[:r], own)
    assert nr[r] == SENTINEL
    assert np.all(dB.get()[0] == B) and np.all(dB.get()[1] == SENTINEL)      # the inputs are only read
    # twice the same bits; the norms alone; the residual alone; in place (Rout == B)
    dR2 = Dev(np.full((m, r), np.nan), pad + 3, off)
    norms2 = torch.full((r + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    _resid(hip, dA, dX, dB, dR2, norms2)
    np.testing.assert_array_equal(dR2.get()[0], got)
    np.testing.assert_array_equal(norms2.cpu().numpy(), nr)
    norms3 = torch.full((r + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    _resid(hip, dA, dX, dB, None, norms3)
    np.testing.assert_array_equal(norms3.cpu().numpy(), nr)
    dR4 = Dev(np.full((m, r), np.nan), pad + 3, off)
    _resid(hip, dA, dX, dB, dR4, None)
    np.testing.assert_array_equal(dR4.get()[0], got)
    norms5 = torch.full((r + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    _resid(hip, dA, dX, dB, dB, norms5)
    inplace, guard = dB.get()
    np.testing.assert_array_equal(inplace, got)
    np.testing.assert_array_equal(norms5.cpu().numpy(), nr)
    assert np.all(guard == SENTINEL)


def test_too_many_right_hand_sides_is_refused(hip):
    """r = 33: a non-zero status, the message names r, and neither output is touched"""
    import torch
    m, n, r = 300, 40, 33
    A, B, X = _inputs(m, n, r, seed=5)
    dA, dB, dX, dC = Dev(A, 0, 0), Dev(B, 0, 0), Dev(X, 0, 0), Dev(np.full((n, r), 3.5), 1, 0)
    rc = hip.L.capi_dgemtn_ts(hip.h, m, n, r, 1.0, dA.ptr, dA.ld, dB.ptr, dB.ld, 0.0, dC.ptr, dC.ld)
    assert rc != 0
    assert "r" in hip.L.capi_last_error(hip.h).decode().split("invalid argument:")[1].split()[0]
    hip.sync()
    assert np.all(dC.get()[0] == 3.5) and np.all(dC.get()[1] == SENTINEL)
    dR = Dev(np.full((m, r), 3.5), 0, 0)
    norms = torch.full((r,), SENTINEL, dtype=torch.float64, device="cuda")
    rc = hip.L.capi_dresid_ts(hip.h, m, n, r, dA.ptr, dA.ld, dX.ptr, dX.ld, dB.ptr, dB.ld, dR.ptr, dR.ld, C.c_void_p(norms.data_ptr()))
    assert rc != 0 and "r:" in hip.L.capi_last_error(hip.h).decode()
    hip.sync()
    assert np.all(dR.get()[0] == 3.5) and np.all(norms.cpu().numpy() == SENTINEL)


@pytest.mark.parametrize("m", [0, 777])
def test_beta_zero_does_not_read_c(hip, m):
    """BLAS rule: beta == 0 overwrites C, NaN in it does not propagate (m == 0: C <- 0)"""
    n, r = 130, 5
    A, B, _ = _inputs(m, n, r, seed=m)
    dA, dB, dC = Dev(A, 0, 0), Dev(B, 0, 0), Dev(np.full((n, r), np.nan), 2, 1)
    _gemtn(hip, dA, dB, dC, 1.0, 0.0)
    got, guard = dC.get()
    assert np.all(np.isfinite(got)) and np.all(guard == SENTINEL)
    if m == 0:
        assert np.all(got == 0.0)
