"""lapack::engine::_ormqr and _gels (capital_amd/src/lapack/engine.h) called by a compiled C++ program (tests/ormqr_engine/ormqr_engine.cpp) with
ArgPack_* objects, at m = 700, n = 48, r = 5 after _geqrf.  Its dump against tests/_ormqr_ref.py on the oracle's dgeqrf image and numpy's Householder
solve (tests/_lstsq_cases.solve_householder), 1e-12.  Every comparison prints err/tol before it asserts."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _lstsq_cases as lc
import _ormqr_ref as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "ormqr_engine")
TOL = 1e-12


def _read(path):
    out = {}
    with open(path, "rb") as f:
        while True:
            tag = f.read(32)
            if not tag:
                break
            (count,) = struct.unpack("<q", f.read(8))
            out[tag.split(b"\0")[0].decode()] = np.frombuffer(f.read(8 * count), dtype=np.float64).copy()
    return out


def _check(what, got, want):
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{what}: err/tol {err:.3e}/{TOL:.1e} = {err / TOL:.3f}")
    assert err <= TOL, (what, err)


def test_ormqr_and_gels_through_the_engine(oracle, tmp_path):
    subprocess.check_call(["make", "-C", DIR, "-s"])
    out = str(tmp_path / "ormqr_engine.bin")
    res = subprocess.run([os.path.join(DIR, "ormqr_engine"), out], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "ormqr_engine ok" in res.stdout, res.stdout + res.stderr
    d = _read(out)
    m, n, r = 700, 48, 5
    rnd = lambda rows, cols, key: np.asfortranarray(oracle.distribute_random(cols, rows, 0, 0, 1, 1, key=key))   # noqa: E731
    F = lambda a, rows, cols: a.reshape((rows, cols), order="F")                                                  # noqa: E731
    A, C, B = rnd(m, n, 9), rnd(m, r, 11), rnd(m, r, 12)
    fac, tau = ref.image(A)
    _check("_geqrf image", F(d["geqrf_A"], m, n), fac)
    _check("_geqrf tau", d["geqrf_tau"], tau)
    _check("_ormqr Trans", F(d["ormqr_qt"], m, r), ref.ormqr(fac, tau, C, True))
    _check("_ormqr NoTrans", F(d["ormqr_q"], m, r), ref.ormqr(fac, tau, C, False))
    assert np.array_equal(d["ormqr_q_after_refusal"], d["ormqr_q"])
    assert d["gels_info"][0] == 0.0
    assert np.array_equal(d["gels_A"], d["geqrf_A"]) and np.array_equal(d["gels_tau"], d["geqrf_tau"])
    X = F(d["gels_B"], m, r)[:n]
    want = lc.solve_householder(A, B)
    _check("_gels X", X, want)
    _check("_gels tail", F(d["gels_B"], m, r)[n:], ref.ormqr(fac, tau, B, True)[n:])
    res2 = np.linalg.norm(B - A @ want, axis=0) ** 2
    _check("_gels squared residual norms", d["gels_norm2"], res2)
