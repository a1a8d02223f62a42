"""lapack::engine::_geqp3 and _gelsy (capital_amd/src/lapack/engine.h) called by a compiled C++ program (tests/gelsy_engine/gelsy_engine.cpp) with
ArgPack_* objects, at 700 x 48 with rank 30, r = 5, rcond = 1e-13.  Its dump against tests/_qrcp_ref.py, the numpy restatement, on the A the program
itself formed: the rank and jpvt equal, the image, tau, X (both solution modes) and the squared residual norms to 1e-12.  Every comparison prints
err/tol before it asserts."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _qrcp_ref as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "gelsy_engine")
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


def test_geqp3_and_gelsy_through_the_engine(tmp_path):
    subprocess.check_call(["make", "-C", DIR, "-s"])
    out = str(tmp_path / "gelsy_engine.bin")
    res = subprocess.run([os.path.join(DIR, "gelsy_engine"), out], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "gelsy_engine ok" in res.stdout, res.stdout + res.stderr
    d = _read(out)
    m, n, rank, r, rcond = 700, 48, 30, 5, 1e-13
    F = lambda a, rows, cols: a.reshape((rows, cols), order="F")                                                  # noqa: E731
    A, B = F(d["A"], m, n), F(d["B"], m, r)
    # _geqp3 on the triangle the program fed it
    W = F(d["geqp3_in"], n, n)
    assert np.all(np.tril(W, -1) == 0.0)
    image, tau, jpvt, k, _ = ref.check_case(W, rcond, rank)
    assert d["geqp3_rank"][0] == k == rank
    jg = d["geqp3_jpvt"].astype(np.int64)
    assert np.array_equal(jg, jpvt)
    _check("_geqp3 image", F(d["geqp3_F"], n, n), image)
    _check("_geqp3 tau", d["geqp3_tau"], tau)
    # _gelsy, both modes
    for mode, mn in (("mn", True), ("basic", False)):
        X, kk, jr, _, _ = ref.gelsy(A, B, rcond, mn)
        assert d[f"gelsy_{mode}_rank"][0] == kk == rank
        assert np.array_equal(d[f"gelsy_{mode}_jpvt"].astype(np.int64)[:rank], jr[:rank])
        got = F(d[f"gelsy_{mode}_B"], m, r)[:n]
        _check(f"_gelsy {mode} X", got, X)
        _check(f"_gelsy {mode} squared residual norms", d[f"gelsy_{mode}_norm2"], np.linalg.norm(B - A @ X, axis=0) ** 2)
        if not mn:
            assert np.all(got[jr[rank:]] == 0.0)
