"""CPU: the entry points that run one SUMMA multiply exist where a caller binds them -- the driver library exports capital_summa_gemm, _trmm and
_syrk, the Python binding has their signatures and the three wrappers, the case table of the grid tests names every form -- and the calls refuse
bad arguments and a missing world communicator before they touch a device."""
import ctypes as C
import os
import re

import numpy as np

import _summa_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"capital_summa_gemm": 17, "capital_summa_trmm": 17, "capital_summa_syrk": 15}


def test_driver_exports_the_three_multiplies():
    from capital_amd import driver
    D = driver.load()
    src = open(os.path.join(ROOT, "capital_amd", "drivers", "capital_driver.cpp")).read()
    for name, nargs in ENTRIES.items():
        assert hasattr(D, name) and len(getattr(D, name).argtypes) == nargs, name
        decl = re.search(r"^int %s\((.*?)\) \{" % name, src, re.S | re.M).group(1)
        assert len(decl.split(",")) == nargs, name                   # the binding's argument count is the definition's
    for wrapper in ("summa_gemm", "summa_trmm", "summa_syrk"):
        assert callable(getattr(driver, wrapper))


def test_calls_refuse_bad_arguments_without_a_gpu():
    from capital_amd import driver
    D = driver.load()
    a = np.zeros((3, 3), order="F")
    p = a.ctypes.data_as(C.POINTER(C.c_double))
    # a non-positive extent, a negative pad, a missing block
    assert D.capital_summa_gemm(1, 0, 0, 0, 0, 0, 3, 3, 1.0, 0.0, p, p, p, 0, 0.0, None, None) == -1
    assert D.capital_summa_trmm(1, 0, 0, 0, 1, 0, 0, 3, 3, 1.0, p, p, p, -1, 0.0, None, None) == -1
    assert D.capital_summa_syrk(1, 0, 0, 1, 1, 3, 3, 1.0, 0.0, None, p, 0, 0.0, None, None) == -1
    assert b"expected" in D.capital_drv_last_error()
    # no world communicator: capital_drv_init has not run in this process
    assert not driver._state["init"]
    assert D.capital_summa_gemm(1, 0, 0, 0, 0, 3, 3, 3, 1.0, 0.0, p, p, p, 0, 0.0, None, None) == -1
    assert b"capital_drv_init" in D.capital_drv_last_error()
    try:
        driver.summa_trmm(a, np.zeros((4, 3)), side="L")
    except driver.DriverError as e:
        assert "order 4" in str(e)
    else:
        raise AssertionError("a T of the wrong order was accepted")


def test_case_table_names_every_form():
    wide = {k: v for k, v in SC.FORMS.items() if not k.endswith("_narrow")}
    gemm = [(f["ta"], f["tb"], f["beta"], f["nan"]) for f in wide.values() if f["op"] == "gemm"]
    assert sorted(g[:2] for g in gemm if not g[3]) == [(0, 0), (0, 1), (1, 0), (1, 1)] and sorted(g[:2] for g in gemm if g[3]) == [(0, 0), (1, 0)]
    assert all(g[2] == (0.0 if g[3] else -0.5) for g in gemm)
    trmm = [(f["side"], f["uplo"], f["tr"], f["unit"]) for f in wide.values() if f["op"] == "trmm"]
    assert sorted(t[:3] for t in trmm if not t[3]) == sorted((s, u, t) for s in "LR" for u in "UL" for t in (0, 1))
    assert sorted(t[:3] for t in trmm if t[3]) == [("L", "L", 1), ("L", "U", 0), ("R", "L", 0), ("R", "U", 0)]
    syrk = [(f["uplo"], f["tr"], f["alpha"], f["beta"]) for f in wide.values() if f["op"] == "syrk"]
    assert sorted(s for s in syrk if s[3] == 1.0) == sorted((u, t, -1.0, 1.0) for u in "UL" for t in (0, 1))
    assert sorted(s for s in syrk if s[3] == 0.0) == [("L", 0, 0.75, 0.0), ("U", 1, 0.75, 0.0)]
    # every form: chunked and not, public and view mode, under each of the five environments
    tags = {c["tag"] for c in SC.cases()}
    assert len(tags) == len(SC.cases())
    for name in wide:
        for ename, _ in SC.ENVS:
            for chunks in (0, SC.CHUNKS):
                for pad in (0, SC.PAD):
                    assert f"{name}-ch{chunks}-p{pad}-{ename}" in tags
    # the chunk plans the table counts on (summa.h: struct chunks): 101 columns in three ragged chunks, 10 columns in 4, 4, 2 and an empty one
    def plan(N, nch):
        per = ((N + nch - 1) // nch + 1) & ~1
        return [min(N, per * j + per) - min(N, per * j) for j in range(nch)]
    assert plan(101, SC.CHUNKS) == [34, 34, 33] and plan(SC.NARROW, SC.NARROW_CHUNKS) == [4, 4, 2, 0]
