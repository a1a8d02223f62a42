"""CPU: the entry points of the pivoted partial Cholesky exist where a caller binds them -- the header declares capi_dpchol and the library exports it,
the Python binding has its signature, the driver library exports capital_cholinv_factor_pivoted / capital_cholinv_get_pivoted and driver.Cholinv has
the methods, the host layer binds the call weakly -- and the call refuses bad arguments before it touches a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("capi_dpchol", "capi_dpchol_thresh")


def test_header_declares_and_library_exports_the_calls():
    from capital_amd import capi
    L = capi.load()
    txt = open(os.path.join(ROOT, "include", "capital_hip.h")).read()
    assert "Not in the reference: cholinv.hpp stops at R and R^-1" in txt
    for name in NAMES:
        assert name in capi.declared_symbols()
        assert hasattr(L, name)
        assert name in capi._SIGS
        # the binding's argument count is the header's (the handle comes first there)
        decl = re.search(r"int %s\((.*?)\);" % name, txt, re.S).group(1)
        assert len(decl.split(",")) == 1 + len(capi._SIGS[name]), name
    assert len(capi._SIGS["capi_dpchol"]) == 11 and len(capi._SIGS["capi_dpchol_thresh"]) == 5
    cap = int(re.search(r"CAPI_PCHOL_MAX_RANK = (\d+)", txt).group(1))
    assert cap >= 4096


def test_driver_exports_the_pivoted_factorization():
    from capital_amd import driver
    D = driver.load()
    assert hasattr(D, "capital_cholinv_factor_pivoted") and len(D.capital_cholinv_factor_pivoted.argtypes) == 6
    assert hasattr(D, "capital_cholinv_get_pivoted") and len(D.capital_cholinv_get_pivoted.argtypes) == 4
    for method in ("factor_pivoted", "L_pivoted", "piv", "schur_diagonal"):
        assert hasattr(driver.Cholinv, method), method


def test_host_layer_binds_the_calls_weakly():
    """a stand-in of the C-ABI without the calls must still link: they are weak references of the host layer, as capi_dchud is"""
    txt = open(os.path.join(ROOT, "capital_amd", "src", "alg", "cholesky", "cholinv", "cholinv.h")).read()
    for name in NAMES:
        assert re.search(r"^#pragma weak %s$" % name, txt, re.M), name


def test_null_handle_is_refused_without_a_gpu():
    from capital_amd import capi
    L = capi.load()
    rank, trace, thresh = C.c_int(-99), C.c_double(-99.0), C.c_double(-99.0)
    assert L.capi_dpchol(None, 4, None, 4, -1.0, 4, None, 4, None, None, C.byref(rank), C.byref(trace)) == -1
    assert rank.value == -99 and trace.value == -99.0
    assert L.capi_dpchol_thresh(None, 4, None, 4, -1.0, C.byref(thresh)) == -1
    assert thresh.value == -99.0
