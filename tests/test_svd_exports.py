"""CPU: the entry points of the tall-skinny SVD exist where a caller binds them -- the header declares capi_dgesvj and the library exports it, the
Python binding has its signature, the driver library exports capital_cacqr_svd and driver.Cacqr has svd -- and the call refuses bad arguments
before it touches a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_dgesvj():
    from capital_amd import capi
    assert "capi_dgesvj" in capi.declared_symbols()
    L = capi.load()
    assert hasattr(L, "capi_dgesvj")
    assert "capi_dgesvj" in capi._SIGS and len(capi._SIGS["capi_dgesvj"]) == 9
    txt = open(os.path.join(ROOT, "include", "capital_hip.h")).read()
    assert "Not in the reference: cacqr.hpp stops at Q and R" in txt
    # the binding's argument count is the header's (the handle comes first there)
    decl = re.search(r"int capi_dgesvj\((.*?)\);", txt, re.S).group(1)
    assert len(decl.split(",")) == 1 + len(capi._SIGS["capi_dgesvj"])


def test_driver_exports_svd():
    from capital_amd import driver
    D = driver.load()
    assert hasattr(D, "capital_cacqr_svd")
    assert hasattr(driver.Cacqr, "svd")
    assert D.capital_cacqr_svd.argtypes is not None and len(D.capital_cacqr_svd.argtypes) == 6


def test_null_handle_is_refused_without_a_gpu():
    from capital_amd import capi
    L = capi.load()
    sweeps = C.c_int(-99)
    assert L.capi_dgesvj(None, 4, None, 4, None, 4, None, None, 4, C.byref(sweeps)) == -1
    assert sweeps.value == -99
