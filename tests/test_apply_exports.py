"""CPU: the entry points of the operations on the factors themselves exist where a caller binds them -- the header declares capi_dtri_rownorm2,
capi_dtri_logdiag and capi_dcolnorm2 and the library exports them, the Python binding has their signatures, the driver library exports the four
capital_cholinv_* calls and driver.Cholinv has the methods, the host layer binds the calls weakly -- and the calls refuse a null handle before they
touch a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("capi_dtri_rownorm2", "capi_dtri_logdiag", "capi_dcolnorm2")
ENTRIES = {"capital_cholinv_apply": 5, "capital_cholinv_quadratic_forms": 4, "capital_cholinv_logdet": 2, "capital_cholinv_inverse_diagonal": 2}


def test_header_declares_and_library_exports_the_three_calls():
    from capital_amd import capi
    L = capi.load()
    txt = open(os.path.join(ROOT, "include", "capital_hip.h")).read()
    for name in NAMES:
        assert name in capi.declared_symbols()
        assert hasattr(L, name)
        assert name in capi._SIGS
        # each call's own comment says where the reference stops
        comment = re.sub(r"\s*\n \*\s*", " ", txt[:txt.index("int %s(" % name)].rsplit("/*", 1)[1])      # (the header wraps its lines)
        assert "Not in the reference: cholinv.hpp stops at R and R^-1" in comment, name
        # the binding's argument count is the header's (the handle comes first there)
        decl = re.search(r"int %s\((.*?)\);" % name, txt, re.S).group(1)
        assert len(decl.split(",")) == 1 + len(capi._SIGS[name]), name
    assert len(capi._SIGS["capi_dtri_rownorm2"]) == 8 and len(capi._SIGS["capi_dtri_logdiag"]) == 5 and len(capi._SIGS["capi_dcolnorm2"]) == 5


def test_driver_exports_the_four_operations():
    from capital_amd import driver
    D = driver.load()
    for name, nargs in ENTRIES.items():
        assert hasattr(D, name) and len(getattr(D, name).argtypes) == nargs, name
    for method in ("apply", "quadratic_forms", "logdet", "inverse_diagonal"):
        assert callable(getattr(driver.Cholinv, method))


def test_host_layer_binds_the_calls_weakly():
    """a stand-in of the C-ABI without the calls must still link: they are weak references of the host layer, as capi_dtrsm_thin is"""
    txt = open(os.path.join(ROOT, "capital_amd", "src", "alg", "cholesky", "cholinv", "cholinv.h")).read()
    for name in NAMES:
        assert re.search(r"^#pragma weak %s$" % name, txt, re.M), name


def test_new_source_is_built_into_the_library():
    mk = open(os.path.join(ROOT, "capital_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "tri_reduce_f64.hip" in srcs and "bounds_f64.hip" in srcs


def test_null_handle_is_refused_without_a_gpu():
    from capital_amd import capi
    L = capi.load()
    assert L.capi_dtri_rownorm2(None, capi.UPPERTRI, 4, 4, None, 4, 0, 0.0, None) == -1
    assert L.capi_dtri_logdiag(None, 4, None, 4, 0, None) == -1
    assert L.capi_dcolnorm2(None, 4, 1, None, 4, None) == -1
