"""CPU: the entry points of the low-rank solve exist where a caller binds them -- the header declares capi_dlr_diag, capi_drow_pow and capi_ddiag_add
and the library exports them, the Python binding has their signatures, the driver library exports capital_cholinv_lowrank_prepare / _solve /
_quadratic_forms and driver.Cholinv has the four methods, the host layer binds the calls weakly -- and the calls refuse a null handle before they touch a
device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"capi_dlr_diag": 6, "capi_drow_pow": 11, "capi_ddiag_add": 4}       # arguments after the handle


def test_header_declares_and_library_exports_the_calls():
    from capital_amd import capi
    L = capi.load()
    txt = open(os.path.join(ROOT, "include", "capital_hip.h")).read()
    for name, count in NAMES.items():
        assert name in capi.declared_symbols()
        assert hasattr(L, name)
        assert name in capi._SIGS and len(capi._SIGS[name]) == count
        # the binding's argument count is the header's (the handle comes first there)
        decl = re.search(r"int %s\((.*?)\);" % name, txt, re.S).group(1)
        assert len(decl.split(",")) == 1 + count, name
        # .. and its comment says where the call stands beside the reference
        comment = txt[:txt.index("int %s(" % name)].rsplit("*/", 2)[-2]
        assert name + ":" in comment and "Not in the reference: cholinv.hpp stops at R and R^-1" in comment, name


def test_driver_exports_the_three_operations():
    from capital_amd import driver
    D = driver.load()
    for name, count in (("capital_cholinv_lowrank_prepare", 6), ("capital_cholinv_lowrank_solve", 5), ("capital_cholinv_lowrank_quadratic_forms", 4)):
        assert hasattr(D, name) and len(getattr(D, name).argtypes) == count, name
    for method in ("lowrank_prepare", "lowrank_solve", "lowrank_quadratic_forms", "lowrank_logdet"):
        assert hasattr(driver.Cholinv, method) and getattr(driver.Cholinv, method).__doc__, method


def test_host_layer_binds_the_calls_weakly():
    """a stand-in of the C-ABI without the calls must still link: they are weak references of the host layer, as capi_dpchol is"""
    txt = open(os.path.join(ROOT, "capital_amd", "src", "alg", "cholesky", "cholinv", "cholinv.h")).read()
    for name in NAMES:
        assert re.search(r"^#pragma weak %s$" % name, txt, re.M), name
    for op in ("lowrank_prepare", "lowrank_solve", "lowrank_quadratic_forms"):
        assert re.search(r"static void %s\(" % op, txt), op
    assert "no solve on the low-rank factor" in txt


def test_null_handle_is_refused_without_a_gpu():
    from capital_amd import capi
    L = capi.load()
    d = (C.c_double * 4)(-99.0, -99.0, -99.0, -99.0)
    rec = (C.c_double * 4)(-99.0, -99.0, -99.0, -99.0)
    assert L.capi_dlr_diag(None, 4, 1.0, None, None, C.addressof(d), C.addressof(rec)) == -1
    assert L.capi_drow_pow(None, 2, 2, -1.0, C.addressof(rec), 1.0, C.addressof(d), 2, 0.0, C.addressof(d), 2, None) == -1
    assert L.capi_ddiag_add(None, 2, 1.0, C.addressof(d), 2) == -1
    assert list(d) == [-99.0] * 4 and list(rec) == [-99.0] * 4
