"""CPU: the entry points of the power-of-two equilibration exist where a caller binds them -- the header declares capi_dpoequ2, capi_dsym_scale2 and
capi_drow_scale2 and the library exports them, the Python binding has their signatures, the driver library exports capital_cholinv_equilibrate and
capital_cholinv_unequilibrate and driver.Cholinv has the methods, the host layer binds the calls weakly, the Makefile builds the new source -- and
the calls refuse a null handle before they touch a device."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"capi_dpoequ2": 5, "capi_dsym_scale2": 5, "capi_drow_scale2": 9}            # arguments after the handle
ENTRIES = {"capital_cholinv_equilibrate": 6, "capital_cholinv_unequilibrate": 1}


def test_header_declares_and_library_exports_the_three_calls():
    from capital_amd import capi
    L = capi.load()
    txt = open(os.path.join(ROOT, "include", "capital_hip.h")).read()
    for name, nargs in NAMES.items():
        assert name in capi.declared_symbols()
        assert hasattr(L, name)
        assert name in capi._SIGS and len(capi._SIGS[name]) == nargs
        # each call's own comment says where the reference stops
        comment = re.sub(r"\s*\n \*\s*", " ", txt[:txt.index("int %s(" % name)].rsplit("/*", 1)[1])      # (the header wraps its lines)
        assert "Not in the reference: cholinv.hpp stops at R and R^-1" in comment, name
        # the binding's argument count is the header's (the handle comes first there)
        decl = re.search(r"int %s\((.*?)\);" % name, txt, re.S).group(1)
        assert len(decl.split(",")) == 1 + len(capi._SIGS[name]), name


def test_driver_exports_the_entries_and_methods():
    from capital_amd import driver
    D = driver.load()
    for name, nargs in ENTRIES.items():
        assert hasattr(D, name) and len(getattr(D, name).argtypes) == nargs, name
    for method in ("equilibrate", "scale", "unequilibrate"):
        assert callable(getattr(driver.Cholinv, method))


def test_host_layer_binds_the_calls_weakly():
    """a stand-in of the C-ABI without the calls must still link: they are weak references of the host layer, as capi_dtrsm_thin is"""
    txt = open(os.path.join(ROOT, "capital_amd", "src", "alg", "cholesky", "cholinv", "cholinv.h")).read()
    for name in NAMES:
        assert re.search(r"^#pragma weak %s$" % name, txt, re.M), name


def test_new_source_is_built_into_the_library():
    mk = open(os.path.join(ROOT, "capital_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "equil_f64.hip" in srcs
    assert os.path.exists(os.path.join(ROOT, "capital_amd", "csrc", "equil_f64.hip"))


def test_null_handle_is_refused_without_a_gpu():
    from capital_amd import capi
    L = capi.load()
    assert L.capi_dpoequ2(None, 4, None, 4, None, None) == -1
    assert L.capi_dsym_scale2(None, 4, None, 4, None, 1) == -1
    assert L.capi_drow_scale2(None, 4, 1, None, 1, None, 4, None, 4, None) == -1
