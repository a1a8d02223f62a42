"""CPU: the entry points of the column-pivoted CholeskyQR exist where a caller binds them -- the header declares capi_dpstrf and capi_drow_scatter and
the library exports them, the Python binding has their signatures, the driver library exports capital_cacqr_factor_pivoted / capital_cacqr_get_piv and
driver.Cacqr has the methods -- and the calls refuse bad arguments before they touch a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("capi_dpstrf", "capi_drow_scatter")


def test_header_declares_and_library_exports_both_calls():
    from capital_amd import capi
    L = capi.load()
    txt = open(os.path.join(ROOT, "include", "capital_hip.h")).read()
    assert "Not in the reference: cacqr.hpp stops at Q and R" in txt
    for name in NAMES:
        assert name in capi.declared_symbols()
        assert hasattr(L, name)
        assert name in capi._SIGS
        # the binding's argument count is the header's (the handle comes first there)
        decl = re.search(r"int %s\((.*?)\);" % name, txt, re.S).group(1)
        assert len(decl.split(",")) == 1 + len(capi._SIGS[name]), name
    assert len(capi._SIGS["capi_dpstrf"]) == 6 and len(capi._SIGS["capi_drow_scatter"]) == 9


def test_driver_exports_the_pivoted_calls():
    from capital_amd import driver
    D = driver.load()
    assert hasattr(D, "capital_cacqr_factor_pivoted") and hasattr(D, "capital_cacqr_get_piv")
    assert len(D.capital_cacqr_factor_pivoted.argtypes) == 4 and len(D.capital_cacqr_get_piv.argtypes) == 2
    for name in ("factor_pivoted", "R_pivoted", "Q_pivoted"):
        assert hasattr(driver.Cacqr, name)


def test_host_layer_binds_the_calls_weakly():
    """a stand-in of the C-ABI without the two calls must still link: they are weak references of the host layer, as capi_dgesvj is"""
    txt = open(os.path.join(ROOT, "capital_amd", "src", "alg", "qr", "cacqr", "cacqr.h")).read()
    for name in NAMES:
        assert re.search(r"^#pragma weak %s$" % name, txt, re.M), name


def test_null_handle_is_refused_without_a_gpu():
    from capital_amd import capi
    L = capi.load()
    rank = C.c_int(-99)
    assert L.capi_dpstrf(None, 4, None, 4, 0.0, None, C.byref(rank)) == -1
    assert rank.value == -99
    assert L.capi_drow_scatter(None, 0, 1, 1, 1, None, 1, None, None, 1) == -1
