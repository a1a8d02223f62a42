"""CPU: the entry points of the factor update exist where a caller binds them -- the header declares capi_dchud, capi_dchud_inv and capi_dchud_log_bytes
and the library exports them, the Python binding has their signatures, the driver library exports capital_cholinv_update and driver.Cholinv has the
method, the host layer binds the calls weakly -- and the calls refuse bad arguments before they touch a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("capi_dchud", "capi_dchud_inv", "capi_dchud_log_bytes")


def test_header_declares_and_library_exports_the_three_calls():
    from capital_amd import capi
    L = capi.load()
    txt = open(os.path.join(ROOT, "include", "capital_hip.h")).read()
    assert "Not in the reference: cholinv.hpp stops at R and R^-1" in txt
    for name in NAMES:
        assert name in capi.declared_symbols()
        assert hasattr(L, name)
    for name in NAMES[:2]:
        assert name in capi._SIGS
        # the binding's argument count is the header's (the handle comes first there)
        decl = re.search(r"int %s\((.*?)\);" % name, txt, re.S).group(1)
        assert len(decl.split(",")) == 1 + len(capi._SIGS[name]), name
    assert len(capi._SIGS["capi_dchud"]) == 10 and len(capi._SIGS["capi_dchud_inv"]) == 9
    decl = re.search(r"size_t capi_dchud_log_bytes\((.*?)\);", txt, re.S).group(1)
    assert len(decl.split(",")) == len(L.capi_dchud_log_bytes.argtypes) == 2 and L.capi_dchud_log_bytes.restype is C.c_size_t


def test_driver_exports_the_update():
    from capital_amd import driver
    D = driver.load()
    assert hasattr(D, "capital_cholinv_update") and len(D.capital_cholinv_update.argtypes) == 4
    assert hasattr(driver.Cholinv, "update")


def test_host_layer_binds_the_calls_weakly():
    """a stand-in of the C-ABI without the calls must still link: they are weak references of the host layer, as capi_dtrsm_thin is"""
    txt = open(os.path.join(ROOT, "capital_amd", "src", "alg", "cholesky", "cholinv", "cholinv.h")).read()
    for name in NAMES:
        assert re.search(r"^#pragma weak %s$" % name, txt, re.M), name


def test_null_handle_is_refused_without_a_gpu():
    from capital_amd import capi
    L = capi.load()
    info = C.c_int(-99)
    assert L.capi_dchud(None, 1, 4, 1, None, 4, 0, None, 4, None, C.byref(info)) == -1
    assert info.value == -99
    assert L.capi_dchud_inv(None, 1, 4, 1, None, 4, 0, None, 0, 4) == -1


def test_log_bytes():
    from capital_amd import capi
    L = capi.load()
    for n, r in ((-1, 1), (1 << 31, 1), (10, 0), (10, 33), (10, -2)):
        assert L.capi_dchud_log_bytes(n, r) == 0, (n, r)
    # per step x_k (r doubles), alpha_k and beta_k
    assert L.capi_dchud_log_bytes(1000, 17) == 8 * 1000 * 19
    assert L.capi_dchud_log_bytes(0, 5) == 0
