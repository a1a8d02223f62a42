"""CPU: capi_dgeqp3 and capi_dgelsy exist where a caller binds them -- the header declares them with the sentence that names the reference interface and
states the step rule, the library exports them, the Python binding has the header's argument counts, the new source is in the Makefile's SRCS,
lapack/engine.h has the slots, capital_amd.hqr.Hqr has the methods, and the calls refuse a null handle before they touch a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("capi_dgeqp3", "capi_dgelsy")
SENTENCE = "Not in the reference: lapack/interface.h declares _geqrf and _orgqr only"


def _header():
    return open(os.path.join(ROOT, "include", "capital_hip.h")).read()


def _comment(txt, name):
    c = re.search(r"/\* %s:(.*?)\*/" % name, txt, re.S)
    assert c, name
    return re.sub(r"\s*\n \*\s*", " ", c.group(1))


def test_header_declares_both_calls_and_states_the_rule():
    from capital_amd import capi
    txt = _header()
    for name in NAMES:
        assert name in capi.declared_symbols()
        assert SENTENCE in _comment(txt, name), name
    rule = _comment(txt, "capi_dgeqp3")
    for words in ("FIRST index", "a NaN is entered as -inf", "nu > rtol * nu_0 && nu > 0", "tol3z = sqrt(2^-53)", "tau = 0, beta = alpha",
                  "max(mr, n) 2^-52", "incremental condition estimator"):
        assert words in rule, words
    assert int(re.search(r"CAPI_GEQP3_MAX = (\d+)", txt).group(1)) == 2048
    seq = _comment(txt, "capi_dgelsy")
    assert "FURTHER RIGHT-HAND SIDES" in seq and "capi_drow_scatter" in seq
    assert "capi_dgelsy" in _comment(txt, "capi_dgels")                     # the pointer for rank-deficient problems


def test_library_exports_and_binding_matches_the_header():
    from capital_amd import capi
    L = capi.load()
    txt = _header()
    for name in NAMES:
        assert hasattr(L, name)
        assert name in capi._SIGS
        decl = re.search(r"^int %s\((.*?)\);" % name, txt, re.S | re.M).group(1)
        assert len(decl.split(",")) == 1 + len(capi._SIGS[name]), name
    assert len(capi._SIGS["capi_dgeqp3"]) == 8 and len(capi._SIGS["capi_dgelsy"]) == 19


def test_source_is_built():
    mk = open(os.path.join(ROOT, "capital_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "qrcp_f64.hip" in srcs
    assert os.path.exists(os.path.join(ROOT, "capital_amd", "csrc", "qrcp_f64.hip"))


def test_null_handle_is_refused_without_a_gpu():
    from capital_amd import capi
    L = capi.load()
    k = C.c_int(-99)
    assert L.capi_dgeqp3(None, 4, 4, None, 4, None, None, 0.0, C.byref(k)) == -1
    assert k.value == -99
    assert L.capi_dgelsy(None, 8, 4, 1, None, 8, None, None, 4, None, None, None, 4, None, None, 8, -1.0, 1, None, C.byref(k)) == -1
    assert k.value == -99


def test_engine_header_has_the_slots():
    txt = open(os.path.join(ROOT, "capital_amd", "src", "lapack", "engine.h")).read()
    for what in ("AlapackGeqp3 = 0x14", "AlapackGelsy = 0x15", "class ArgPack_geqp3", "class ArgPack_gelsy", "ArgPack_gelsy(Order o, bool mn)",
                 "inline int engine::_geqp3(", "inline int engine::_gelsy("):
        assert what in txt, what


def test_hqr_has_the_new_methods():
    from capital_amd import hqr
    for name in ("factor_pivoted", "lstsq_pivoted"):
        assert callable(getattr(hqr.Hqr, name)), name
