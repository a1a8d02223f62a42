"""CPU: capi_dormqr and capi_dgels exist where a caller binds them -- the header declares them with the sentence that names the reference interface,
the library exports them, the Python binding has the header's argument counts, the new source is in the Makefile's SRCS, the calls refuse a null
handle before they touch a device, and capital_amd.hqr.Hqr has its methods."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("capi_dormqr", "capi_dgels")
SENTENCE = "Not in the reference: lapack/interface.h declares _geqrf and _orgqr only"


def _header():
    return open(os.path.join(ROOT, "include", "capital_hip.h")).read()


def test_header_declares_both_calls_with_the_reference_sentence():
    from capital_amd import capi
    txt = _header()
    for name in NAMES:
        assert name in capi.declared_symbols()
        # the comment that ends at the declaration
        comment = re.search(r"/\* %s:(.*?)\*/\s*int %s\(" % (name, name), txt, re.S)
        assert comment, name
        assert SENTENCE in re.sub(r"\s*\n \*\s*", " ", comment.group(1)), name
    assert "CAPI_RIGHT" in re.search(r"/\* capi_dormqr:(.*?)\*/", txt, re.S).group(1)


def test_library_exports_and_binding_matches_the_header():
    from capital_amd import capi
    L = capi.load()
    txt = _header()
    for name in NAMES:
        assert hasattr(L, name)
        assert name in capi._SIGS
        decl = re.search(r"int %s\((.*?)\);" % name, txt, re.S).group(1)
        assert len(decl.split(",")) == 1 + len(capi._SIGS[name]), name
    assert len(capi._SIGS["capi_dormqr"]) == 10 and len(capi._SIGS["capi_dgels"]) == 10


def test_source_is_built():
    mk = open(os.path.join(ROOT, "capital_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "qr_apply_f64.hip" in srcs
    assert "ormqr_plan.h" in mk
    assert os.path.exists(os.path.join(ROOT, "capital_amd", "csrc", "qr_apply_f64.hip"))
    assert os.path.exists(os.path.join(ROOT, "capital_amd", "csrc", "ormqr_plan.h"))


def test_null_handle_is_refused_without_a_gpu():
    from capital_amd import capi
    L = capi.load()
    assert L.capi_dormqr(None, capi.LEFT, capi.TRANS, 4, 1, 2, None, 4, None, None, 4) == -1
    info = C.c_int(-99)
    assert L.capi_dgels(None, 4, 2, 1, None, 4, None, None, 4, None, C.byref(info)) == -1
    assert info.value == -99


def test_engine_header_has_the_slots():
    txt = open(os.path.join(ROOT, "capital_amd", "src", "lapack", "engine.h")).read()
    for what in ("class ArgPack_ormqr", "class ArgPack_gels", "inline void engine::_ormqr(", "inline int engine::_gels("):
        assert what in txt, what


def test_hqr_has_its_methods():
    from capital_amd import hqr
    for name in ("factor", "R", "apply_qt", "apply_q", "lstsq", "close"):
        assert callable(getattr(hqr.Hqr, name)), name
