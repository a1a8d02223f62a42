"""CPU: the entry points of the condition estimate and the error bounds exist where a caller binds them -- the driver library exports the two
calls, the header declares the C-ABI pieces (and the library exports them: test_capi_exports.py checks that for every declared name), and the
size of the estimator's state is pure host arithmetic that needs no GPU."""
import ctypes as C


def test_driver_exports_rcond_and_solve_expert():
    from capital_amd import driver
    D = driver.load()
    for sym in ("capital_cholinv_rcond", "capital_cholinv_solve_expert", "capital_cholinv_error_bounds"):
        assert hasattr(D, sym), sym
    assert hasattr(driver.Cholinv, "rcond") and hasattr(driver.Cholinv, "solve_expert")


def test_header_declares_the_new_calls():
    from capital_amd import capi
    declared = set(capi.declared_symbols())
    new = {"capi_dsym_abs", "capi_dberr", "capi_dlacn_block", "capi_dlacn_state_bytes", "capi_dcolamax"}
    assert new <= declared, sorted(new - declared)
    L = capi.load()
    assert all(hasattr(L, s) for s in new)
    assert {"capi_dsym_abs", "capi_dberr", "capi_dlacn_block", "capi_dcolamax"} <= set(capi._SIGS)


def test_state_size_without_a_gpu():
    from capital_amd import capi
    L = capi.load()
    assert L.capi_dlacn_state_bytes.restype is C.c_size_t
    nbytes = L.capi_dlacn_state_bytes(1000, 32)
    assert nbytes > 0 and nbytes >= 8 * 32 * 1000               # per column the n signs of dlacn2's ISGN at least
    assert L.capi_dlacn_state_bytes(1000, 1) < nbytes
    # out of range: no size
    assert L.capi_dlacn_state_bytes(1000, 33) == 0 and L.capi_dlacn_state_bytes(1000, 0) == 0 and L.capi_dlacn_state_bytes(0, 4) == 0
