"""CPU: the numpy restatement of the low-rank solve (tests/_lowrank_ref.py: the formulas of cholesky::cholinv::lowrank_prepare / lowrank_solve /
lowrank_quadratic_forms) against a Cholesky solve of the dense M = L L^T + D in longdouble, on every case of tests/_lowrank_cases.py.

The Woodbury form's error scale is ||C||_1 u, not kappa(C) u.  On a gated case (||C||_1 u <= 1e-7) X and q are within 4 ||C||_1 u of the reference and
log det M within 64 u S + 64 k ||C||_1 u; the uniform path C = I + G / sigma^2 agrees with the general one to the same bound.  The printed ratios are the
record (the worst of each stands in the docstring of tests/_lowrank_cases.py); a report-only case prints its errors and is only asked for finite results."""
import numpy as np
import pytest

import _lowrank_cases as lc
import _lowrank_ref as lref
from _lowrank_ref import U64


def test_the_gate_leaves_out_exactly_the_smallest_shift():
    for name, label in lc.CASES:
        assert lc.gated(name, label) == (label != "s1e-10"), (name, label, lc.restated(name, label)["cu"])


@pytest.mark.parametrize("name,label", lc.CASES, ids=["-".join(c) for c in lc.CASES])
def test_restatement_against_longdouble(name, label):
    L, _ = lc.factor(name)
    k = L.shape[1]
    rs = lc.restated(name, label)
    Xr, ldr, qr = lc.reference(name, label)
    cu, prep = rs["cu"], rs["prep"]
    ex = float(np.max(lc.restatement_errors(name, label)))
    eq = float(np.max(np.abs(rs["q"] - qr) / rs["b2"]))
    el = abs(prep["logdet"] - ldr)
    bl = 64 * U64 * prep["S"] + 64 * k * cu
    B = lc.rhs(L.shape[0])
    rr = float(np.max(lref.residual_norms(L, rs["d"], B, rs["X"]) / np.linalg.norm(B, axis=0)))
    print(f"lowrank restatement {name} {label}: k {k} |C|_1 u {cu:.2e}  X err {ex:.2e} = {ex / cu:.3f} |C|_1 u  q err {eq:.2e} = {eq / cu:.3f} |C|_1 u  "
          f"relres {rr:.2e} = {rr / cu:.3f} |C|_1 u  logdet err {el:.2e} = {el / bl:.2e} of its bound ({el / prep['S']:.2e} S)")
    assert np.all(np.isfinite(rs["X"])) and np.all(np.isfinite(rs["q"])) and np.isfinite(prep["logdet"])
    if not lc.gated(name, label):
        return
    assert ex <= 4 * cu
    assert eq <= 4 * cu
    assert el <= bl


@pytest.mark.parametrize("name", lc.NAMES)
@pytest.mark.parametrize("label", ["s1e-2", "s1e-6"])
def test_uniform_path_agrees_with_the_general_one(name, label):
    L, _ = lc.factor(name)
    rs = lc.restated(name, label)
    assert rs["uniform"]
    B = lc.rhs(L.shape[0])
    Xr, ldr, qr = lc.reference(name, label)
    gen = lref.prepare(L, rs["d"], uniform=False)
    Xg = lref.solve(L, rs["d"], gen["Rc"], B)
    eu, eg = float(np.max(lref.column_errors(rs["X"], Xr))), float(np.max(lref.column_errors(Xg, Xr)))
    qg, b2 = lref.quadratic_forms(L, rs["d"], gen["Rc"], B)
    print(f"lowrank uniform vs general {name} {label}: X err {eu:.2e} / {eg:.2e}, |C|_1 {rs['prep']['cnorm1']:.6e} / {gen['cnorm1']:.6e}")
    assert eu <= 4 * rs["cu"] and eg <= 4 * rs["cu"]
    assert float(np.max(np.abs(qg - qr) / b2)) <= 4 * rs["cu"]
    assert abs(gen["logdet"] - ldr) <= 64 * U64 * gen["S"] + 64 * L.shape[1] * rs["cu"]
    assert abs(gen["cnorm1"] - rs["prep"]["cnorm1"]) <= 1e-12 * gen["cnorm1"]


def test_two_by_two_against_the_dense_solve():
    L = np.array([[2.0, 0.0], [1.0, 0.5]])
    d = np.array([0.25, 3.0])
    B = np.array([[1.0, -2.0, 0.5], [4.0, 0.25, -1.0]])
    M = L @ L.T + np.diag(d)
    prep = lref.prepare(L, d)
    X = lref.solve(L, d, prep["Rc"], B)
    Xd = np.linalg.solve(M, B)
    assert np.max(np.abs(X - Xd)) <= 64 * U64 * prep["cnorm1"] * np.max(np.abs(Xd))
    q, _ = lref.quadratic_forms(L, d, prep["Rc"], B)
    assert np.max(np.abs(q - np.sum(B * Xd, axis=0))) <= 64 * U64 * prep["cnorm1"] * np.max(np.abs(q))
    assert abs(prep["logdet"] - np.linalg.slogdet(M)[1]) <= 64 * U64 * prep["S"]
    assert np.max(lref.residual_norms(L, d, B, X)) <= 64 * U64 * prep["cnorm1"] * np.max(lref.residual_scale(L, d, B, X))
    # d = (shift + diag) + schur, in that order
    assert lref.diag_vector(2, 0.1, np.array([0.2, 0.3]), np.array([0.3, 1e-17])).tolist() == [(0.1 + 0.2) + 0.3, (0.1 + 0.3) + 1e-17]
