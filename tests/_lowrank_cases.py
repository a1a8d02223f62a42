"""The seeded cases of the low-rank solve tests (tests/_lowrank_ref.py is the restatement and the reference), each built once and read-only.

L, piv and the Schur diagonal are those of tests/_pchol_cases.restatement(name), so a device test feeds the same A through factor_pivoted():
  exact300 (k = 40), rbf700 (k = 166), rbf700cap33 (k = 33), pad33 (n = 33, k = 9), one (n = k = 1)
and d is one of, with abar = trace(A) / n:
  s1e-2, s1e-6, s1e-10   a uniform shift 1e-2, 1e-6, 1e-10 abar
  schur+1e-4             the remaining Schur diagonal + 1e-4 abar (FITC's diagonal)
  graded                 a user diagonal graded over 6 decades, abar logspace(0, -6, n), no shift
A case is GATED where ||C||_1 u <= 1e-7 -- every d but s1e-10 -- and REPORT-ONLY otherwise: finite results, the errors printed beside ||C||_1 u.  Every
listed case is one or the other; none is skipped.

Worst ratios of the restatement against the longdouble reference over the gated cases, r = 33 right-hand sides (tests/test_lowrank_host.py prints them):
  max_j ||x_j - x_ref,j|| / ||x_ref,j|| / (||C||_1 u)      1.99   (n = k = 1, s1e-6; at most 0.006 on the cases with n >= 33: 1e-15 .. 3e-12)
  max_j |q_j - q_ref,j| / (sum b^2 / d) / (||C||_1 u)       0.91   (n = k = 1, graded; at most 0.003 on the cases with n >= 33)
  max_j ||b_j - M x_j|| / ||b_j|| / (||C||_1 u)             5.7    (rbf700, graded; not gated)
  |logdet - ref| / (64 u S + 64 k ||C||_1 u)                1.5e-2 (n = k = 1, graded); |logdet - ref| <= 1.9e-15 S on every gated case
  uniform path C = I + G / sigma^2 against the general one  both within 4 ||C||_1 u of the reference; ||C||_1 equal to 1e-12
On the report-only cases (||C||_1 u = 1.1e-6 .. 4.8e-4) the same ratios are 2.34, 3e-5, 2.2 and 5e-7."""
import functools

import numpy as np

import _lowrank_ref as lref
import _pchol_cases as pc

NAMES = ("exact300", "rbf700", "rbf700cap33", "pad33", "one")
LABELS = ("s1e-2", "s1e-6", "s1e-10", "schur+1e-4", "graded")
CASES = tuple((name, label) for name in NAMES for label in LABELS)
GATE = 1e-7                  # on ||C||_1 u
RMAX = 33                    # right-hand sides of a case; the sets the tests use are its first 3 and all 33


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


def abar(name):
    A = pc.case(name)[0]
    return float(np.trace(A)) / A.shape[0]


def diag_args(name, label):
    """(shift, diag or None, schur flag): what lowrank_prepare() is called with"""
    A = pc.case(name)[0]
    n, a = A.shape[0], abar(name)
    if label.startswith("s1e-"):
        return float(label[1:]) * a, None, False
    if label == "schur+1e-4":
        return 1e-4 * a, None, True
    assert label == "graded"
    return 0.0, _frozen(a * np.logspace(0, -6, n)), False


@functools.lru_cache(maxsize=None)
def rhs(n):
    return _frozen(np.asfortranarray(np.random.default_rng(5 + n).standard_normal((n, RMAX))))


@functools.lru_cache(maxsize=None)
def factor(name):
    """(L n x k, schur diagonal) of the restatement of the pivoted partial Cholesky"""
    r = pc.restatement(name)
    return _frozen(r["L"][:, :r["rank"]]), r["d"]


@functools.lru_cache(maxsize=None)
def restated(name, label):
    """dict(d, uniform, prep, X, q, b2, cu): the restatement on the case and its 33 right-hand sides; cu = ||C||_1 u"""
    L, schur = factor(name)
    shift, diag, use_schur = diag_args(name, label)
    d = _frozen(lref.diag_vector(L.shape[0], shift, diag, schur if use_schur else None))
    uniform = diag is None and not use_schur
    prep = lref.prepare(L, d, uniform)
    B = rhs(L.shape[0])
    q, b2 = lref.quadratic_forms(L, d, prep["Rc"], B)
    return {"d": d, "uniform": uniform, "prep": prep, "X": _frozen(lref.solve(L, d, prep["Rc"], B)), "q": _frozen(q), "b2": _frozen(b2),
            "cu": prep["cnorm1"] * lref.U64}


def gated(name, label):
    return restated(name, label)["cu"] <= GATE


@functools.lru_cache(maxsize=None)
def reference(name, label):
    """(X, logdet, q) of the longdouble reference on the restatement's own L and d"""
    L, _ = factor(name)
    X, ld, q = lref.reference(L, restated(name, label)["d"], rhs(L.shape[0]))
    return _frozen(X), ld, _frozen(q)


@functools.lru_cache(maxsize=None)
def restatement_errors(name, label):
    """per column of the 33: the restatement's own relative error in X against the reference (e_rest of a column set is the max over the set)"""
    return _frozen(lref.column_errors(restated(name, label)["X"], reference(name, label)[0]))
