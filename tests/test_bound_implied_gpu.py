"""mi_lp_bound_implied_bounds(_from) / mi_lp_bound_tightened_columns(_from) /
mi_lp_get_tightened_columns (include/mi_lp.h) through mi_glop.engine.LpHandle,
on solved LPs of tests/lp_gen.py (the set-up of tests/test_bound_ranges_gpu.py).

Both forms equal, on every bit, the numpy reference of
tests/bound_implied_cases.py on the same bound sets; NULL row bounds mean the
loaded ones; every error of the header's table is returned and leaves the
outputs and the stored list alone; the four stores of a handle do not see each
other; k = 0; a handle that made the calls solves on exactly as one that never
did; cpsat.tightened_overrides fed back gives the second round's ranges; and a
known answer small enough to check by hand.
"""
import ctypes
import types

import numpy as np
import pytest

from mi_glop import abi, cpsat, engine
from mi_glop.lp import LinearProgram

import bound_implied_cases as ic
import bound_range_cases as bc
import lp_gen
from device_ref import bits

pytestmark = pytest.mark.gpu

ERROR_NULL, ERROR_INVALID_PROBLEM, ERROR_STATE, ERROR_DEVICE = 3, 4, 101, 100
INF = np.inf

_device_error = []


@pytest.fixture(autouse=True)
def _stop_after_a_device_error(monkeypatch):
    """A device error is never part of a test here: after one, nothing more
    is started on the GPU."""
    check = engine.LpHandle._check

    def recording_check(self, rc, what):
        if rc == ERROR_DEVICE:
            _device_error.append(f"{what}: {self.last_error()}")
        return check(self, rc, what)

    monkeypatch.setattr(engine.LpHandle, "_check", recording_check)
    yield
    if _device_error:
        pytest.exit(f"device error: {_device_error[0]}", returncode=3)


def _solved(m=60, n=200, density=0.08, seed=11, **kw):
    lp = lp_gen.random_sparse_lp(m, n, density, seed)
    g = engine.LpHandle(abi.default_params(**kw))
    assert hasattr(g, "implied_bounds"), "LpHandle has no implied column bounds"
    g.load(lp)
    assert g.solve().problem_status == abi.OPTIMAL
    return g, lp


@pytest.fixture(scope="module")
def solved():
    g, lp = _solved()
    yield g, lp
    g.close()


def _matrix(lp):
    """What bound_range_cases.ranges (rows) and bound_implied_cases.implied
    (columns) read of a matrix."""
    cols = [[] for _ in range(lp.m)]
    vals = [[] for _ in range(lp.m)]
    for c in range(lp.n):
        for i in range(lp.col_starts[c], lp.col_starts[c + 1]):
            cols[lp.row_idx[i]].append(c)
            vals[lp.row_idx[i]].append(lp.vals[i])
    return types.SimpleNamespace(
        m=lp.m, n=lp.n, col_starts=np.asarray(lp.col_starts), row_idx=np.asarray(lp.row_idx),
        vals=np.asarray(lp.vals, np.float64),
        t_cols=[np.array(c + [lp.n + r], np.int32) for r, c in enumerate(cols)],
        t_vals=[np.array(v + [1.0]) for v in vals])


def _children(lp, k, seed):
    """Children of a node: the loaded bounds (free and one-sided columns
    included) with some columns fixed, some boxed and some opened."""
    rng = np.random.default_rng(seed)
    L = np.tile(np.array(lp.col_lb, np.float64), (k, 1))
    U = np.tile(np.array(lp.col_ub, np.float64), (k, 1))
    for j in range(k):
        cols = rng.permutation(lp.n)[:2 + 3 * j]
        third = len(cols) // 3
        fixed, boxed, opened = cols[:third], cols[third:2 * third], cols[2 * third:]
        L[j, fixed] = U[j, fixed] = np.round(rng.normal(size=len(fixed)) * 3.0)
        L[j, boxed] = np.round(rng.normal(size=len(boxed)) * 4.0)
        U[j, boxed] = L[j, boxed] + rng.integers(0, 3, len(boxed))
        U[j, opened] = INF
    return L, U


def _as_overrides(lp, L, U):
    base_lb, base_ub = np.array(lp.col_lb, np.float64), np.array(lp.col_ub, np.float64)
    sets = []
    for lo, hi in zip(L, U):
        cols = np.nonzero((bits(lo) != bits(base_lb)) | (bits(hi) != bits(base_ub)))[0]
        sets.append((cols.astype(np.int32), lo[cols], hi[cols]))
    return base_lb, base_ub, sets


def _loaded_bounds(lp):
    return np.array(lp.row_lb, np.float64), np.array(lp.row_ub, np.float64)


def _reference(lp, L, U, rlb, rub):
    mat = _matrix(lp)
    return ic.implied(mat, L, U, bc.ranges(mat, L, U), rlb, rub)


@pytest.mark.parametrize("k", [1, 3, 17])
def test_both_forms_against_the_reference(solved, k):
    g, lp = solved
    L, U = _children(lp, k, 40 + k)
    rlb, rub = _loaded_bounds(lp)
    NL, NU = _reference(lp, L, U, rlb, rub)
    assert (bits(NU) != bits(U)).any() and (k < 17 or (bits(NL) != bits(L)).any())
    base_lb, base_ub, sets = _as_overrides(lp, L, U)
    # NULL row bounds mean the loaded ones, one at a time and both.
    for a, b in ((None, None), (rlb, None), (None, rub), (rlb, rub)):
        ic.same_bounds(g.implied_bounds(L, U, a, b), (NL, NU), f"k={k} dense")
    ic.same_bounds(g.implied_bounds_from(base_lb, base_ub, sets), (NL, NU), f"k={k} overrides")
    for tol in (0.0, 1e-6, 0.5):
        ref = ic.keep_reference(L, U, NL, NU, tol)
        ic.same_lists(g.tightened_columns(L, U, tolerance=tol), ref, f"k={k} tol={tol}")
        ic.same_lists(g.tightened_columns(L, U, rlb, rub, tol), ref, f"k={k} tol={tol} own bounds")
        ref_from = ic.keep_reference(L, U, NL, NU, tol, base=(base_lb, base_ub))
        ic.same_lists(g.tightened_columns_from(base_lb, base_ub, sets, tolerance=tol), ref_from,
                      f"k={k} tol={tol} overrides")
        only = g.tightened_columns(L, U, tolerance=tol, lists=False)
        assert only[:4] == (None, None, None, None)
        bc.same_summaries(only[4], ref[4], f"k={k} summaries only")
    if k == 17:
        assert 0 < ref[0][k] < k * lp.n
    # Row bounds of the caller's own, infinite on either side.
    lb = np.where(np.arange(lp.m) % 3 == 0, -INF, rlb - 1.0)
    ub = np.where(np.arange(lp.m) % 4 == 1, INF, rub + 0.5)
    ic.same_bounds(g.implied_bounds(L, U, lb, ub), _reference(lp, L, U, lb, ub), "own row bounds")
    with pytest.raises(ValueError):
        g.implied_bounds(np.zeros((2, lp.n + 1)), np.zeros((2, lp.n + 1)))
    with pytest.raises(ValueError):
        g.tightened_columns(L, U, row_lb=np.zeros(lp.m + 1))


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _dense(g, h, L, U, k, lb, ub, lo, hi):
    return g._L.mi_lp_bound_implied_bounds(h, _vp(L), _vp(U), k, _vp(lb), _vp(ub), _vp(lo),
                                           _vp(hi))


def _dense_from(g, h, bl, bu, k, ov, lb, ub, lo, hi):
    s, c, a, b = ov
    return g._L.mi_lp_bound_implied_bounds_from(h, _vp(bl), _vp(bu), k, _vp(s), _vp(c), _vp(a),
                                                _vp(b), _vp(lb), _vp(ub), _vp(lo), _vp(hi))


def _lists(g, h, L, U, k, lb, ub, tol, starts, summaries):
    return g._L.mi_lp_bound_tightened_columns(h, _vp(L), _vp(U), k, _vp(lb), _vp(ub), tol,
                                              _vp(starts), _vp(summaries))


def _lists_from(g, h, bl, bu, k, ov, lb, ub, tol, starts, summaries):
    s, c, a, b = ov
    return g._L.mi_lp_bound_tightened_columns_from(h, _vp(bl), _vp(bu), k, _vp(s), _vp(c),
                                                   _vp(a), _vp(b), _vp(lb), _vp(ub), tol,
                                                   _vp(starts), _vp(summaries))


def _get(g, h, cols, lo, hi):
    return g._L.mi_lp_get_tightened_columns(h, _vp(cols), _vp(lo), _vp(hi))


class _Outputs:
    """Every output filled with a mark, and the stored list as it was;
    untouched() is true while none of them changed."""

    def __init__(self, g, k, n):
        self.g = g
        self.starts = np.full(k + 1, -9, np.int64)
        self.summaries = np.zeros(k, engine.POINT_VIOLATIONS)
        self.summaries["count"] = -9
        self.lo, self.hi = np.full(k * n, -9.5), np.full(k * n, -9.5)
        self.stored = self._stored()

    def _stored(self):
        cols, lo, hi = np.full(4096, -9, np.int32), np.full(4096, -9.5), np.full(4096, -9.5)
        rc = _get(self.g, self.g.h, cols, lo, hi)
        return rc, cols.tobytes(), lo.tobytes(), hi.tobytes()

    def untouched(self):
        return (np.all(self.starts == -9) and np.all(self.summaries["count"] == -9) and
                np.all(self.lo == -9.5) and np.all(self.hi == -9.5) and
                self._stored() == self.stored)


def test_errors_write_nothing_and_keep_the_stored_list(solved):
    g, lp = solved
    n, m = lp.n, lp.m
    L, U = np.full(2 * n, -1.0), np.full(2 * n, 1.0)
    # Upper row bounds just above the rows' minima, so that columns move.
    lo, hi, _, _ = bc.ranges(_matrix(lp), L.reshape(2, n), U.reshape(2, n))
    lb, ub = np.full(m, -INF), lo[0] + 0.01 * (hi[0] - lo[0])
    first = g.tightened_columns(L.reshape(2, n), U.reshape(2, n), lb, ub)
    assert 0 < first[0][2] < 4096
    o = _Outputs(g, 2, n)
    assert o.stored[0] == 0
    no_ov = (np.zeros(3, np.int64), None, None, None)

    def bad(r, value, upper):
        b = (ub if upper else lb).copy()
        b[r] = value
        return (lb, b) if upper else (b, ub)

    # MI_LP_ERROR_INVALID_PROBLEM.
    for k, bl, bu, tol in [(-1, lb, ub, 0.0), (2, lb, ub, -1e-9), (2, lb, ub, np.nan),
                           (2, lb, ub, INF), (2, *bad(3, np.nan, False), 0.0),
                           (2, *bad(m - 1, np.nan, True), 0.0)]:
        assert _lists(g, g.h, L, U, k, bl, bu, tol, o.starts, o.summaries) == ERROR_INVALID_PROBLEM
        assert _lists_from(g, g.h, L, U, k, no_ov, bl, bu, tol, o.starts,
                           o.summaries) == ERROR_INVALID_PROBLEM
        if tol == 0.0:  # the dense calls take no tolerance
            assert _dense(g, g.h, L, U, k, bl, bu, o.lo, o.hi) == ERROR_INVALID_PROBLEM
            assert _dense_from(g, g.h, L, U, k, no_ov, bl, bu, o.lo,
                               o.hi) == ERROR_INVALID_PROBLEM
        assert o.untouched(), (k, tol)
    i64, i32 = lambda a: np.array(a, np.int64), lambda a: np.array(a, np.int32)
    vals = np.ones(4)
    for starts, cols in [(i64([0, 2, 4]), i32([0, 1, 5, 5])),   # the same column twice in a set
                         (i64([0, 2, 4]), i32([0, n, 1, 2])),   # a slack column: out of range
                         (i64([0, 2, 4]), i32([0, 1, -1, 2])),
                         (i64([0, 3, 2]), i32([0, 1, 2, 3])),   # decreasing starts
                         (i64([1, 2, 4]), i32([0, 1, 2, 3]))]:  # starts[0] != 0
        ov = (starts, cols, vals, vals)
        assert _lists_from(g, g.h, L, U, 2, ov, lb, ub, 0.0, o.starts,
                           o.summaries) == ERROR_INVALID_PROBLEM
        assert _dense_from(g, g.h, L, U, 2, ov, lb, ub, o.lo, o.hi) == ERROR_INVALID_PROBLEM
        assert o.untouched(), starts
    # MI_LP_ERROR_NULL.
    ov = (i64([0, 1, 2]), i32([0, 1]), np.ones(2), np.ones(2))
    assert _lists(g, None, L, U, 2, lb, ub, 0.0, o.starts, o.summaries) == ERROR_NULL
    assert _lists(g, g.h, None, U, 2, lb, ub, 0.0, o.starts, o.summaries) == ERROR_NULL
    assert _lists(g, g.h, L, None, 2, lb, ub, 0.0, o.starts, o.summaries) == ERROR_NULL
    assert _lists(g, g.h, L, U, 2, lb, ub, 0.0, None, None) == ERROR_NULL
    assert _lists_from(g, None, L, U, 2, ov, lb, ub, 0.0, o.starts, o.summaries) == ERROR_NULL
    assert _lists_from(g, g.h, None, U, 2, ov, lb, ub, 0.0, o.starts, o.summaries) == ERROR_NULL
    assert _lists_from(g, g.h, L, None, 2, ov, lb, ub, 0.0, o.starts, o.summaries) == ERROR_NULL
    assert _lists_from(g, g.h, L, U, 2, ov, lb, ub, 0.0, None, None) == ERROR_NULL
    for missing in range(4):
        part = tuple(None if i == missing else a for i, a in enumerate(ov))
        assert _lists_from(g, g.h, L, U, 2, part, lb, ub, 0.0, o.starts, o.summaries) == ERROR_NULL
        assert _dense_from(g, g.h, L, U, 2, part, lb, ub, o.lo, o.hi) == ERROR_NULL
    assert _dense(g, None, L, U, 2, lb, ub, o.lo, o.hi) == ERROR_NULL
    assert _dense(g, g.h, None, U, 2, lb, ub, o.lo, o.hi) == ERROR_NULL
    assert _dense(g, g.h, L, None, 2, lb, ub, o.lo, o.hi) == ERROR_NULL
    assert _dense(g, g.h, L, U, 2, lb, ub, None, o.hi) == ERROR_NULL
    assert _dense(g, g.h, L, U, 2, lb, ub, o.lo, None) == ERROR_NULL
    assert _dense_from(g, g.h, None, U, 2, ov, lb, ub, o.lo, o.hi) == ERROR_NULL
    assert _dense_from(g, g.h, L, U, 2, ov, lb, ub, None, o.hi) == ERROR_NULL
    one = np.zeros(1)
    assert _get(g, None, np.zeros(1, np.int32), one, one) == ERROR_NULL
    assert _get(g, g.h, None, one, one) == ERROR_NULL
    assert _get(g, g.h, np.zeros(1, np.int32), None, one) == ERROR_NULL
    assert _get(g, g.h, np.zeros(1, np.int32), one, None) == ERROR_NULL
    assert o.untouched()
    # Summaries may be NULL, and col_starts may be NULL (summaries only: the
    # stored list stays).
    assert _lists(g, g.h, L, U, 2, lb, ub, 0.0, None, o.summaries) == 0
    assert np.array_equal(o.summaries["count"], first[4]["count"])
    assert o._stored() == o.stored
    assert _lists(g, g.h, L, U, 2, lb, ub, 0.0, o.starts, None) == 0
    assert np.array_equal(o.starts, first[0]) and o._stored() == o.stored
    # k = 0 of the dense calls succeeds and writes nothing.
    assert _dense(g, g.h, L, U, 0, lb, ub, o.lo, o.hi) == 0 and np.all(o.lo == -9.5)
    # +-inf row bounds on either side are allowed, and give no candidate.
    free = g.implied_bounds(L.reshape(2, n), U.reshape(2, n), np.full(m, INF), np.full(m, -INF))
    ic.same_bounds(free, (L.reshape(2, n), U.reshape(2, n)), "crossed row bounds")


def test_error_state_and_k_zero():
    lp = lp_gen.random_sparse_lp(20, 50, 0.2, 8)
    g = engine.LpHandle(abi.default_params())
    g.load(lp)
    L, U = np.full(lp.n, -1.0), np.ones(lp.n)
    lb, ub = np.full(lp.m, -1.0), np.full(lp.m, 0.0)
    starts = np.full(2, -9, np.int64)
    summaries = np.zeros(1, engine.POINT_VIOLATIONS)
    summaries["count"] = -9
    lo, hi = np.full(lp.n, -9.5), np.full(lp.n, -9.5)
    cols, a, b = np.zeros(64, np.int32), np.zeros(64), np.zeros(64)
    no_ov = (np.zeros(2, np.int64), None, None, None)
    # Before a solve, and no list before any list-building call.
    assert _lists(g, g.h, L, U, 1, lb, ub, 0.0, starts, summaries) == ERROR_STATE
    assert _lists_from(g, g.h, L, U, 1, no_ov, lb, ub, 0.0, starts, summaries) == ERROR_STATE
    assert _dense(g, g.h, L, U, 1, lb, ub, lo, hi) == ERROR_STATE
    assert _dense_from(g, g.h, L, U, 1, no_ov, lb, ub, lo, hi) == ERROR_STATE
    assert _get(g, g.h, cols, a, b) == ERROR_STATE
    assert np.all(starts == -9) and summaries["count"][0] == -9 and np.all(lo == -9.5)
    assert g.solve().problem_status == abi.OPTIMAL
    assert _get(g, g.h, cols, a, b) == ERROR_STATE
    assert _lists(g, g.h, L, U, 1, lb, ub, 0.0, None, summaries) == 0  # summaries only: no list
    assert _get(g, g.h, cols, a, b) == ERROR_STATE
    assert _lists(g, g.h, L, U, 1, lb, ub, 0.0, starts, summaries) == 0
    assert _get(g, g.h, cols, a, b) == 0
    # k = 0 succeeds, writes col_starts[0] = 0 and stores an empty list.
    starts[:] = -9
    assert _lists(g, g.h, L, U, 0, lb, ub, 0.0, starts, None) == 0 and starts[0] == 0
    cols[:] = -9
    assert _get(g, g.h, cols, a, b) == 0 and np.all(cols == -9)
    got = g.tightened_columns_from(L, U, [], lb, ub)
    assert list(got[0]) == [0] and all(len(x) == 0 for x in got[1:])
    assert cpsat.tightened_overrides(got) == []
    dense = g.implied_bounds(np.zeros((0, lp.n)), np.zeros((0, lp.n)))
    assert dense[0].shape == dense[1].shape == (0, lp.n)
    # After mi_lp_load the list is gone.
    g.load(lp)
    assert _get(g, g.h, cols, a, b) == ERROR_STATE
    g.close()


def test_the_four_stores_are_separate(solved):
    g, lp = solved
    L, U = _children(lp, 5, 77)
    mine = g.tightened_columns(L, U)
    assert len(mine[1]) > 0
    infeasible = g.infeasible_rows(L, U, np.full(lp.m, INF), np.full(lp.m, -INF))
    x = np.tile(np.concatenate([g.primal(), -g.activities()]), (3, 1))
    x[:, ::2] += 1.0
    violated = g.column_violations(x, tolerance=1e-9)
    sparse = g.row_combinations_sparse(np.random.default_rng(5).normal(size=(3, lp.m)), 1e-9)
    assert len(infeasible[1]) > 0 and len(violated[1]) > 0 and len(sparse[1]) > 0

    def stored(call, want_idx, want_vals):
        idx, vals = np.zeros(len(want_idx) + 1, np.int32), np.zeros(len(want_idx) + 1)
        assert call(g.h, _vp(idx), _vp(vals)) == 0
        assert np.array_equal(idx[:-1], want_idx), call
        assert np.array_equal(bits(vals[:-1]), bits(want_vals)), call

    def mine_stored(want):
        kept = len(want[1])
        cols, lo, hi = np.zeros(kept + 1, np.int32), np.zeros(kept + 1), np.zeros(kept + 1)
        assert _get(g, g.h, cols, lo, hi) == 0
        assert np.array_equal(cols[:-1], want[1])
        assert np.array_equal(bits(lo[:-1]), bits(want[2]))
        assert np.array_equal(bits(hi[:-1]), bits(want[3]))

    # Each store still holds what its own call left, after the three others ran.
    mine_stored(mine)
    stored(g._L.mi_lp_get_infeasible_rows, infeasible[1], infeasible[2])
    stored(g._L.mi_lp_get_violated_rows, violated[1], violated[2])
    stored(g._L.mi_lp_get_sparse_rows, sparse[1], sparse[2])
    # And a new list of this call disturbs none of the others.
    again = g.tightened_columns(L[:2], U[:2], tolerance=0.25)
    mine_stored(again)
    stored(g._L.mi_lp_get_infeasible_rows, infeasible[1], infeasible[2])
    stored(g._L.mi_lp_get_violated_rows, violated[1], violated[2])
    stored(g._L.mi_lp_get_sparse_rows, sparse[1], sparse[2])


def test_a_later_solve_does_not_see_the_calls():
    """Two handles solve the same LP; one makes the calls in between; then
    both get the same tighter bounds and solve on from their bases."""
    g, lp = _solved(use_dual_simplex=1)
    q, _ = _solved(use_dual_simplex=1)
    try:
        L, U = _children(lp, 17, 95)
        g.implied_bounds(L, U)
        g.tightened_columns(L, U, tolerance=1e-9)
        g.tightened_columns(L, U, lists=False)
        g.tightened_columns_from(*_as_overrides(lp, L, U))
        star = q.primal()
        lb, ub = np.array(lp.col_lb), np.array(lp.col_ub)
        moved = [c for c in range(lp.n) if np.isfinite(lb[c]) and star[c] > lb[c] + 1e-3][:6]
        assert moved
        for c in moved:
            ub[c] = 0.5 * (lb[c] + star[c])
        results = []
        for h in (g, q):
            h.set_variable_bounds(lb, ub)
            results.append(h.solve())
        rg, rq = results
        assert rq.iterations > 0
        assert (rg.problem_status, rg.iterations) == (rq.problem_status, rq.iterations)
        assert np.array_equal(g.basis(), q.basis())
        assert np.array_equal(g.state(), q.state())
        assert np.array_equal(bits(g.primal()), bits(q.primal()))
        assert np.array_equal(bits(g.duals()), bits(q.duals()))
    finally:
        g.close()
        q.close()


def test_tightened_overrides_fed_back(solved):
    """The override form's lists, fed back unchanged, are the next round's
    sets: their ranges equal bound_activity_ranges on the materialised
    tightened sets, and their second round equals the dense second round."""
    g, lp = solved
    L, U = _children(lp, 9, 123)
    base_lb, base_ub, sets = _as_overrides(lp, L, U)
    result = g.tightened_columns_from(base_lb, base_ub, sets)
    fed = cpsat.tightened_overrides(result)
    assert len(fed) == 9 and sum(len(c) for c, _, _ in fed) == result[0][9] > 0
    TL, TU = bc.materialise(base_lb, base_ub, fed)
    NL, NU = g.implied_bounds(L, U)
    # At tolerance 0 the materialised sets are the implied bounds wherever a
    # difference is finite.
    with np.errstate(invalid="ignore", over="ignore"):
        odd = ~np.isfinite(NL - L) | ~np.isfinite(U - NU)
    assert not (((bits(TL) != bits(NL)) | (bits(TU) != bits(NU))) & ~odd).any()
    bc.same_ranges(g.bound_activity_ranges_from(base_lb, base_ub, fed),
                   g.bound_activity_ranges(TL, TU), "second round's ranges")
    bc.same_ranges(g.bound_activity_ranges(TL, TU), bc.ranges(_matrix(lp), TL, TU),
                   "second round's ranges against the reference")
    ic.same_bounds(g.implied_bounds_from(base_lb, base_ub, fed), g.implied_bounds(TL, TU),
                   "second round")
    bc.same_result(g.infeasible_rows_from(base_lb, base_ub, fed), g.infeasible_rows(TL, TU),
                   "screening of the tightened sets")


def test_known_answer():
    """x + y <= 4 with x, y in [0, 10]: the row's minimum is 0, so each
    variable is at most (4 - (0 - 1 * 0)) / 1 = 4. A second child with x >= 5
    crosses: y <= 4 - 5 = -1 < 0 = its lower bound, by 1; x <= 4 < 5, by 1 too,
    and x is the lower column."""
    lp = LinearProgram(m=1, n=2, col_starts=np.array([0, 1, 2], np.int64),
                       row_idx=np.array([0, 0], np.int32), vals=np.ones(2),
                       col_lb=np.zeros(2), col_ub=np.full(2, 10.0), row_lb=np.full(1, -INF),
                       row_ub=np.array([4.0]), obj=-np.ones(2))
    g = engine.LpHandle(abi.default_params())
    try:
        g.load(lp)
        assert g.solve().problem_status == abi.OPTIMAL
        lbs = np.array([[0.0, 0.0], [5.0, 0.0]])
        ubs = np.full((2, 2), 10.0)
        nl, nu = g.implied_bounds(lbs, ubs)
        assert nl.tolist() == [[0.0, 0.0], [5.0, 0.0]]
        assert nu.tolist() == [[4.0, 4.0], [4.0, -1.0]]
        starts, cols, lo, hi, summaries = g.tightened_columns(lbs, ubs)
        assert starts.tolist() == [0, 2, 4] and cols.tolist() == [0, 1, 0, 1]
        assert lo.tolist() == [0.0, 0.0, 5.0, 0.0] and hi.tolist() == [4.0, 4.0, 4.0, -1.0]
        assert summaries["count"].tolist() == [2, 2]
        assert summaries["worst_row"].tolist() == [-1, 0]  # not proven; proven by column 0
        assert summaries["worst"].tolist() == [0.0, 1.0]
        # A tolerance of 6 keeps nothing of the first child (both moved by 6
        # exactly) and nothing of the second.
        starts, cols, _, _, summaries = g.tightened_columns(lbs, ubs, tolerance=6.0)
        assert starts.tolist() == [0, 0, 1] and cols.tolist() == [1]  # y moved by 11
        assert summaries["worst_row"].tolist() == [-1, -1]
        over = g.tightened_columns_from(lbs[0], ubs[0], [((), (), ()), ([0], [5.0], [10.0])],
                                        tolerance=6.0)
        assert over[0].tolist() == [0, 0, 2] and over[1].tolist() == [0, 1]  # x changed
    finally:
        g.close()
