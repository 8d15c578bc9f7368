"""mi_lp_bound_activity_ranges(_from) / mi_lp_bound_infeasible_rows(_from) /
mi_lp_get_infeasible_rows (include/mi_lp.h) through mi_glop.engine.LpHandle,
on solved LPs of tests/lp_gen.py (the set-up of
tests/test_column_violations_gpu.py).

Both forms equal, on every bit, the numpy reference of
tests/bound_range_cases.py on the same bound sets; NULL row bounds mean the
loaded ones; every error of the header's table is returned and leaves the
outputs and the stored list alone; the three stores of a handle do not see
each other; a handle that made the calls solves on exactly as one that never
did; cpsat.branch_overrides through infeasible_rows_from equals branch_lps
through infeasible_rows; and the screen is sound against the solver on a small
LP whose infeasible child is known.
"""
import ctypes
import types

import numpy as np
import pytest

from mi_glop import abi, cpsat, engine
from mi_glop.lp import LinearProgram

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
    assert hasattr(g, "bound_activity_ranges"), "LpHandle has no bound-set activity ranges"
    g.load(lp)
    assert g.solve().problem_status == abi.OPTIMAL
    return g, lp


@pytest.fixture(scope="module")
def solved():
    g, lp = _solved()
    yield g, lp
    g.close()


def _rows(lp):
    """What bound_range_cases.ranges reads of a matrix: per row the structural
    entries in increasing column order, and a last entry it leaves out."""
    cols = [[] for _ in range(lp.m)]
    vals = [[] for _ in range(lp.m)]
    for c in range(lp.n):
        for i in range(lp.col_starts[c], lp.col_starts[c + 1]):
            cols[lp.row_idx[i]].append(c)
            vals[lp.row_idx[i]].append(lp.vals[i])
    return types.SimpleNamespace(
        m=lp.m, t_cols=[np.array(c + [lp.n + r], np.int32) for r, c in enumerate(cols)],
        t_vals=[np.array(v + [1.0]) for v in vals])


def _children(lp, k, seed):
    """Children of a node: the loaded bounds (free and one-sided columns
    included) with some columns fixed far out, some boxed and some opened."""
    rng = np.random.default_rng(seed)
    L = np.tile(np.array(lp.col_lb, np.float64), (k, 1))
    U = np.tile(np.array(lp.col_ub, np.float64), (k, 1))
    for j in range(k):
        cols = rng.permutation(lp.n)[:2 + 3 * j]
        third = len(cols) // 3
        fixed, boxed, opened = cols[:third], cols[third:2 * third], cols[2 * third:]
        L[j, fixed] = U[j, fixed] = np.round(rng.normal(size=len(fixed)) * 100.0)
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


@pytest.mark.parametrize("k", [1, 3, 17])
def test_both_forms_against_the_reference(solved, k):
    g, lp = solved
    L, U = _children(lp, k, 40 + k)
    want = bc.ranges(_rows(lp), L, U)
    assert want[2].any() and want[3].any()  # free columns: infinite bounds are counted
    got = g.bound_activity_ranges(L, U)
    bc.same_ranges(got, want, f"k={k} dense")
    base_lb, base_ub, sets = _as_overrides(lp, L, U)
    over = g.bound_activity_ranges_from(base_lb, base_ub, sets)
    bc.same_ranges(over, want, f"k={k} overrides")
    rlb, rub = _loaded_bounds(lp)
    for tol in (0.0, 1e-6):
        ref = bc.filter_reference(want, rlb, rub, tol)
        # NULL row bounds mean the loaded ones, one at a time and both.
        for a, b in ((None, None), (rlb, None), (None, rub), (rlb, rub)):
            bc.same_result(g.infeasible_rows(L, U, a, b, tol), ref, f"k={k} tol={tol}")
        bc.same_result(g.infeasible_rows_from(base_lb, base_ub, sets, tolerance=tol), ref,
                       f"k={k} tol={tol} overrides")
        only = g.infeasible_rows(L, U, tolerance=tol, lists=False)
        assert only[:3] == (None, None, None)
        bc.same_summaries(only[3], ref[3], f"k={k} summaries only")
    if k == 17:
        assert 0 < ref[0][k] < k * lp.m  # columns fixed far out put rows past their bounds
    # Row bounds of the caller's own, infinite on either side.
    lb = np.where(np.arange(lp.m) % 3 == 0, INF, np.quantile(want[1], 0.5, axis=0))
    ub = np.where(np.arange(lp.m) % 4 == 1, -INF, INF)
    lb = np.where(np.isnan(lb), -INF, lb)
    bc.same_result(g.infeasible_rows(L, U, lb, ub, 0.25), bc.filter_reference(want, lb, ub, 0.25),
                   "own row bounds")
    with pytest.raises(ValueError):
        g.bound_activity_ranges(np.zeros((2, lp.n + 1)), np.zeros((2, lp.n + 1)))
    with pytest.raises(ValueError):
        g.infeasible_rows(L, U, row_lb=np.zeros(lp.m + 1))


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _dense(g, h, L, U, k, lb, ub, tol, starts, summaries):
    return g._L.mi_lp_bound_infeasible_rows(h, _vp(L), _vp(U), k, _vp(lb), _vp(ub), tol,
                                            _vp(starts), _vp(summaries))


def _from(g, h, bl, bu, k, ov, lb, ub, tol, starts, summaries):
    s, c, lo, hi = ov
    return g._L.mi_lp_bound_infeasible_rows_from(h, _vp(bl), _vp(bu), k, _vp(s), _vp(c), _vp(lo),
                                                 _vp(hi), _vp(lb), _vp(ub), tol, _vp(starts),
                                                 _vp(summaries))


def _ranges(g, h, L, U, k, lo, hi, counts):
    return g._L.mi_lp_bound_activity_ranges(h, _vp(L), _vp(U), k, _vp(lo), _vp(hi), _vp(counts))


def _ranges_from(g, h, bl, bu, k, ov, lo, hi, counts):
    s, c, a, b = ov
    return g._L.mi_lp_bound_activity_ranges_from(h, _vp(bl), _vp(bu), k, _vp(s), _vp(c), _vp(a),
                                                 _vp(b), _vp(lo), _vp(hi), _vp(counts))


def _get(g, h, rows, vals):
    return g._L.mi_lp_get_infeasible_rows(h, _vp(rows), _vp(vals))


class _Outputs:
    """Every output filled with a mark, and the stored list as it was;
    untouched() is true while none of them changed."""

    def __init__(self, g, k, m):
        self.g = g
        self.starts = np.full(k + 1, -9, np.int64)
        self.summaries = np.zeros(k, engine.POINT_VIOLATIONS)
        self.summaries["count"] = -9
        self.lo, self.hi = np.full(k * m, -9.5), np.full(k * m, -9.5)
        self.counts = np.full(2 * k * m, -9, np.int32)
        self.stored = self._stored()

    def _stored(self):
        rows, vals = np.full(4096, -9, np.int32), np.full(4096, -9.5)
        rc = _get(self.g, self.g.h, rows, vals)
        return rc, rows.tobytes(), vals.tobytes()

    def untouched(self):
        return (np.all(self.starts == -9) and np.all(self.summaries["count"] == -9) and
                np.all(self.lo == -9.5) and np.all(self.hi == -9.5) and
                np.all(self.counts == -9) and self._stored() == self.stored)


def test_errors_write_nothing_and_keep_the_stored_list(solved):
    g, lp = solved
    n, m = lp.n, lp.m
    L, U = np.full(2 * n, 1.0), np.full(2 * n, 1.0)
    lb, ub = np.full(m, -1.0), np.full(m, 1.0)
    first = g.infeasible_rows(L.reshape(2, n), U.reshape(2, n), lb, ub)
    assert 0 < first[0][2] < 4096
    o = _Outputs(g, 2, m)
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
        assert _dense(g, g.h, L, U, k, bl, bu, tol, o.starts, o.summaries) == ERROR_INVALID_PROBLEM
        assert _from(g, g.h, L, U, k, no_ov, bl, bu, tol, o.starts,
                     o.summaries) == ERROR_INVALID_PROBLEM
        assert o.untouched(), (k, tol)
    assert _ranges(g, g.h, L, U, -1, o.lo, o.hi, o.counts) == ERROR_INVALID_PROBLEM
    assert _ranges_from(g, g.h, L, U, -1, no_ov, o.lo, o.hi, o.counts) == ERROR_INVALID_PROBLEM
    i64, i32 = lambda a: np.array(a, np.int64), lambda a: np.array(a, np.int32)
    vals = np.ones(4)
    for starts, cols in [(i64([0, 2, 4]), i32([0, 1, 5, 5])),   # the same column twice in a set
                         (i64([0, 2, 4]), i32([0, n, 1, 2])),   # a slack column: out of range
                         (i64([0, 2, 4]), i32([0, 1, -1, 2])),
                         (i64([0, 3, 2]), i32([0, 1, 2, 3])),   # decreasing starts
                         (i64([1, 2, 4]), i32([0, 1, 2, 3]))]:  # starts[0] != 0
        ov = (starts, cols, vals, vals)
        assert _from(g, g.h, L, U, 2, ov, lb, ub, 0.0, o.starts,
                     o.summaries) == ERROR_INVALID_PROBLEM
        assert _ranges_from(g, g.h, L, U, 2, ov, o.lo, o.hi, o.counts) == ERROR_INVALID_PROBLEM
        assert o.untouched(), starts
    # +-inf row bounds on either side are allowed.
    crossed = g.infeasible_rows(L.reshape(2, n), U.reshape(2, n), np.full(m, INF), np.full(m, -INF))
    assert crossed[0][2] == 2 * m and np.all(crossed[2] == INF)
    g.infeasible_rows(L.reshape(2, n), U.reshape(2, n), lb, ub)  # the watched list again
    # MI_LP_ERROR_NULL.
    ov = (i64([0, 1, 2]), i32([0, 1]), np.ones(2), np.ones(2))
    assert _dense(g, None, L, U, 2, lb, ub, 0.0, o.starts, o.summaries) == ERROR_NULL
    assert _dense(g, g.h, None, U, 2, lb, ub, 0.0, o.starts, o.summaries) == ERROR_NULL
    assert _dense(g, g.h, L, None, 2, lb, ub, 0.0, o.starts, o.summaries) == ERROR_NULL
    assert _dense(g, g.h, L, U, 2, lb, ub, 0.0, None, None) == ERROR_NULL
    assert _from(g, None, L, U, 2, ov, lb, ub, 0.0, o.starts, o.summaries) == ERROR_NULL
    assert _from(g, g.h, None, U, 2, ov, lb, ub, 0.0, o.starts, o.summaries) == ERROR_NULL
    assert _from(g, g.h, L, None, 2, ov, lb, ub, 0.0, o.starts, o.summaries) == ERROR_NULL
    for missing in range(4):
        part = tuple(None if i == missing else a for i, a in enumerate(ov))
        assert _from(g, g.h, L, U, 2, part, lb, ub, 0.0, o.starts, o.summaries) == ERROR_NULL
        assert _ranges_from(g, g.h, L, U, 2, part, o.lo, o.hi, o.counts) == ERROR_NULL
    assert _from(g, g.h, L, U, 2, ov, lb, ub, 0.0, None, None) == ERROR_NULL
    assert _ranges(g, None, L, U, 2, o.lo, o.hi, o.counts) == ERROR_NULL
    assert _ranges(g, g.h, None, U, 2, o.lo, o.hi, o.counts) == ERROR_NULL
    assert _ranges(g, g.h, L, None, 2, o.lo, o.hi, o.counts) == ERROR_NULL
    assert _ranges(g, g.h, L, U, 2, None, o.hi, o.counts) == ERROR_NULL
    assert _ranges(g, g.h, L, U, 2, o.lo, None, o.counts) == ERROR_NULL
    assert _ranges_from(g, g.h, None, U, 2, ov, o.lo, o.hi, o.counts) == ERROR_NULL
    assert _ranges_from(g, g.h, L, U, 2, ov, None, o.hi, o.counts) == ERROR_NULL
    assert _get(g, None, np.zeros(1, np.int32), np.zeros(1)) == ERROR_NULL
    assert _get(g, g.h, None, np.zeros(1)) == ERROR_NULL
    assert _get(g, g.h, np.zeros(1, np.int32), None) == ERROR_NULL
    assert o.untouched()
    # Summaries may be NULL, row_starts may be NULL (summaries only: the stored
    # list stays), and so may inf_counts.
    assert _dense(g, g.h, L, U, 2, lb, ub, 0.0, None, o.summaries) == 0
    assert np.array_equal(o.summaries["count"], first[3]["count"])
    assert o._stored() == o.stored
    assert _dense(g, g.h, L, U, 2, lb, ub, 0.0, o.starts, None) == 0
    assert np.array_equal(o.starts, first[0]) and o._stored() == o.stored
    assert _ranges(g, g.h, L, U, 2, o.lo, o.hi, None) == 0
    want = bc.ranges(_rows(lp), L.reshape(2, n), U.reshape(2, n))
    assert np.array_equal(bits(o.lo), bits(want[0].ravel()))
    assert np.array_equal(bits(o.hi), bits(want[1].ravel())) and np.all(o.counts == -9)
    assert _ranges(g, g.h, L, U, 0, o.lo, o.hi, o.counts) == 0 and np.all(o.counts == -9)


def test_error_state():
    lp = lp_gen.random_sparse_lp(20, 50, 0.2, 8)
    g = engine.LpHandle(abi.default_params())
    g.load(lp)
    L, U, lb, ub = np.zeros(lp.n), np.ones(lp.n), np.full(lp.m, -1.0), np.full(lp.m, 0.0)
    starts = np.full(2, -9, np.int64)
    summaries = np.zeros(1, engine.POINT_VIOLATIONS)
    summaries["count"] = -9
    lo, hi = np.full(lp.m, -9.5), np.full(lp.m, -9.5)
    rows, vals = np.zeros(64, np.int32), np.zeros(64)
    no_ov = (np.zeros(2, np.int64), None, None, None)
    # Before a solve, and no list before any list-building call.
    assert _dense(g, g.h, L, U, 1, lb, ub, 0.0, starts, summaries) == ERROR_STATE
    assert _from(g, g.h, L, U, 1, no_ov, lb, ub, 0.0, starts, summaries) == ERROR_STATE
    assert _ranges(g, g.h, L, U, 1, lo, hi, None) == ERROR_STATE
    assert _ranges_from(g, g.h, L, U, 1, no_ov, lo, hi, None) == ERROR_STATE
    assert _get(g, g.h, rows, vals) == ERROR_STATE
    assert np.all(starts == -9) and summaries["count"][0] == -9 and np.all(lo == -9.5)
    assert g.solve().problem_status == abi.OPTIMAL
    assert _get(g, g.h, rows, vals) == ERROR_STATE
    assert _dense(g, g.h, L, U, 1, lb, ub, 0.0, None, summaries) == 0  # summaries only: no list
    assert _get(g, g.h, rows, vals) == ERROR_STATE
    assert _dense(g, g.h, L, U, 1, lb, ub, 0.0, starts, summaries) == 0
    assert _get(g, g.h, rows, vals) == 0
    # k = 0 succeeds, writes row_starts[0] = 0 and stores an empty list.
    starts[:] = -9
    assert _dense(g, g.h, L, U, 0, lb, ub, 0.0, starts, None) == 0 and starts[0] == 0
    rows[:] = -9
    assert _get(g, g.h, rows, vals) == 0 and np.all(rows == -9)
    got = g.infeasible_rows_from(L, U, [], lb, ub)
    assert list(got[0]) == [0] and len(got[1]) == len(got[2]) == len(got[3]) == 0
    # After mi_lp_load the list is gone.
    g.load(lp)
    assert _get(g, g.h, rows, vals) == ERROR_STATE
    g.close()


def test_the_three_stores_are_separate(solved):
    g, lp = solved
    L, U = _children(lp, 5, 77)
    mine = g.infeasible_rows(L, U, np.full(lp.m, INF), np.full(lp.m, -INF))
    assert len(mine[1]) > 0
    x = np.tile(np.concatenate([g.primal(), -g.activities()]), (3, 1))
    x[:, ::2] += 1.0
    violated = g.column_violations(x, tolerance=1e-9)
    sparse = g.row_combinations_sparse(np.random.default_rng(5).normal(size=(3, lp.m)), 1e-9)
    assert len(violated[1]) > 0 and len(sparse[1]) > 0

    def stored(call, want_idx, want_vals):
        idx, vals = np.zeros(len(want_idx) + 1, np.int32), np.zeros(len(want_idx) + 1)
        assert call(g.h, _vp(idx), _vp(vals)) == 0
        assert np.array_equal(idx[:-1], want_idx), call
        assert np.array_equal(bits(vals[:-1]), bits(want_vals)), call

    # Each store still holds what its own call left, after the two others ran.
    stored(g._L.mi_lp_get_infeasible_rows, mine[1], mine[2])
    stored(g._L.mi_lp_get_violated_rows, violated[1], violated[2])
    stored(g._L.mi_lp_get_sparse_rows, sparse[1], sparse[2])
    # And a new list of the screening disturbs neither of the others.
    again = g.infeasible_rows(L[:2], U[:2])
    stored(g._L.mi_lp_get_infeasible_rows, again[1], again[2])
    stored(g._L.mi_lp_get_violated_rows, violated[1], violated[2])
    stored(g._L.mi_lp_get_sparse_rows, sparse[1], sparse[2])


@pytest.mark.parametrize("dual", [0, 1])
def test_a_later_solve_does_not_see_the_calls(dual):
    """Two handles solve the same LP; one makes the calls in between; then
    both get the same tighter bounds and solve on from their bases."""
    g, lp = _solved(use_dual_simplex=dual)
    q, _ = _solved(use_dual_simplex=dual)
    try:
        L, U = _children(lp, 17, 95)
        g.bound_activity_ranges(L, U)
        g.infeasible_rows(L, U, tolerance=1e-9)
        g.infeasible_rows(L, U, lists=False)
        g.infeasible_rows_from(*_as_overrides(lp, L, U))
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
        assert bits(np.float64(rg.objective)) == bits(np.float64(rq.objective))
    finally:
        g.close()
        q.close()


def test_branch_overrides_equal_branch_lps(solved):
    g, lp = solved
    star = g.primal()
    lb = np.where(np.isfinite(lp.col_lb), lp.col_lb, -50.0)
    ub = np.where(np.isfinite(lp.col_ub), lp.col_ub, 50.0)
    trail = types.SimpleNamespace(lb=np.floor(lb), ub=np.ceil(ub))
    cols = [int(c) for c in np.argsort(-np.abs(star - np.round(star)))[:9]]
    lbs, ubs = cpsat.branch_lps(trail, star, cols)
    want = g.infeasible_rows(lbs, ubs, tolerance=1e-6)
    got = g.infeasible_rows_from(*cpsat.branch_overrides(trail, star, cols), tolerance=1e-6)
    bc.same_result(got, want, "branch_overrides")
    bc.same_result(want, bc.filter_reference(bc.ranges(_rows(lp), lbs, ubs),
                                             *_loaded_bounds(lp), 1e-6), "branch_lps")
    assert len(want[3]) == 18


def test_the_screen_is_sound_against_the_solver():
    """max x0 + x1 + x2 with x0 + x1 <= 1, x1 + x2 <= 1.5 and 0/1 bounds. The
    child with l0 = l1 = 1 is infeasible: the screen names the first row with
    g = 1 + 1 - 1, and the solver agrees; no child the solver finds optimal is
    reported."""
    lp = LinearProgram(m=2, n=3, col_starts=np.array([0, 1, 3, 4], np.int64),
                       row_idx=np.array([0, 0, 1, 1], np.int32), vals=np.ones(4),
                       col_lb=np.zeros(3), col_ub=np.ones(3), row_lb=np.full(2, -INF),
                       row_ub=np.array([1.0, 1.5]), obj=-np.ones(3))
    lbs = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 1], [0, 0, 1], [1, 0, 1]], np.float64)
    ubs = np.ones_like(lbs)
    ubs[4, 1] = 0.0
    p = abi.default_params(use_dual_simplex=1, max_number_of_iterations=1000)
    workers = [engine.LpHandle(p) for _ in range(2)]
    try:
        for w in workers:
            w.load(lp)
        assert workers[0].solve().problem_status == abi.OPTIMAL
        starts, rows, amounts, summaries = workers[0].infeasible_rows(lbs, ubs, tolerance=1e-6)
        both = 2  # the child with l0 = l1 = 1
        assert summaries["count"][both] >= 1 and summaries["worst"][both] == 1.0
        assert summaries["worst_row"][both] == 0
        assert list(rows[starts[both]:starts[both + 1]]) == [0]
        assert list(amounts[starts[both]:starts[both + 1]]) == [1.0]
        results = engine.batch_solve_bounds(workers, lbs, ubs, workers[0].state())
        assert all(r.error_code == 0 for r in results)
        assert results[both].problem_status in (abi.PRIMAL_INFEASIBLE, abi.DUAL_UNBOUNDED)
        optimal = [j for j, r in enumerate(results) if r.problem_status == abi.OPTIMAL]
        assert len(optimal) >= 3
        for j in optimal:
            assert summaries["count"][j] == 0, j
        # The child with l1 = l2 = 1 misses the second row by 1/2.
        assert summaries["count"][3] == 1 and summaries["worst"][3] == 0.5
        assert results[3].problem_status in (abi.PRIMAL_INFEASIBLE, abi.DUAL_UNBOUNDED)
    finally:
        for w in workers:
            w.close()
