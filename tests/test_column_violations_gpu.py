"""mi_lp_column_combinations_violations / mi_lp_column_combinations_from_violations
/ mi_lp_get_violated_rows (include/mi_lp.h) through mi_glop.engine.LpHandle,
on solved LPs of tests/lp_gen.py (the set-up of
tests/test_column_combinations_gpu.py).

Both forms equal, on every bit, column_combinations of the same points
filtered in numpy with the header's rule (row_violation_cases.filter_reference);
NULL bounds mean the loaded ones; (k, n) input means zero slacks; every error
of the header's table is returned and leaves the outputs and the stored list
alone; the stored list and the sparse rows' store do not see each other; and a
handle that made the calls solves on exactly as one that never did.
"""
import ctypes

import numpy as np
import pytest

from mi_glop import abi, engine

import lp_gen
import row_violation_cases as vc
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
    g.load(lp)
    assert g.solve().problem_status == abi.OPTIMAL
    return g, lp


@pytest.fixture(scope="module")
def solved():
    g, lp = _solved()
    yield g, lp
    g.close()


def _points(lp, g, k, seed):
    """Roundings and neighbours of x*: the primal with its slacks set to minus
    the activities, columns rounded, zeroed or moved."""
    rng = np.random.default_rng(seed)
    star = np.concatenate([g.primal(), -g.activities()])
    x = np.tile(star, (k, 1))
    for j in range(k):
        cols = rng.permutation(lp.n + lp.m)[:1 + 3 * j]
        x[j, cols] = np.round(x[j, cols] + rng.normal(size=len(cols)))
    x[k - 1, :: 3] = 0.0
    return x


def _bounds(acts):
    """Per row the quartiles of the given activities: about half violated."""
    return np.quantile(acts, 0.25, axis=0), np.quantile(acts, 0.75, axis=0)


def _loaded_bounds(lp):
    return np.array(lp.row_lb, np.float64), np.array(lp.row_ub, np.float64)


@pytest.mark.parametrize("k", [1, 3, 17])
def test_dense_call_against_the_filtered_dense_result(solved, k):
    g, lp = solved
    x = _points(lp, g, k, 70 + k)
    acts = g.column_combinations(x)
    lb, ub = _bounds(g.column_combinations(_points(lp, g, 17, 87)))
    for tol in (0.0, 1e-6):
        want = vc.filter_reference(acts, lb, ub, tol)
        got = g.column_violations(x, lb, ub, tol)
        vc.same_result(got, want, f"k={k} tol={tol}")
        if k == 17 and tol > 0.0:
            # The points are neighbours of x*, so most activities are rounding
            # noise around 0: above the tolerance are the rows a moved column
            # reaches, and the early points move few columns.
            assert 0 < want[0][k] < k * lp.m
        only = g.column_violations(x, lb, ub, tol, lists=False)
        assert only[:3] == (None, None, None)
        vc.same_summaries(only[3], want[3], f"k={k} summaries only")
    # The loaded bounds, given or NULL, one at a time and both.
    rlb, rub = _loaded_bounds(lp)
    want = vc.filter_reference(acts, rlb, rub, 1e-9)
    for a, b in ((None, None), (rlb, None), (None, rub), (rlb, rub)):
        vc.same_result(g.column_violations(x, a, b, 1e-9), want, "loaded bounds")
    # (k, n) input: zero slacks, the plain A x.
    xs = x[:, :lp.n]
    padded = np.concatenate([xs, np.zeros((k, lp.m))], axis=1)
    want_s = vc.filter_reference(g.column_combinations(padded), lb, ub, 0.0)
    vc.same_result(g.column_violations(xs, lb, ub), want_s, "(k, n) input")
    vc.same_result(g.column_violations(padded, lb, ub), want_s, "(k, n+m) input, zero slacks")
    with pytest.raises(ValueError):
        g.column_violations(np.zeros((2, lp.n + 1)))
    with pytest.raises(ValueError):
        g.column_violations(x, row_lb=np.zeros(lp.m + 1))


def test_override_call_against_the_filtered_dense_result(solved):
    g, lp = solved
    N = lp.n + lp.m
    rng = np.random.default_rng(81)
    base = np.concatenate([g.primal(), -g.activities()])
    overrides = []
    for j in range(18):
        cols = rng.permutation(N)[:j % 5].astype(np.int32)
        overrides.append((cols, np.round(rng.normal(size=len(cols)) * 4.0)))
    overrides[3] = (np.array([N - 1, 0], np.int32), np.array([0.0, -0.0]))
    held = [c for c in range(lp.n) if lp.col_starts[c + 1] > lp.col_starts[c]][:2]
    overrides[5] = (np.array(held, np.int32), np.array([np.nan, -INF]))
    acts = g.column_combinations_from(base, overrides)
    finite = np.where(np.isfinite(acts), acts, 0.0)
    lb, ub = _bounds(finite)
    want = vc.filter_reference(acts, lb, ub, 1e-7)
    assert np.isnan(want[2]).any() and np.isinf(want[2]).any()
    got = g.column_violations_from(base, overrides, lb, ub, 1e-7)
    vc.same_result(got, want, "overrides")
    x = np.tile(base, (len(overrides), 1))
    for j, (cols, vals) in enumerate(overrides):
        x[j, cols] = vals
    vc.same_result(g.column_violations(x, lb, ub, 1e-7), got, "against the dense form")
    only = g.column_violations_from(base, overrides, lb, ub, 1e-7, lists=False)
    vc.same_summaries(only[3], want[3], "overrides, summaries only")
    empty = g.column_violations_from(base, [], lb, ub)
    assert list(empty[0]) == [0] and len(empty[1]) == len(empty[2]) == len(empty[3]) == 0


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _dense(g, h, x, k, lb, ub, tol, starts, summaries):
    return g._L.mi_lp_column_combinations_violations(h, _vp(x), k, _vp(lb), _vp(ub), tol,
                                                     _vp(starts), _vp(summaries))


def _from(g, h, base, k, ov, lb, ub, tol, starts, summaries):
    s, c, v = ov
    return g._L.mi_lp_column_combinations_from_violations(
        h, _vp(base), k, _vp(s), _vp(c), _vp(v), _vp(lb), _vp(ub), tol, _vp(starts),
        _vp(summaries))


def _get(g, h, rows, vals):
    return g._L.mi_lp_get_violated_rows(h, _vp(rows), _vp(vals))


class _Outputs:
    """row_starts and summaries filled with a mark, and the stored list as it
    was; untouched() is true while neither changed."""

    def __init__(self, g, k):
        self.g = g
        self.starts = np.full(k + 1, -9, np.int64)
        self.summaries = np.zeros(k, engine.POINT_VIOLATIONS)
        self.summaries["count"] = -9
        self.stored = self._stored()

    def _stored(self):
        rows, vals = np.full(4096, -9, np.int32), np.full(4096, -9.5)
        rc = _get(self.g, self.g.h, rows, vals)
        return rc, rows.tobytes(), vals.tobytes()

    def untouched(self):
        return (np.all(self.starts == -9) and np.all(self.summaries["count"] == -9) and
                self._stored() == self.stored)


def test_errors_write_nothing_and_keep_the_stored_list(solved):
    g, lp = solved
    N, m = lp.n + lp.m, lp.m
    x = np.ones(2 * N)
    lb, ub = np.full(m, -1.0), np.full(m, 1.0)
    # A stored list to watch.
    first = g.column_violations(x.reshape(2, N), lb, ub)
    assert 0 < first[0][2] < 4096
    o = _Outputs(g, 2)
    assert o.stored[0] == 0
    no_ov = (np.zeros(3, np.int64), None, None)

    def bad_bounds(r, value, upper):
        b = (ub if upper else lb).copy()
        b[r] = value
        return (lb, b) if upper else (b, ub)

    # MI_LP_ERROR_INVALID_PROBLEM.
    for k, bl, bu, tol in [(-1, lb, ub, 0.0), (2, lb, ub, -1e-9), (2, lb, ub, np.nan),
                           (2, lb, ub, INF), (2, *bad_bounds(3, np.nan, False), 0.0),
                           (2, *bad_bounds(m - 1, np.nan, True), 0.0),
                           (2, *bad_bounds(0, INF, False), 0.0),
                           (2, *bad_bounds(5, -INF, True), 0.0)]:
        assert _dense(g, g.h, x, k, bl, bu, tol, o.starts, o.summaries) == ERROR_INVALID_PROBLEM
        assert _from(g, g.h, x, k, no_ov, bl, bu, tol, o.starts,
                     o.summaries) == ERROR_INVALID_PROBLEM
        assert o.untouched(), (k, tol)
    i64, i32 = lambda a: np.array(a, np.int64), lambda a: np.array(a, np.int32)
    vals = np.ones(4)
    for starts, cols in [(i64([0, 2, 4]), i32([0, 1, 5, 5])),   # the same column twice in a point
                         (i64([0, 2, 4]), i32([0, N, 1, 2])),   # a column out of range
                         (i64([0, 2, 4]), i32([0, 1, -1, 2])),
                         (i64([0, 3, 2]), i32([0, 1, 2, 3])),   # decreasing starts
                         (i64([1, 2, 4]), i32([0, 1, 2, 3]))]:  # starts[0] != 0
        assert _from(g, g.h, x, 2, (starts, cols, vals), lb, ub, 0.0, o.starts,
                     o.summaries) == ERROR_INVALID_PROBLEM
        assert o.untouched(), starts
    # lb > ub is allowed: every row is violated.
    crossed = g.column_violations(x.reshape(2, N), ub, lb)
    assert crossed[0][2] == 2 * m
    g.column_violations(x.reshape(2, N), lb, ub)  # the watched list again
    # MI_LP_ERROR_NULL.
    ov = (i64([0, 1, 2]), i32([0, 1]), np.ones(2))
    assert _dense(g, None, x, 2, lb, ub, 0.0, o.starts, o.summaries) == ERROR_NULL
    assert _dense(g, g.h, None, 2, lb, ub, 0.0, o.starts, o.summaries) == ERROR_NULL
    assert _dense(g, g.h, x, 2, lb, ub, 0.0, None, None) == ERROR_NULL
    assert _from(g, None, x, 2, ov, lb, ub, 0.0, o.starts, o.summaries) == ERROR_NULL
    assert _from(g, g.h, None, 2, ov, lb, ub, 0.0, o.starts, o.summaries) == ERROR_NULL
    assert _from(g, g.h, x, 2, (None, ov[1], ov[2]), lb, ub, 0.0, o.starts,
                 o.summaries) == ERROR_NULL
    assert _from(g, g.h, x, 2, (ov[0], None, ov[2]), lb, ub, 0.0, o.starts,
                 o.summaries) == ERROR_NULL
    assert _from(g, g.h, x, 2, (ov[0], ov[1], None), lb, ub, 0.0, o.starts,
                 o.summaries) == ERROR_NULL
    assert _from(g, g.h, x, 2, ov, lb, ub, 0.0, None, None) == ERROR_NULL
    assert _get(g, None, np.zeros(1, np.int32), np.zeros(1)) == ERROR_NULL
    assert _get(g, g.h, None, np.zeros(1)) == ERROR_NULL
    assert _get(g, g.h, np.zeros(1, np.int32), None) == ERROR_NULL
    assert o.untouched()
    # Summaries may be NULL, and row_starts may be NULL (summaries only: the
    # stored list stays).
    assert _dense(g, g.h, x, 2, lb, ub, 0.0, None, o.summaries) == 0
    assert np.array_equal(o.summaries["count"], first[3]["count"])
    assert o._stored() == o.stored
    assert _dense(g, g.h, x, 2, lb, ub, 0.0, o.starts, None) == 0
    assert np.array_equal(o.starts, first[0]) and o._stored() == o.stored


def test_error_state():
    lp = lp_gen.random_sparse_lp(20, 50, 0.2, 8)
    g = engine.LpHandle(abi.default_params())
    g.load(lp)
    N = lp.n + lp.m
    x, lb, ub = np.zeros(N), np.full(lp.m, -1.0), np.full(lp.m, 1.0)
    starts = np.full(2, -9, np.int64)
    summaries = np.zeros(1, engine.POINT_VIOLATIONS)
    summaries["count"] = -9
    rows, vals = np.zeros(64, np.int32), np.zeros(64)
    no_ov = (np.zeros(2, np.int64), None, None)
    # Before a solve, and no list before any list-building call.
    assert _dense(g, g.h, x, 1, lb, ub, 0.0, starts, summaries) == ERROR_STATE
    assert _from(g, g.h, x, 1, no_ov, lb, ub, 0.0, starts, summaries) == ERROR_STATE
    assert _get(g, g.h, rows, vals) == ERROR_STATE
    assert np.all(starts == -9) and summaries["count"][0] == -9
    assert g.solve().problem_status == abi.OPTIMAL
    assert _get(g, g.h, rows, vals) == ERROR_STATE
    assert _dense(g, g.h, x, 1, lb, ub, 0.0, None, summaries) == 0  # summaries only: no list
    assert _get(g, g.h, rows, vals) == ERROR_STATE
    assert _dense(g, g.h, x, 1, lb, ub, 0.0, starts, summaries) == 0
    assert _get(g, g.h, rows, vals) == 0
    # After mi_lp_load the list is gone.
    g.load(lp)
    assert _get(g, g.h, rows, vals) == ERROR_STATE
    g.close()


def test_k_zero_is_ok_and_stores_an_empty_list(solved):
    g, lp = solved
    N = lp.n + lp.m
    x, lb, ub = np.ones(N), np.full(lp.m, -1.0), np.full(lp.m, 1.0)
    assert g.column_violations(x, lb, ub)[0][1] > 0  # a non-empty list first
    starts = np.full(1, -9, np.int64)
    rows, vals = np.full(8, -9, np.int32), np.full(8, -9.5)
    assert _dense(g, g.h, x, 0, lb, ub, 0.0, starts, None) == 0
    assert starts[0] == 0
    assert _get(g, g.h, rows, vals) == 0 and np.all(rows == -9) and np.all(vals == -9.5)
    starts[0] = -9
    assert _from(g, g.h, x, 0, (np.zeros(1, np.int64), None, None), lb, ub, 0.0, starts,
                 None) == 0
    assert starts[0] == 0
    got = g.column_violations(np.zeros((0, N)), lb, ub)
    assert list(got[0]) == [0] and len(got[1]) == len(got[2]) == len(got[3]) == 0


def test_the_sparse_rows_store_is_separate(solved):
    g, lp = solved
    N = lp.n + lp.m
    x = _points(lp, g, 5, 77)
    lb, ub = _bounds(g.column_combinations(x))
    want = g.column_violations(x, lb, ub)
    y = np.random.default_rng(5).normal(size=(3, lp.m))
    sparse = g.row_combinations_sparse(y, 1e-9)
    # The violated rows are still the ones stored before the sparse call.
    rows, vals = np.zeros(len(want[1]) + 1, np.int32), np.zeros(len(want[1]) + 1)
    assert _get(g, g.h, rows, vals) == 0
    assert np.array_equal(rows[:-1], want[1]) and np.array_equal(bits(vals[:-1]), bits(want[2]))
    # And the sparse rows survive a violations call.
    g.column_violations(x[:2], lb, ub)
    cols, svals = np.zeros(len(sparse[1]) + 1, np.int32), np.zeros(len(sparse[1]) + 1)
    assert g._L.mi_lp_get_sparse_rows(g.h, _vp(cols), _vp(svals)) == 0
    assert np.array_equal(cols[:-1], sparse[1]) and np.array_equal(bits(svals[:-1]),
                                                                   bits(sparse[2]))
    assert N > 0


@pytest.mark.parametrize("dual", [0, 1])
def test_a_later_solve_does_not_see_the_calls(dual):
    """Two handles solve the same LP; one asks for violations in between; then
    both get the same tighter bounds and solve on from their bases."""
    g, lp = _solved(use_dual_simplex=dual)
    q, _ = _solved(use_dual_simplex=dual)
    try:
        x = _points(lp, g, 17, 95)
        g.column_violations(x, tolerance=1e-9)
        g.column_violations(x, lists=False)
        g.column_violations_from(x[0], [(np.array([0, 3], np.int32), np.array([1.0, 0.0]))] * 5)
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
