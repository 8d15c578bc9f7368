"""mi_lp_bound_propagate(_from) / mi_lp_bound_propagated_columns_from /
mi_lp_get_propagated_columns (include/mi_lp.h) through mi_glop.engine.LpHandle
and through ctypes, on solved LPs of tests/lp_gen.py (the set-up of
tests/test_bound_implied_gpu.py).

The three forms equal, on every bit, the numpy reference of
tests/bound_propagate_cases.py on the same bound sets; every error of the
header's table is returned and leaves the outputs and the stored list alone;
k = 0; the state before a solve and after mi_lp_load; summaries only leaves the
stored list in place; the five stores of a handle do not see each other; R
rounds of tightened_columns_from fed back through cpsat.tightened_overrides
equal propagated_columns_from(max_rounds=R); cpsat.propagate_branches equals
the reference on the materialised branch LPs; and a handle that made the calls
solves on exactly as one that never did.
"""
import ctypes
import types

import numpy as np
import pytest

from mi_glop import abi, cpsat, engine
from mi_glop.lp import LinearProgram

import bound_implied_cases as ic
import bound_propagate_cases as pc
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
    assert hasattr(g, "propagate_bounds"), "LpHandle has no bound propagation"
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


def _node(lp, k, seed):
    """A node in the manner of bound_propagate_cases.node on an LP of lp_gen:
    a finite base box, the LP's own row bounds, k children that override a few
    columns. Returns (base_lb, base_ub, sets, row_lb, row_ub, is_integer)."""
    rng = np.random.default_rng(seed)
    is_integer = (np.arange(lp.n) % 3 == 0).astype(np.uint8)
    ints = is_integer != 0
    base_lb = np.floor(rng.normal(size=lp.n) * 2.0 - 3.0)
    base_ub = base_lb + rng.integers(2, 9, lp.n)
    x0 = 0.5 * (base_lb + base_ub)
    x0[ints] = np.round(x0[ints])
    row_lb, row_ub = np.array(lp.row_lb, np.float64), np.array(lp.row_ub, np.float64)
    sets = [(np.zeros(0, np.int32), np.zeros(0), np.zeros(0))]
    for j in range(1, k):
        cols = np.sort(rng.choice(lp.n, 1 + j % 3, replace=False)).astype(np.int32)
        if j % 2 == 0:
            sets.append((cols, np.ceil(x0[cols] - 0.5), np.floor(x0[cols] + 0.5)))
        else:
            sets.append((cols, np.ceil(x0[cols] + 0.6 * (base_ub[cols] - x0[cols])),
                         base_ub[cols].copy()))
    return base_lb, base_ub, sets[:k], row_lb, row_ub, is_integer


NODE, NODE_F = "steps", 0.05


@pytest.fixture(scope="module")
def node_handle():
    """bound_propagate_cases' node on `steps` as a solved LP: its matrix, its
    base box and its row bounds (feasible at the witness), no objective."""
    mat = ic.matrix(NODE)
    base_lb, base_ub, _, row_lb, row_ub = pc.node(NODE, NODE_F)
    lp = LinearProgram(m=mat.m, n=mat.n, col_starts=np.asarray(mat.col_starts, np.int64),
                       row_idx=np.asarray(mat.row_idx, np.int32),
                       vals=np.asarray(mat.vals, np.float64), col_lb=base_lb.copy(),
                       col_ub=base_ub.copy(), row_lb=row_lb.copy(), row_ub=row_ub.copy(),
                       obj=np.zeros(mat.n))
    g = engine.LpHandle(abi.default_params())
    g.load(lp)
    assert g.solve().problem_status == abi.OPTIMAL
    yield g
    g.close()


@pytest.mark.parametrize("k", [1, 3, 17])
def test_every_form_against_the_reference(node_handle, k):
    """The node cases of `steps` through LpHandle; the row bounds are the
    loaded ones, passed and left out."""
    g = node_handle
    base_lb, base_ub, sets, row_lb, row_ub = pc.node(NODE, NODE_F)
    sets = sets[:k]
    L, U = bc.materialise(base_lb, base_ub, sets)
    statuses = set()
    for f, tol, integers in pc.grid(NODE):
        if f != NODE_F:
            continue
        ints = pc.integer_columns(NODE) if integers else None
        for max_rounds in pc.ROUNDS:
            want = pc.expected(NODE, f, tol, integers, max_rounds, k)
            statuses |= set(want[2]["status"].tolist())
            what = f"k={k} tol={tol} R={max_rounds} ints={integers}"
            kw = dict(is_integer=ints, tolerance=tol, integrality_tolerance=pc.ITOL)
            if max_rounds == 3:
                kw.update(row_lb=row_lb, row_ub=row_ub)
            pc.same_result(g.propagate_bounds(L, U, max_rounds, **kw), want, what + " dense")
            pc.same_result(g.propagate_bounds_from(base_lb, base_ub, sets, max_rounds, **kw), want,
                           what + " overrides")
            lists = pc.list_result(want, base_lb, base_ub, tol)
            pc.same_lists(g.propagated_columns_from(base_lb, base_ub, sets, max_rounds, **kw),
                          lists, what + " lists")
            only = g.propagated_columns_from(base_lb, base_ub, sets, max_rounds, lists=False, **kw)
            assert only[:4] == (None, None, None, None)
            pc.same_summaries(only[4], lists[4], what + " summaries only")
    if k == 17:
        assert statuses == {pc.ROUND_LIMIT, pc.FIXPOINT, pc.INFEASIBLE}, statuses
    with pytest.raises(ValueError):
        g.propagate_bounds(L, U, 3, is_integer=np.zeros(len(base_lb) + 1))
    with pytest.raises(ValueError):
        g.propagate_bounds(np.zeros((2, len(base_lb) + 1)), np.zeros((2, len(base_lb) + 1)), 3)


def test_own_row_bounds(solved):
    """Row bounds of the caller's own on a random LP, infinite on either side."""
    g, lp = solved
    base_lb, base_ub, sets, rlb, rub, is_integer = _node(lp, 5, 317)
    L, U = bc.materialise(base_lb, base_ub, sets)
    lb = np.where(np.arange(lp.m) % 5 == 0, -INF, rlb)
    ub = np.where(np.arange(lp.m) % 7 == 1, INF, rub - 0.25)
    want = pc.propagate(_matrix(lp), L, U, lb, ub, is_integer, 0.0, pc.ITOL, 4)
    assert want[2]["moves"].min() > 0
    pc.same_result(g.propagate_bounds(L, U, 4, is_integer=is_integer, row_lb=lb, row_ub=ub,
                                      integrality_tolerance=pc.ITOL), want, "own row bounds")


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _dense(g, h, L, U, k, ints, lb, ub, tol, itol, rounds, lo, hi, s):
    return g._L.mi_lp_bound_propagate(h, _vp(L), _vp(U), k, _vp(ints), _vp(lb), _vp(ub), tol,
                                      itol, rounds, _vp(lo), _vp(hi), _vp(s))


def _dense_from(g, h, bl, bu, k, ov, ints, lb, ub, tol, itol, rounds, lo, hi, s):
    st, c, a, b = ov
    return g._L.mi_lp_bound_propagate_from(h, _vp(bl), _vp(bu), k, _vp(st), _vp(c), _vp(a),
                                           _vp(b), _vp(ints), _vp(lb), _vp(ub), tol, itol, rounds,
                                           _vp(lo), _vp(hi), _vp(s))


def _lists_from(g, h, bl, bu, k, ov, ints, lb, ub, tol, itol, rounds, starts, s):
    st, c, a, b = ov
    return g._L.mi_lp_bound_propagated_columns_from(
        h, _vp(bl), _vp(bu), k, _vp(st), _vp(c), _vp(a), _vp(b), _vp(ints), _vp(lb), _vp(ub), tol,
        itol, rounds, _vp(starts), _vp(s))


def _get(g, h, cols, lo, hi):
    return g._L.mi_lp_get_propagated_columns(h, _vp(cols), _vp(lo), _vp(hi))


class _Outputs:
    """Every output filled with a mark, and the stored list as it was;
    untouched() is true while none of them changed."""

    def __init__(self, g, k, n):
        self.g = g
        self.starts = np.full(k + 1, -9, np.int64)
        self.summaries = np.zeros(k, engine.PROPAGATION)
        self.summaries["rounds"] = -9
        self.lo, self.hi = np.full(k * n, -9.5), np.full(k * n, -9.5)
        self.stored = self._stored()

    def _stored(self):
        cols, lo, hi = np.full(4096, -9, np.int32), np.full(4096, -9.5), np.full(4096, -9.5)
        rc = _get(self.g, self.g.h, cols, lo, hi)
        return rc, cols.tobytes(), lo.tobytes(), hi.tobytes()

    def untouched(self):
        return (np.all(self.starts == -9) and np.all(self.summaries["rounds"] == -9) and
                np.all(self.lo == -9.5) and np.all(self.hi == -9.5) and
                self._stored() == self.stored)


def test_errors_write_nothing_and_keep_the_stored_list(solved):
    g, lp = solved
    n, m = lp.n, lp.m
    base_lb, base_ub, sets, lb, ub, ints = _node(lp, 2, 17)
    first = g.propagated_columns_from(base_lb, base_ub, sets, 5, row_lb=lb, row_ub=ub)
    assert 0 < first[0][2] < 4096
    L, U = (np.ascontiguousarray(a).reshape(-1) for a in bc.materialise(base_lb, base_ub, sets))
    o = _Outputs(g, 2, n)
    assert o.stored[0] == 0
    no_ov = (np.zeros(3, np.int64), None, None, None)

    def every(k, ov, ints, bl, bu, tol, itol, rounds, want):
        assert _dense(g, g.h, L, U, k, ints, bl, bu, tol, itol, rounds, o.lo, o.hi,
                      o.summaries) == want
        assert _dense_from(g, g.h, base_lb, base_ub, k, ov, ints, bl, bu, tol, itol, rounds, o.lo,
                           o.hi, o.summaries) == want
        assert _lists_from(g, g.h, base_lb, base_ub, k, ov, ints, bl, bu, tol, itol, rounds,
                           o.starts, o.summaries) == want
        assert o.untouched(), (k, tol, itol, rounds)

    def bad(r, upper):
        b = (ub if upper else lb).copy()
        b[r] = np.nan
        return (lb, b) if upper else (b, ub)

    # MI_LP_ERROR_INVALID_PROBLEM.
    for k, bl, bu, tol, itol, rounds in [
            (-1, lb, ub, 0.0, 0.0, 3), (2, lb, ub, -1e-9, 0.0, 3), (2, lb, ub, np.nan, 0.0, 3),
            (2, lb, ub, INF, 0.0, 3), (2, *bad(3, False), 0.0, 0.0, 3),
            (2, *bad(m - 1, True), 0.0, 0.0, 3),
            (2, lb, ub, 0.0, 0.0, 0), (2, lb, ub, 0.0, 0.0, -4),        # max_rounds < 1
            (2, lb, ub, 0.0, -1e-9, 3), (2, lb, ub, 0.0, np.nan, 3),   # integrality tolerance
            (2, lb, ub, 0.0, 0.5, 3), (2, lb, ub, 0.0, INF, 3)]:
        every(k, no_ov, ints, bl, bu, tol, itol, rounds, ERROR_INVALID_PROBLEM)
    i64, i32 = lambda a: np.array(a, np.int64), lambda a: np.array(a, np.int32)
    vals = np.ones(4)
    for starts, cols in [(i64([0, 2, 4]), i32([0, 1, 5, 5])),   # the same column twice in a set
                         (i64([0, 2, 4]), i32([0, n, 1, 2])),   # a slack column: out of range
                         (i64([0, 2, 4]), i32([0, 1, -1, 2])),
                         (i64([0, 3, 2]), i32([0, 1, 2, 3])),   # decreasing starts
                         (i64([1, 2, 4]), i32([0, 1, 2, 3]))]:  # starts[0] != 0
        ov = (starts, cols, vals, vals)
        assert _lists_from(g, g.h, base_lb, base_ub, 2, ov, ints, lb, ub, 0.0, 0.0, 3, o.starts,
                           o.summaries) == ERROR_INVALID_PROBLEM
        assert _dense_from(g, g.h, base_lb, base_ub, 2, ov, ints, lb, ub, 0.0, 0.0, 3, o.lo, o.hi,
                           o.summaries) == ERROR_INVALID_PROBLEM
        assert o.untouched(), starts
    # MI_LP_ERROR_NULL.
    ov = (i64([0, 1, 2]), i32([0, 1]), np.ones(2), np.ones(2))
    rest = (ints, lb, ub, 0.0, 0.0, 3)
    assert _dense(g, None, L, U, 2, *rest, o.lo, o.hi, o.summaries) == ERROR_NULL
    assert _dense(g, g.h, None, U, 2, *rest, o.lo, o.hi, o.summaries) == ERROR_NULL
    assert _dense(g, g.h, L, None, 2, *rest, o.lo, o.hi, o.summaries) == ERROR_NULL
    assert _dense(g, g.h, L, U, 2, *rest, None, o.hi, o.summaries) == ERROR_NULL
    assert _dense(g, g.h, L, U, 2, *rest, o.lo, None, o.summaries) == ERROR_NULL
    assert _dense_from(g, None, base_lb, base_ub, 2, ov, *rest, o.lo, o.hi,
                       o.summaries) == ERROR_NULL
    assert _dense_from(g, g.h, None, base_ub, 2, ov, *rest, o.lo, o.hi, o.summaries) == ERROR_NULL
    assert _dense_from(g, g.h, base_lb, base_ub, 2, ov, *rest, None, o.hi,
                       o.summaries) == ERROR_NULL
    assert _lists_from(g, None, base_lb, base_ub, 2, ov, *rest, o.starts,
                       o.summaries) == ERROR_NULL
    assert _lists_from(g, g.h, base_lb, None, 2, ov, *rest, o.starts, o.summaries) == ERROR_NULL
    assert _lists_from(g, g.h, base_lb, base_ub, 2, ov, *rest, None, None) == ERROR_NULL
    for missing in range(4):
        part = tuple(None if i == missing else a for i, a in enumerate(ov))
        assert _lists_from(g, g.h, base_lb, base_ub, 2, part, *rest, o.starts,
                           o.summaries) == ERROR_NULL
        assert _dense_from(g, g.h, base_lb, base_ub, 2, part, *rest, o.lo, o.hi,
                           o.summaries) == ERROR_NULL
    one = np.zeros(1)
    assert _get(g, None, np.zeros(1, np.int32), one, one) == ERROR_NULL
    assert _get(g, g.h, None, one, one) == ERROR_NULL
    assert _get(g, g.h, np.zeros(1, np.int32), None, one) == ERROR_NULL
    assert _get(g, g.h, np.zeros(1, np.int32), one, None) == ERROR_NULL
    assert o.untouched()
    # col_starts may be NULL (summaries only: the stored list stays), and the
    # summaries may be NULL.
    flat = bc.flatten(sets)
    flat = (flat[0], flat[1], flat[2], flat[3])
    assert _lists_from(g, g.h, base_lb, base_ub, 2, flat, None, lb, ub, 0.0, 0.0, 5, None,
                       o.summaries) == 0
    pc.same_summaries(o.summaries, first[4], "summaries only")
    assert o._stored() == o.stored
    assert _lists_from(g, g.h, base_lb, base_ub, 2, flat, None, lb, ub, 0.0, 0.0, 5, o.starts,
                       None) == 0
    assert np.array_equal(o.starts, first[0]) and o._stored() == o.stored
    assert _dense(g, g.h, L, U, 2, None, lb, ub, 0.0, 0.0, 5, o.lo, o.hi, None) == 0
    want = g.propagate_bounds(L.reshape(2, n), U.reshape(2, n), 5, row_lb=lb, row_ub=ub)
    assert np.array_equal(bits(o.lo), bits(want[0].reshape(-1)))
    # k = 0 of the dense calls succeeds and writes nothing.
    o = _Outputs(g, 2, n)
    assert _dense(g, g.h, L, U, 0, *rest, o.lo, o.hi, o.summaries) == 0 and o.untouched()


def test_error_state_and_k_zero():
    lp = lp_gen.random_sparse_lp(20, 50, 0.2, 8)
    g = engine.LpHandle(abi.default_params())
    g.load(lp)
    L, U = np.full(lp.n, -1.0), np.ones(lp.n)
    lb, ub = np.full(lp.m, -1.0), np.full(lp.m, 0.0)
    starts = np.full(2, -9, np.int64)
    s = np.zeros(1, engine.PROPAGATION)
    s["rounds"] = -9
    lo, hi = np.full(lp.n, -9.5), np.full(lp.n, -9.5)
    cols, a, b = np.zeros(64, np.int32), np.zeros(64), np.zeros(64)
    no_ov = (np.zeros(2, np.int64), None, None, None)
    rest = (None, lb, ub, 0.0, 0.0, 3)
    # Before a solve, and no list before any list-building call.
    assert _dense(g, g.h, L, U, 1, *rest, lo, hi, s) == ERROR_STATE
    assert _dense_from(g, g.h, L, U, 1, no_ov, *rest, lo, hi, s) == ERROR_STATE
    assert _lists_from(g, g.h, L, U, 1, no_ov, *rest, starts, s) == ERROR_STATE
    assert _get(g, g.h, cols, a, b) == ERROR_STATE
    assert np.all(starts == -9) and s["rounds"][0] == -9 and np.all(lo == -9.5)
    assert g.solve().problem_status == abi.OPTIMAL
    assert _get(g, g.h, cols, a, b) == ERROR_STATE
    assert _lists_from(g, g.h, L, U, 1, no_ov, *rest, None, s) == 0  # summaries only: no list
    assert _get(g, g.h, cols, a, b) == ERROR_STATE
    assert _lists_from(g, g.h, L, U, 1, no_ov, *rest, starts, s) == 0
    assert _get(g, g.h, cols, a, b) == 0
    # k = 0 succeeds, writes col_starts[0] = 0 and stores an empty list.
    starts[:] = -9
    assert _lists_from(g, g.h, L, U, 0, (np.zeros(1, np.int64), None, None, None), *rest, starts,
                       None) == 0 and starts[0] == 0
    cols[:] = -9
    assert _get(g, g.h, cols, a, b) == 0 and np.all(cols == -9)
    got = g.propagated_columns_from(L, U, [], 3, row_lb=lb, row_ub=ub)
    assert list(got[0]) == [0] and all(len(x) == 0 for x in got[1:])
    assert cpsat.tightened_overrides(got) == []
    dense = g.propagate_bounds(np.zeros((0, lp.n)), np.zeros((0, lp.n)), 3)
    assert dense[0].shape == dense[1].shape == (0, lp.n) and len(dense[2]) == 0
    # After mi_lp_load the list is gone.
    g.load(lp)
    assert _get(g, g.h, cols, a, b) == ERROR_STATE
    g.close()


def test_the_five_stores_are_separate(solved):
    g, lp = solved
    base_lb, base_ub, sets, lb, ub, ints = _node(lp, 5, 77)
    L, U = bc.materialise(base_lb, base_ub, sets)
    mine = g.propagated_columns_from(base_lb, base_ub, sets, 4, is_integer=ints, row_lb=lb,
                                     row_ub=ub)
    tightened = g.tightened_columns(L, U, lb, ub)
    infeasible = g.infeasible_rows(L, U, np.full(lp.m, INF), np.full(lp.m, -INF))
    x = np.tile(np.concatenate([g.primal(), -g.activities()]), (3, 1))
    x[:, ::2] += 1.0
    violated = g.column_violations(x, tolerance=1e-9)
    sparse = g.row_combinations_sparse(np.random.default_rng(5).normal(size=(3, lp.m)), 1e-9)
    assert min(len(r[1]) for r in (mine, tightened, infeasible, violated, sparse)) > 0

    def stored(call, want_idx, want_vals):
        idx, vals = np.zeros(len(want_idx) + 1, np.int32), np.zeros(len(want_idx) + 1)
        assert call(g.h, _vp(idx), _vp(vals)) == 0
        assert np.array_equal(idx[:-1], want_idx), call
        assert np.array_equal(bits(vals[:-1]), bits(want_vals)), call

    def columns_stored(call, want):
        kept = len(want[1])
        cols, lo, hi = np.zeros(kept + 1, np.int32), np.zeros(kept + 1), np.zeros(kept + 1)
        assert call(g.h, _vp(cols), _vp(lo), _vp(hi)) == 0
        assert np.array_equal(cols[:-1], want[1])
        assert np.array_equal(bits(lo[:-1]), bits(want[2]))
        assert np.array_equal(bits(hi[:-1]), bits(want[3]))

    def others():
        columns_stored(g._L.mi_lp_get_tightened_columns, tightened)
        stored(g._L.mi_lp_get_infeasible_rows, infeasible[1], infeasible[2])
        stored(g._L.mi_lp_get_violated_rows, violated[1], violated[2])
        stored(g._L.mi_lp_get_sparse_rows, sparse[1], sparse[2])

    # Each store still holds what its own call left, after the four others ran.
    columns_stored(g._L.mi_lp_get_propagated_columns, mine)
    others()
    # And a new list of this call disturbs none of the others.
    again = g.propagated_columns_from(base_lb, base_ub, sets[:2], 1, row_lb=lb, row_ub=ub)
    columns_stored(g._L.mi_lp_get_propagated_columns, again)
    others()
    g.propagate_bounds(L, U, 2, row_lb=lb, row_ub=ub)
    columns_stored(g._L.mi_lp_get_propagated_columns, again)


@pytest.mark.parametrize("rounds", [1, 2, 5])
def test_rounds_of_tightened_columns_fed_back(node_handle, rounds):
    """Without integers and at tolerance 0, R rounds of tightened_columns_from,
    each list fed back as the set's overrides, are propagated_columns_from with
    max_rounds = R on every set that the new call does not report INFEASIBLE
    before round R: lists and bounds, bit for bit."""
    g = node_handle
    k = pc.CHILDREN
    base_lb, base_ub, sets, lb, ub = pc.node(NODE, NODE_F)
    got = g.propagated_columns_from(base_lb, base_ub, sets, rounds)
    fed = sets
    for _ in range(rounds):
        result = g.tightened_columns_from(base_lb, base_ub, fed, tolerance=0.0)
        fed = cpsat.tightened_overrides(result)
    mine = cpsat.tightened_overrides(got)
    s = got[4]
    compared = [j for j in range(k)
                if not (s["status"][j] == pc.INFEASIBLE and s["rounds"][j] < rounds)]
    assert len(compared) >= k // 2 and (rounds == 1 or len(compared) < k)
    # A set at its fixpoint before round R repeats itself and is compared too;
    # every other compared set took part in all R rounds.
    assert all(s["rounds"][j] == rounds or s["status"][j] == pc.FIXPOINT for j in compared)
    assert any(s["rounds"][j] == rounds for j in compared)
    for j in compared:
        for a, b, part in zip(mine[j], fed[j], ("cols", "new_lbs", "new_ubs")):
            assert np.array_equal(a, b) if part == "cols" else \
                np.array_equal(bits(a), bits(b)), (rounds, j, part)
    FL, FU = bc.materialise(base_lb, base_ub, fed)
    NL, NU, _ = g.propagate_bounds_from(base_lb, base_ub, sets, rounds)
    ic.same_bounds((NL[compared], NU[compared]), (FL[compared], FU[compared]), f"R={rounds}")


def test_propagate_branches(solved):
    g, lp = solved
    base_lb, base_ub, _, lb, ub, ints = _node(lp, 1, 501)
    # The handle's loaded row bounds are the LP's: propagate_branches uses them.
    rlb, rub = np.array(lp.row_lb, np.float64), np.array(lp.row_ub, np.float64)
    trail = types.SimpleNamespace(lb=base_lb, ub=base_ub)
    x = 0.5 * (base_lb + base_ub) + 0.25
    cols = [3, 4, 10, 50, 51, 120, 199, 7, 8]
    int_cols = [c for c in range(lp.n) if ints[c]]
    overrides, summaries = cpsat.propagate_branches(g, trail, x, cols, int_cols, 6, 1e-9, pc.ITOL)
    L, U = cpsat.branch_lps(trail, x, cols)
    want = pc.propagate(_matrix(lp), L, U, rlb, rub, ints, 1e-9, pc.ITOL, 6)
    assert len(overrides) == 2 * len(cols) == len(summaries)
    ic.same_bounds(bc.materialise(base_lb, base_ub, overrides), want[:2], "propagate_branches")
    lists = pc.list_result(want, base_lb, base_ub, 1e-9)
    pc.same_summaries(summaries, lists[4], "propagate_branches")
    assert (summaries["moves"] > 0).any()


def test_a_later_solve_does_not_see_the_calls():
    """Two handles solve the same LP; one makes the calls in between; then
    both get the same tighter bounds and solve on from their bases."""
    g, lp = _solved(use_dual_simplex=1)
    q, _ = _solved(use_dual_simplex=1)
    try:
        base_lb, base_ub, sets, lb, ub, ints = _node(lp, 17, 95)
        L, U = bc.materialise(base_lb, base_ub, sets)
        g.propagate_bounds(L, U, 5, is_integer=ints, row_lb=lb, row_ub=ub)
        g.propagate_bounds_from(base_lb, base_ub, sets, 5, row_lb=lb, row_ub=ub, tolerance=1e-9)
        g.propagated_columns_from(base_lb, base_ub, sets, 5, is_integer=ints)
        g.propagated_columns_from(base_lb, base_ub, sets, 5, lists=False)
        star = q.primal()
        clb, cub = np.array(lp.col_lb), np.array(lp.col_ub)
        moved = [c for c in range(lp.n) if np.isfinite(clb[c]) and star[c] > clb[c] + 1e-3][:6]
        assert moved
        for c in moved:
            cub[c] = 0.5 * (clb[c] + star[c])
        results = []
        for h in (g, q):
            h.set_variable_bounds(clb, cub)
            results.append(h.solve())
        rg, rq = results
        assert rq.iterations > 0
        assert (rg.problem_status, rg.iterations) == (rq.problem_status, rq.iterations)
        assert bits(np.float64(rg.objective)) == bits(np.float64(rq.objective))
        assert np.array_equal(g.basis(), q.basis())
        assert np.array_equal(g.state(), q.state())
        assert np.array_equal(bits(g.primal()), bits(q.primal()))
        assert np.array_equal(bits(g.duals()), bits(q.duals()))
    finally:
        g.close()
        q.close()
