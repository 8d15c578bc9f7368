"""mi_lp_add_rows (include/mi_lp.h) through mi_glop.engine.LpHandle: in
everything a handle later returns, appending rows is the load of the extended
LP.

Nodes are the job-shop relaxations ft06 and random_6_4_7 under the dual
simplex. Handle A appends with add_rows, handle B loads lp.with_rows(...), the
CPU oracle loads the same. The cuts of a round are the Gomory cuts of the
oracle's fractional basic integer columns (tests/gomory_cases.py
node_reference, zero tolerance 1e-9, drop tolerance 1e-12) with
rhs = 1 + fsum(c . x*).

  1. a three-round cut loop: A, B and the oracle agree after every round in
     status, iterations, objective bits, primal, duals, reduced costs, basis
     and state, and the warm re-solve takes fewer iterations than a fresh
     handle solving the same extended LP from scratch;
  2. after add_rows and a solve, the panel calls equal B's bit for bit;
  3. add_rows before the first solve, add_rows then set_variable_bounds,
     add_rows then the load of a different LP, and k = 0 equal their load
     twins;
  4. the header's error table, each error leaving the next solve that of an
     untouched twin;
  5. MILP_SHARDS=2 takes path 2 with equal results;
  6. batch_solve_bounds over workers that appended equals workers that loaded;
  7. cpsat.add_cuts on the engine equals a test-side adapter on the oracle.
"""
import ctypes
import math

import numpy as np
import pytest

from mi_glop import abi, cpsat, engine

import gomory_cases as gc
import jobshop
import oracle_lib
import parity_util
from device_ref import bits

pytestmark = pytest.mark.gpu

ERROR_NULL, ERROR_INVALID_PROBLEM, ERROR_STATE, ERROR_DEVICE = 3, 4, 101, 100
NODES = ("ft06", "random_6_4_7")
ZERO_TOLERANCE, DROP_TOLERANCE = 1e-9, 1e-12

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


def params():
    return abi.default_params(use_dual_simplex=1, max_number_of_iterations=1000)


def node_lp(name):
    jobs = jobshop.FT06 if name == "ft06" else jobshop.random_instance(6, 4, 7)
    lp, ycols = jobshop.relaxation(jobs)
    unit = np.zeros(lp.n)
    unit[ycols] = 1.0
    return lp, list(ycols), unit


def round_cuts(o, lp, ycols, unit):
    """add_rows' arguments for the cuts of the node the oracle `o` has solved."""
    x = np.asarray(o.primal())
    state = np.asarray(o.state())
    f = x[ycols] - np.floor(x[ycols])
    cols = [int(c) for c, fc in zip(ycols, f) if 1e-6 < fc < 1 - 1e-6 and state[c] == gc.BASIC]
    (starts, kept, vals, summaries), _ = gc.node_reference(o, lp, cols, unit, ZERO_TOLERANCE,
                                                           DROP_TOLERANCE)
    cuts = []
    for j in range(len(cols)):
        if summaries["bad_count"][j] > 0 or summaries["count"][j] == 0:
            continue
        idx = np.asarray(kept[starts[j]:starts[j + 1]], np.int64)
        coefs = np.asarray(vals[starts[j]:starts[j + 1]], np.float64)
        cuts.append({"cols": idx, "coefs": coefs, "rhs": 1.0 + math.fsum(coefs * x[idx])})
    assert cuts, "a round without cuts"
    return cpsat.cut_rows(cuts)


def same_solution(a, ra, b, rb):
    assert (ra.error_code, ra.problem_status, ra.iterations) == \
        (rb.error_code, rb.problem_status, rb.iterations)
    assert bits(np.float64(ra.objective)) == bits(np.float64(rb.objective))
    for get in ("primal", "duals", "reduced_costs"):
        assert np.array_equal(bits(np.asarray(getattr(a, get)())),
                              bits(np.asarray(getattr(b, get)()))), get
    assert np.array_equal(a.basis(), b.basis()) and np.array_equal(a.state(), b.state())


def solved_pair(lp):
    """Two engine handles that loaded and solved lp."""
    out = []
    for _ in range(2):
        h = engine.LpHandle(params())
        h.load(lp)
        out += [h, h.solve()]
    same_solution(*out)
    return out[0], out[2]


@pytest.mark.parametrize("name", NODES)
def test_cut_loop_equals_reloads_and_the_oracle_and_stays_warm(name):
    lp, ycols, unit = node_lp(name)
    o, ro, a, ra = parity_util.solve_both(lp, params(), lambda q: engine.LpHandle(q))
    parity_util.compare(o, ro, a, ra, lp)
    b = engine.LpHandle(params())
    b.load(lp)
    same_solution(a, ra, b, b.solve())
    for rnd in range(3):
        rows = round_cuts(o, lp, ycols, unit)
        k, e = len(rows[0]) - 1, int(rows[0][-1])
        info = a.add_rows(*rows)
        assert info == {"path": 1, "rows": k, "entries": e, "bytes_up": info["bytes_up"]}
        assert 0 < info["bytes_up"] <= 24 * (e + k) + 16 * (k + 1) + 64
        lp = lp.with_rows(*rows)
        assert a.lp.m == lp.m and np.array_equal(a.lp.row_idx, lp.row_idx)
        b.load(lp)
        o.load(lp)
        ra, rb, ro = a.solve(), b.solve(), o.solve()
        assert ra.problem_status == abi.OPTIMAL, (rnd, ra.problem_status)
        same_solution(a, ra, b, rb)
        parity_util.compare(o, ro, a, ra, lp)
        assert bits(np.float64(ra.objective)) == bits(np.float64(ro.objective))
        fresh = engine.LpHandle(params())
        fresh.load(lp)
        rf = fresh.solve()
        assert rf.problem_status == abi.OPTIMAL
        assert ra.iterations < rf.iterations, (rnd, ra.iterations, rf.iterations)
        fresh.close()
    a.close()
    b.close()


@pytest.fixture(scope="module")
def appended():
    """ft06 with one round of cuts: (lp, unit, ycols, A appended and solved,
    B loaded and solved)."""
    lp, ycols, unit = node_lp("ft06")
    o = oracle_lib.OracleLp(params())
    o.load(lp)
    o.solve()
    rows = round_cuts(o, lp, ycols, unit)
    a, b = solved_pair(lp)
    a.add_rows(*rows)
    ext = lp.with_rows(*rows)
    b.load(ext)
    same_solution(a, a.solve(), b, b.solve())
    yield ext, unit, ycols, a, b, lp, rows
    a.close()
    b.close()


def test_panel_calls_after_an_append_equal_the_reloads(appended):
    lp, unit, ycols, a, b, _, _ = appended
    rng = np.random.default_rng(3)
    rows = [0, lp.m - 1, lp.m // 2, 5]
    x = rng.uniform(-1.0, 1.0, (3, lp.n + lp.m))
    c0 = ycols[0]  # one child per side of a branch on the first integer column, and the node
    overrides = [([c0], [lp.col_lb[c0]], [lp.col_lb[c0]]), ([c0], [lp.col_ub[c0]], [lp.col_ub[c0]]),
                 ([], [], [])]
    state = np.asarray(a.state())
    xa = np.asarray(a.primal())
    f = xa[ycols] - np.floor(xa[ycols])
    cols = [int(c) for c, fc in zip(ycols, f) if 1e-6 < fc < 1 - 1e-6 and state[c] == gc.BASIC]
    assert cols

    def flat(result):
        items = result if isinstance(result, (tuple, list)) else (result,)
        return [np.asarray(r) for r in items if r is not None]

    calls = {
        "tableau_rows": lambda h: h.tableau_rows(rows, True),
        "column_combinations": lambda h: h.column_combinations(x),
        "bound_activity_ranges_from": lambda h: h.bound_activity_ranges_from(
            lp.col_lb, lp.col_ub, overrides),
        "implied_bounds_from": lambda h: h.implied_bounds_from(
            lp.col_lb, lp.col_ub, overrides, lp.row_lb, lp.row_ub),
        "gomory_cuts": lambda h: h.gomory_cuts(cols, unit, ZERO_TOLERANCE, DROP_TOLERANCE),
    }
    for what, call in calls.items():
        got, want = flat(call(a)), flat(call(b))
        assert len(got) == len(want) > 0, what
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), what


def test_sequences_equal_their_load_twins(appended):
    _, _, _, _, _, lp, rows = appended
    ext = lp.with_rows(*rows)
    # Before the first solve: no device matrix yet.
    a, b = engine.LpHandle(params()), engine.LpHandle(params())
    a.load(lp)
    assert a.add_rows(*rows)["path"] == 0
    b.load(ext)
    same_solution(a, a.solve(), b, b.solve())
    # Then bounds, then a solve.
    lb, ub = np.array(lp.col_lb), np.array(lp.col_ub)
    ub[:3] = np.minimum(ub[:3], lb[:3] + 1.0)
    more = (np.array([0, 2]), np.array([0, 1]), np.array([1.0, 1.0]), np.array([-np.inf]),
            np.array([1e6]))
    assert a.add_rows(*more)["path"] == 1
    a.set_variable_bounds(lb, ub)
    b.load(ext.with_rows(*more))
    b.set_variable_bounds(lb, ub)
    same_solution(a, a.solve(), b, b.solve())
    # An append, then the load of a different LP (here: the LP without any cut).
    a.add_rows(*more)
    b.load(a.lp)
    a.load(lp)
    b.load(lp)
    same_solution(a, a.solve(), b, b.solve())
    # k = 0 is the load of the same LP: getters are refused until the next solve.
    none = (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0), np.zeros(0), np.zeros(0))
    info = a.add_rows(*none)
    assert (info["rows"], info["entries"]) == (0, 0) and a.lp.m == lp.m
    out = np.zeros(lp.n)
    assert a._L.mi_lp_get_primal(a.h, out.ctypes.data_as(ctypes.c_void_p)) == ERROR_STATE
    b.load(lp)
    same_solution(a, a.solve(), b, b.solve())
    a.close()
    b.close()


def _raw(h, k, starts, cols, vals, lb, ub):
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    return h._L.mi_lp_add_rows(h.h, k, p(starts), p(cols), p(vals), p(lb), p(ub), None)


def test_error_table_changes_nothing():
    lp, _, _ = node_lp("random_6_4_7")
    a, b = solved_pair(lp)
    i64, i32, f64 = np.int64, np.int32, np.float64
    starts = np.array([0, 2], i64)
    cols, vals = np.array([1, 4], i32), np.array([1.0, -2.0])
    lb, ub = np.array([0.0]), np.array([np.inf])
    nan, inf = np.nan, np.inf
    fresh = engine.LpHandle(params())
    assert _raw(fresh, 1, starts, cols, vals, lb, ub) == ERROR_STATE  # before a load
    fresh.close()
    assert a._L.mi_lp_add_rows(None, 1, None, None, None, None, None, None) == ERROR_NULL
    table = [
        (ERROR_NULL, (1, None, cols, vals, lb, ub)),
        (ERROR_NULL, (1, starts, None, vals, lb, ub)),
        (ERROR_NULL, (1, starts, cols, None, lb, ub)),
        (ERROR_NULL, (1, starts, cols, vals, None, ub)),
        (ERROR_NULL, (1, starts, cols, vals, lb, None)),
        (ERROR_INVALID_PROBLEM, (-1, starts, cols, vals, lb, ub)),
        (ERROR_INVALID_PROBLEM, (1, np.array([1, 2], i64), cols, vals, lb, ub)),
        (ERROR_INVALID_PROBLEM, (2, np.array([0, 2, 1], i64), cols, vals, np.zeros(2),
                                 np.ones(2))),
        (ERROR_INVALID_PROBLEM, (1, starts, np.array([1, lp.n], i32), vals, lb, ub)),
        (ERROR_INVALID_PROBLEM, (1, starts, np.array([-1, 4], i32), vals, lb, ub)),
        (ERROR_INVALID_PROBLEM, (1, starts, np.array([4, 1], i32), vals, lb, ub)),
        (ERROR_INVALID_PROBLEM, (1, starts, np.array([4, 4], i32), vals, lb, ub)),
        (ERROR_INVALID_PROBLEM, (1, starts, cols, np.array([1.0, 0.0]), lb, ub)),
        (ERROR_INVALID_PROBLEM, (1, starts, cols, np.array([nan, 1.0]), lb, ub)),
        (ERROR_INVALID_PROBLEM, (1, starts, cols, np.array([1.0, inf]), lb, ub)),
        (ERROR_INVALID_PROBLEM, (1, starts, cols, vals, np.array([nan]), ub)),
        (ERROR_INVALID_PROBLEM, (1, starts, cols, vals, lb, np.array([nan]))),
    ]
    for i, (code, args) in enumerate(table):
        assert _raw(a, *args) == code, i
    # Nothing changed: the getters still answer, and the next solve is the twin's.
    assert np.array_equal(bits(np.asarray(a.primal())), bits(np.asarray(b.primal())))
    assert a.lp.m == lp.m
    same_solution(a, a.solve(), b, b.solve())
    a.close()
    b.close()


def test_column_shards_take_the_full_upload(appended, monkeypatch):
    ext, _, _, _, _, lp, rows = appended
    monkeypatch.setenv("MILP_SHARDS", "2")
    s, t = solved_pair(lp)
    assert s.add_rows(*rows)["path"] == 2
    t.load(ext)
    rs, rt = s.solve(), t.solve()
    assert rs.problem_status == abi.OPTIMAL
    same_solution(s, rs, t, rt)
    s.close()
    t.close()


def test_batch_solve_bounds_over_appended_workers(appended):
    ext, _, _, solved, _, lp, rows = appended
    # Every child starts from the extended node's state, whichever worker takes it.
    warm = np.asarray(solved.state(), np.int8)
    workers = {"appended": [], "loaded": []}
    for _ in range(2):
        a, b = solved_pair(lp)
        a.add_rows(*rows)
        b.load(ext)
        workers["appended"].append(a)
        workers["loaded"].append(b)
    rng = np.random.default_rng(5)
    count = 6
    lbs = np.tile(ext.col_lb, (count, 1))
    ubs = np.tile(ext.col_ub, (count, 1))
    for i in range(count):
        c = rng.integers(0, ext.n)
        ubs[i, c] = min(ubs[i, c], lbs[i, c] + 1.0)
    out = {key: engine.batch_solve_bounds(w, lbs, ubs, warm) for key, w in workers.items()}
    for ra, rb in zip(out["appended"], out["loaded"]):
        assert (ra.error_code, ra.problem_status, ra.iterations) == \
            (rb.error_code, rb.problem_status, rb.iterations)
        assert bits(np.float64(ra.objective)) == bits(np.float64(rb.objective))
    for w in workers["appended"] + workers["loaded"]:
        w.close()


class OracleWithCuts(oracle_lib.OracleLp):
    """The oracle handle with the two calls it lacks: the cuts served by the
    numpy reference, the append by a load of the extended LP."""

    def gomory_cuts(self, cols, unit, zero_tolerance=0.0, drop_tolerance=0.0):
        return gc.node_reference(self, self.lp, cols, unit, zero_tolerance, drop_tolerance)[0]

    def add_rows(self, row_starts, cols, vals, row_lb, row_ub):
        # LpConstraint.solve_lp has told the solver that the matrix stays.
        self.notify_matrix_changed()
        self.load(self.lp.with_rows(row_starts, cols, vals, row_lb, row_ub))
        return None


def test_cpsat_add_cuts_on_the_oracle_and_on_the_engine():
    lp, ycols = jobshop.relaxation(jobshop.random_instance(6, 4, 7))
    out = []
    for handle in (OracleWithCuts(params()), engine.LpHandle(params())):
        c = cpsat.LpConstraint(lp, ycols, handle)
        t = cpsat.IntegerTrail(lp.col_lb, lp.col_ub)
        assert c.solve_lp(t) and c.analyze_lp(t)
        first = c.last.iterations
        cols = cpsat.fractional_columns(c.lp_solution, ycols, limit=20)
        cuts = cpsat.gomory_cuts(c, c.lp_solution, cols)
        info = cpsat.add_cuts(c, cuts)
        assert c.lp.m == lp.m + len(cuts) and c.lp is c.lp_data
        assert c.solve_lp(t)
        out.append((len(cuts), c.last.problem_status, c.last.iterations,
                    np.asarray(c.lp_solution, np.float64), info, first))
    (ko, so, io, xo, _, _), (kg, sg, ig, xg, info, _) = out
    assert (ko, so, io) == (kg, sg, ig) and ko > 0
    assert np.array_equal(bits(xo), bits(xg))
    assert info["path"] == 1 and info["rows"] == kg
