"""mi_lp_gomory_cuts / mi_lp_row_gomory_cuts / mi_lp_get_cut_rows
(include/mi_lp.h) through mi_glop.engine.LpHandle, on the branch-and-bound
nodes of tests/test_branching_penalties_gpu.py (the root LPs of job-shop
relaxations) and on a variant whose integer columns are scaled by powers of
two, so that the integer steps are not 1.

The cuts are pinned by Glop's public surface and the rule alone: the oracle's
GetUnitRowLeftInverse, statuses and primal values feed the numpy reference
(tests/gomory_cases.py node_reference). The engine's lists and summaries equal
it in every bit and index; they equal the composition of two dense
row_combinations calls on the GPU with the numpy rule; row_gomory_cuts gives
the same from the same inputs; the stored lists outlive a summaries-only call;
every error of the header's table is returned with nothing written; column
shards are refused before any device work; and cpsat.gomory_cuts gives the
same cuts on the engine as on the oracle. tests/test_gomory_ref_cpu.py checks
that the rule's cuts are valid.
"""
import ctypes
import math

import numpy as np
import pytest

from mi_glop import abi, cpsat, engine
from mi_glop.lp import LinearProgram

import gomory_cases as gc
import jobshop
import oracle_lib
import parity_util
import penalty_cases as pn
from device_ref import bits

pytestmark = pytest.mark.gpu

ERROR_NULL, ERROR_INVALID_PROBLEM, ERROR_STATE, ERROR_DEVICE = 3, 4, 101, 100
NODES = ("ft06", "random_6_4_7", "random_6_4_7_scaled")
ZERO_TOLERANCE = cpsat.PENALTY_PIVOT_TOLERANCE

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
    """(lp, integer columns, unit): the relaxation, and in the scaled variant
    integer column j replaced by 2^e_j times itself (e_j in -2 .. 2): its
    entries and cost divided, its bounds multiplied, its integer step 2^e_j."""
    if name == "ft06":
        lp, ycols = jobshop.relaxation(jobshop.FT06)
    else:
        lp, ycols = jobshop.relaxation(jobshop.random_instance(6, 4, 7))
    unit = np.zeros(lp.n)
    unit[ycols] = 1.0
    if name.endswith("_scaled"):
        rng = np.random.default_rng(21)
        unit[ycols] = np.ldexp(1.0, rng.integers(-2, 3, len(ycols)))
        scale = np.where(unit > 0, unit, 1.0)
        per_entry = np.repeat(scale, np.diff(lp.col_starts))
        lp = LinearProgram(lp.m, lp.n, lp.col_starts, lp.row_idx, np.asarray(lp.vals) / per_entry,
                           np.asarray(lp.col_lb) * scale, np.asarray(lp.col_ub) * scale,
                           lp.row_lb, lp.row_ub, np.asarray(lp.obj) / scale, lp.obj_offset,
                           lp.obj_scale, lp.maximize, lp.name + "_scaled")
    return lp, list(ycols), unit


def fractional(x, ycols, unit, state):
    t = np.asarray(x)[ycols] / unit[ycols]
    f = t - np.floor(t)
    return [int(c) for c, fc in zip(ycols, f) if 1e-6 < fc < 1 - 1e-6 and state[c] == gc.BASIC]


def same_summaries(got, want, what):
    assert got.dtype == engine.CUT_SUMMARY and got.shape == want.shape, (what, got.shape)
    for f in ("max_abs", "min_abs"):
        assert np.array_equal(bits(got[f]), bits(want[f])), (what, f, got[f], want[f])
    for f in ("count", "bad_count", "max_col", "min_col"):
        assert np.array_equal(got[f], want[f]), (what, f, got[f], want[f])


def same_cuts(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "row_starts", got[0], want[0])
    assert np.array_equal(got[1], want[1]), (what, "columns")
    assert np.array_equal(bits(got[2]), bits(want[2])), (what, "coefficients")
    same_summaries(got[3], want[3], what)


@pytest.fixture(scope="module", params=NODES)
def node(request):
    """(lp, unit, oracle, engine handle, fractional integer columns): the
    node solved by both, with equal results."""
    lp, ycols, unit = node_lp(request.param)
    o, ro, g, rg = parity_util.solve_both(lp, params(), lambda q: engine.LpHandle(q))
    parity_util.compare(o, ro, g, rg, lp)
    assert rg.problem_status == abi.OPTIMAL
    assert np.array_equal(bits(np.asarray(g.primal())), bits(np.asarray(o.primal())))
    cols = fractional(o.primal(), ycols, unit, np.asarray(o.state()))
    assert len(cols) > 16, "more than one panel of cuts"
    yield lp, unit, o, g, cols
    g.close()


def test_gomory_cuts_equal_the_reference_fed_from_the_oracle(node):
    lp, unit, o, g, cols = node
    want, _ = gc.node_reference(o, lp, cols, unit, ZERO_TOLERANCE, 0.0)
    assert (want[3]["count"] > 0).all() and want[0][-1] > len(cols)
    same_cuts(g.gomory_cuts(cols, unit, ZERO_TOLERANCE, 0.0), want, "all columns")
    for k in (1, 4, 16, 17):
        same_cuts(g.gomory_cuts(cols[:k], unit, ZERO_TOLERANCE, 0.0),
                  gc.node_reference(o, lp, cols[:k], unit, ZERO_TOLERANCE, 0.0)[0], f"{k} columns")
    # A drop tolerance that is an existing |c|, and both tolerances at 0.
    hit = float(np.abs(want[2]).min())
    dropped = gc.node_reference(o, lp, cols, unit, ZERO_TOLERANCE, hit)[0]
    assert dropped[0][-1] < want[0][-1]
    same_cuts(g.gomory_cuts(cols, unit, ZERO_TOLERANCE, hit), dropped, "drop tolerance")
    same_cuts(g.gomory_cuts(cols, unit), gc.node_reference(o, lp, cols, unit)[0], "tolerances 0")
    # Summaries alone: the same records, no lists.
    alone = g.gomory_cuts(cols, unit, ZERO_TOLERANCE, 0.0, lists=False)
    assert alone[:3] == (None, None, None)
    same_summaries(alone[3], want[3], "summaries only")


def test_gomory_cuts_equal_two_dense_calls_and_the_numpy_rule(node):
    lp, unit, o, g, cols = node
    left, status, steps, f0, row_unit = gc.node_inputs(g, lp, cols, unit)
    result = g.gomory_cuts(cols, unit, ZERO_TOLERANCE, 0.0, with_left_inverses=True)
    got, left_g = result[:4], result[4]
    assert np.array_equal(bits(left_g), bits(left))
    basis = list(np.asarray(g.basis()))
    assert np.array_equal(bits(g.tableau_rows([basis.index(c) for c in cols], True)[1]),
                          bits(left))
    alpha = g.row_combinations(left)
    coef, bad = gc.coefficients(alpha, status, steps, f0, row_unit, ZERO_TOLERANCE)
    s = g.row_combinations(np.ascontiguousarray(coef[:, lp.n:]))[:, :lp.n]
    c = coef[:, :lp.n] - s
    want = gc.cut_lists(c, 0.0) + (gc.summarize(c, 0.0, bad.sum(axis=1)),)
    same_cuts(got, want, "two dense calls")
    # row_gomory_cuts takes everything from the caller: the same result.
    same_cuts(g.row_gomory_cuts(left, status, f0, row_unit, steps, ZERO_TOLERANCE, 0.0), want,
              "row_gomory_cuts")
    # Other inputs than the node's: every status, no units.
    rng = np.random.default_rng(8)
    status2 = rng.integers(0, 5, lp.n + lp.m).astype(np.int8)
    f2 = 0.05 + 0.9 * rng.random(len(cols))
    r2 = np.ldexp(1.0, rng.integers(-2, 3, len(cols)))
    _, bad2, c2 = gc.reference(pn.lp_matrix(lp), left, status2, None, f2, r2, 1e-7)
    assert (bad2 > 0).any()
    median = float(np.median(np.abs(c2)))
    same_cuts(g.row_gomory_cuts(left, status2, f2, r2, None, 1e-7, median),
              gc.cut_lists(c2, median) + (gc.summarize(c2, median, bad2),), "other inputs")


def test_get_cut_rows_returns_the_earlier_lists_after_a_summaries_only_call(node):
    lp, unit, o, g, cols = node
    starts, ccols, vals, _ = g.gomory_cuts(cols[:5], unit, ZERO_TOLERANCE, 0.0)
    g.gomory_cuts(cols, unit, ZERO_TOLERANCE, 0.0, lists=False)
    again_cols, again_vals = g.get_cut_rows(int(starts[-1]))
    assert np.array_equal(again_cols, ccols) and np.array_equal(bits(again_vals), bits(vals))
    # The sparse rows' store is another one.
    sparse = g.tableau_rows_sparse([0, 1])
    assert np.array_equal(g.get_cut_rows(int(starts[-1]))[0], ccols)
    g.gomory_cuts(cols[:2], unit)
    assert np.array_equal(g._sparse_rows(sparse[0], 2)[1], sparse[1])


def _raw(g, cols, unit, starts, summaries, zero=0.0, drop=0.0, k=None):
    vp = ctypes.c_void_p
    cols = None if cols is None else np.ascontiguousarray(cols, np.int32)

    def p(a):
        return None if a is None else a.ctypes.data_as(vp)

    count = k if k is not None else len(cols)
    return g._L.mi_lp_gomory_cuts(g.h, p(cols), count, p(unit), ctypes.c_double(zero),
                                  ctypes.c_double(drop), p(starts), p(summaries), None)


def test_errors_leave_the_outputs_and_the_store_untouched(node):
    lp, unit, o, g, cols = node
    N, vp = lp.n + lp.m, ctypes.c_void_p
    stored = g.gomory_cuts(cols[:3], unit, ZERO_TOLERANCE, 0.0)
    state = np.asarray(g.state())
    non_basic = int(np.nonzero(state[:lp.n] != 0)[0][0])
    continuous = int(np.nonzero((unit == 0) & (state[:lp.n] == 0))[0][0])
    basic_slack = int(lp.n + np.nonzero(state[lp.n:] == 0)[0][0])
    starts = np.zeros(4, np.int64)
    summaries = np.zeros(3, engine.CUT_SUMMARY)
    raw = (starts.view(np.uint8), summaries.view(np.uint8))
    for r in raw:
        r[:] = 0xA5
    good = np.array(cols[:2], np.int32)

    def with_unit(col, value):
        u = unit.copy()
        u[col] = value
        return u

    other = next(c for c in range(lp.n) if c not in good)
    for what, rc, want in (
            ("a non-basic column", _raw(g, [cols[0], non_basic], unit, starts, summaries),
             ERROR_INVALID_PROBLEM),
            ("a basic slack", _raw(g, [cols[0], basic_slack], unit, starts, summaries),
             ERROR_INVALID_PROBLEM),
            ("a column out of range", _raw(g, [cols[0], N], unit, starts, summaries),
             ERROR_INVALID_PROBLEM),
            ("a negative column", _raw(g, [-1], unit, starts, summaries), ERROR_INVALID_PROBLEM),
            ("a column with unit 0", _raw(g, [continuous], unit, starts, summaries),
             ERROR_INVALID_PROBLEM),
            ("k < 0", _raw(g, good, unit, starts, summaries, k=-1), ERROR_INVALID_PROBLEM),
            ("negative zero tolerance", _raw(g, good, unit, starts, summaries, zero=-1e-9),
             ERROR_INVALID_PROBLEM),
            ("NaN zero tolerance", _raw(g, good, unit, starts, summaries, zero=math.nan),
             ERROR_INVALID_PROBLEM),
            ("infinite zero tolerance", _raw(g, good, unit, starts, summaries, zero=math.inf),
             ERROR_INVALID_PROBLEM),
            ("negative drop tolerance", _raw(g, good, unit, starts, summaries, drop=-1.0),
             ERROR_INVALID_PROBLEM),
            ("NaN drop tolerance", _raw(g, good, unit, starts, summaries, drop=math.nan),
             ERROR_INVALID_PROBLEM),
            ("negative unit", _raw(g, good, with_unit(other, -1.0), starts, summaries),
             ERROR_INVALID_PROBLEM),
            ("NaN unit", _raw(g, good, with_unit(other, math.nan), starts, summaries),
             ERROR_INVALID_PROBLEM),
            ("infinite unit", _raw(g, good, with_unit(other, math.inf), starts, summaries),
             ERROR_INVALID_PROBLEM),
            ("infinite unit of the row", _raw(g, good, with_unit(good[0], math.inf), starts,
                                              summaries), ERROR_INVALID_PROBLEM),
            # value / unit is then an integer: the computed f0 is 0.
            ("f0 = 0", _raw(g, good, with_unit(good[0], float(g.primal()[good[0]])), starts,
                            summaries), ERROR_INVALID_PROBLEM),
            ("NULL cols", _raw(g, None, unit, starts, summaries, k=1), ERROR_NULL),
            ("NULL unit", _raw(g, good, None, starts, summaries), ERROR_NULL),
            ("both outputs NULL", _raw(g, good, unit, None, None), ERROR_NULL)):
        assert rc == want, (what, rc)
        assert all(np.all(r == 0xA5) for r in raw), what
    # mi_lp_row_gomory_cuts: its own table.
    left, status, steps, f0, row_unit = gc.node_inputs(o, lp, cols[:2], unit)
    bad_status = status.copy()
    bad_status[5] = 5
    args = {"y": left, "status": status, "unit": steps, "f0": f0, "row_unit": row_unit}

    def row_call(zero=0.0, drop=0.0, k=2, outputs=True, **replace):
        a = dict(args, **replace)
        keep = {key: None if v is None else np.ascontiguousarray(v) for key, v in a.items()}
        ptr = {key: None if v is None else v.ctypes.data_as(vp) for key, v in keep.items()}
        return g._L.mi_lp_row_gomory_cuts(
            g.h, ptr["y"], k, ptr["status"], ptr["unit"], ptr["f0"], ptr["row_unit"],
            ctypes.c_double(zero), ctypes.c_double(drop),
            starts.ctypes.data_as(vp) if outputs else None,
            summaries.ctypes.data_as(vp) if outputs else None)

    two = np.array
    for what, rc, want in (
            ("status 5", row_call(status=bad_status), ERROR_INVALID_PROBLEM),
            ("status -1", row_call(status=-bad_status.clip(0, 1)), ERROR_INVALID_PROBLEM),
            ("k < 0", row_call(k=-1), ERROR_INVALID_PROBLEM),
            ("NaN zero tolerance", row_call(zero=math.nan), ERROR_INVALID_PROBLEM),
            ("infinite zero tolerance", row_call(zero=math.inf), ERROR_INVALID_PROBLEM),
            ("negative drop tolerance", row_call(drop=-0.5), ERROR_INVALID_PROBLEM),
            ("infinite unit", row_call(unit=np.full(N, math.inf)), ERROR_INVALID_PROBLEM),
            ("negative unit", row_call(unit=np.full(N, -1.0)), ERROR_INVALID_PROBLEM),
            ("f0 = 0", row_call(f0=two([0.5, 0.0])), ERROR_INVALID_PROBLEM),
            ("f0 = 1", row_call(f0=two([1.0, 0.5])), ERROR_INVALID_PROBLEM),
            ("NaN f0", row_call(f0=two([math.nan, 0.5])), ERROR_INVALID_PROBLEM),
            ("row_unit 0", row_call(row_unit=two([0.0, 1.0])), ERROR_INVALID_PROBLEM),
            ("negative row_unit", row_call(row_unit=two([1.0, -1.0])), ERROR_INVALID_PROBLEM),
            ("infinite row_unit", row_call(row_unit=two([math.inf, 1.0])), ERROR_INVALID_PROBLEM),
            ("NaN row_unit", row_call(row_unit=two([1.0, math.nan])), ERROR_INVALID_PROBLEM),
            ("NULL y", row_call(y=None), ERROR_NULL),
            ("NULL status", row_call(status=None), ERROR_NULL),
            ("NULL f0", row_call(f0=None), ERROR_NULL),
            ("NULL row_unit", row_call(row_unit=None), ERROR_NULL),
            ("both outputs NULL", row_call(outputs=False), ERROR_NULL)):
        assert rc == want, (what, rc)
        assert all(np.all(r == 0xA5) for r in raw), what
    # An infinite drop tolerance is allowed: nothing is kept.
    assert row_call(drop=math.inf) == 0
    assert np.all(starts[:3] == 0) and np.all(summaries["count"][:2] == 0)
    for r in raw:
        r[:] = 0xA5
    # The store is the one from before the errors (the last call replaced it
    # with an empty one: build it again and fail again).
    stored = g.gomory_cuts(cols[:3], unit, ZERO_TOLERANCE, 0.0)
    assert row_call(k=-1) == ERROR_INVALID_PROBLEM and row_call(f0=two([0.5, 1.5])) == \
        ERROR_INVALID_PROBLEM
    again = g.get_cut_rows(int(stored[0][-1]))
    assert np.array_equal(again[0], stored[1]) and np.array_equal(bits(again[1]), bits(stored[2]))
    # k = 0 succeeds, writes row_starts[0] = 0 and stores an empty result.
    assert _raw(g, good, unit, starts, summaries, k=0) == 0 and starts[0] == 0
    assert np.all(raw[0][8:] == 0xA5) and np.all(raw[1] == 0xA5)
    assert g.get_cut_rows(0)[0].shape == (0,)
    out = g.gomory_cuts([], unit)
    assert out[0].tolist() == [0] and len(out[1]) == len(out[2]) == len(out[3]) == 0
    # Beyond k nothing is written.
    starts.view(np.uint8)[:] = 0xA5
    assert _raw(g, good, unit, starts, summaries) == 0
    assert np.all(raw[0][24:] == 0xA5) and np.all(raw[1][64:] == 0xA5)
    same_summaries(summaries[:2], g.gomory_cuts(good, unit)[3], "raw call")


def test_before_a_solve_and_after_a_load_are_state_errors():
    lp, ycols, unit = node_lp("ft06")
    g = engine.LpHandle(params())
    g.load(lp)
    starts = np.zeros(2, np.int64)
    raw = starts.view(np.uint8)
    raw[:] = 0xA5
    vp = ctypes.c_void_p
    assert _raw(g, [ycols[0]], unit, starts, None) == ERROR_STATE
    y, st, half = np.zeros(lp.m), np.zeros(lp.n + lp.m, np.int8), np.full(1, 0.5)
    assert g._L.mi_lp_row_gomory_cuts(g.h, y.ctypes.data_as(vp), 1, st.ctypes.data_as(vp), None,
                                      half.ctypes.data_as(vp), half.ctypes.data_as(vp),
                                      ctypes.c_double(0.0), ctypes.c_double(0.0),
                                      starts.ctypes.data_as(vp), None) == ERROR_STATE
    assert np.all(raw == 0xA5)
    buf_c, buf_v = np.zeros(4, np.int32), np.zeros(4)
    assert g._L.mi_lp_get_cut_rows(g.h, buf_c.ctypes.data_as(vp),
                                   buf_v.ctypes.data_as(vp)) == ERROR_STATE
    assert g.solve().problem_status == abi.OPTIMAL
    cols = fractional(g.primal(), ycols, unit, np.asarray(g.state()))
    g.gomory_cuts(cols[:2], unit)
    assert g._L.mi_lp_get_cut_rows(g.h, np.zeros(4096, np.int32).ctypes.data_as(vp),
                                   np.zeros(4096).ctypes.data_as(vp)) == 0
    g.load(lp)
    assert g._L.mi_lp_get_cut_rows(g.h, buf_c.ctypes.data_as(vp),
                                   buf_v.ctypes.data_as(vp)) == ERROR_STATE
    g.close()


def test_column_shards_are_refused_before_any_device_work(monkeypatch):
    monkeypatch.setenv("MILP_SHARDS", "2")
    lp, ycols, unit = node_lp("ft06")
    g = engine.LpHandle(params())
    g.load(lp)
    assert g.solve().problem_status == abi.OPTIMAL
    cols = fractional(g.primal(), ycols, unit, np.asarray(g.state()))
    starts = np.zeros(3, np.int64)
    summaries = np.zeros(2, engine.CUT_SUMMARY)
    raw = (starts.view(np.uint8), summaries.view(np.uint8))
    for r in raw:
        r[:] = 0xA5
    assert _raw(g, cols[:2], unit, starts, summaries) == ERROR_STATE
    assert "not with column shards" in g.last_error()
    vp = ctypes.c_void_p
    y, st, half = np.zeros((2, lp.m)), np.asarray(g.state(), np.int8), np.full(2, 0.5)
    assert g._L.mi_lp_row_gomory_cuts(g.h, y.ctypes.data_as(vp), 2, st.ctypes.data_as(vp), None,
                                      half.ctypes.data_as(vp), half.ctypes.data_as(vp),
                                      ctypes.c_double(0.0), ctypes.c_double(0.0),
                                      starts.ctypes.data_as(vp),
                                      summaries.ctypes.data_as(vp)) == ERROR_STATE
    assert "not with column shards" in g.last_error()
    assert all(np.all(r == 0xA5) for r in raw)
    # No device error, and the handle is as good as before.
    assert not _device_error
    assert g.solve().problem_status == abi.OPTIMAL
    g.close()


def test_a_later_solve_is_unaffected():
    lp, ycols, unit = node_lp("random_6_4_7")
    o, ro, g, rg = parity_util.solve_both(lp, params(), lambda q: engine.LpHandle(q))
    cols = fractional(o.primal(), ycols, unit, np.asarray(o.state()))
    g.gomory_cuts(cols, unit, ZERO_TOLERANCE, 0.0)
    basis = list(np.asarray(o.basis()))
    for c in cols:  # the side effects the header names: one left solve per column
        o.unit_row_left_inverse(basis.index(c))
    x = o.primal()
    lb, ub = np.array(lp.col_lb), np.array(lp.col_ub)
    ub[cols[0]] = math.floor(x[cols[0]])
    lb[cols[1]] = math.ceil(x[cols[1]])
    for h in (o, g):
        h.set_variable_bounds(lb, ub)
    ro2, rg2 = o.solve(), g.solve()
    assert ro2.iterations > 0
    parity_util.compare(o, ro2, g, rg2, lp)
    g.close()


class OracleWithCuts(oracle_lib.OracleLp):
    """The oracle handle with the one call it lacks, served by the numpy
    reference: what cpsat.gomory_cuts needs of a handle."""

    def gomory_cuts(self, cols, unit, zero_tolerance=0.0, drop_tolerance=0.0):
        return gc.node_reference(self, self.lp, cols, unit, zero_tolerance, drop_tolerance)[0]


@pytest.mark.parametrize("scaling", [False, True])
def test_cpsat_gomory_cuts_on_the_oracle_and_on_the_engine(scaling):
    lp, ycols = jobshop.relaxation(jobshop.random_instance(6, 4, 7))
    out = []
    for handle in (OracleWithCuts(params()), engine.LpHandle(params())):
        c = cpsat.LpConstraint(lp, ycols, handle, scaling=scaling)
        t = cpsat.IntegerTrail(lp.col_lb, lp.col_ub)
        assert c.solve_lp(t) and c.analyze_lp(t)
        cols = cpsat.fractional_columns(c.lp_solution, ycols, limit=20)
        out.append((cols, cpsat.gomory_cuts(c, c.lp_solution, cols),
                    np.asarray(c.lp_solution, np.float64) * c.factor))
    (cols_o, cuts_o, x_o), (cols_g, cuts_g, x_g) = out
    assert cols_o == cols_g and len(cuts_o) == len(cuts_g) > 0
    for a, b in zip(cuts_o, cuts_g):
        assert a["col"] == b["col"] and np.array_equal(a["cols"], b["cols"])
        assert np.array_equal(bits(a["coefs"]), bits(b["coefs"])) and a["rhs"] == b["rhs"]
        assert a["max_abs"] == b["max_abs"] and a["min_abs"] == b["min_abs"]
    for cut in cuts_g:
        # coefs . x* == rhs - 1 to within an ulp of the sum.
        lhs = math.fsum(cut["coefs"] * x_g[cut["cols"]])
        assert abs(lhs - (cut["rhs"] - 1.0)) <= np.spacing(abs(cut["rhs"]) + 1.0)
