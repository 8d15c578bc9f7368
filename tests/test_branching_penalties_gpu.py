"""mi_lp_branching_penalties / mi_lp_row_penalties (include/mi_lp.h) through
mi_glop.engine.LpHandle, on the branch-and-bound nodes of tests/test_cpsat.py
(the root LPs of job-shop relaxations).

The records are pinned by Glop's public surface and the rule alone: the
oracle's GetUnitRowLeftInverse, reduced costs, dual values, statuses and
primal values feed the numpy reference (tests/penalty_cases.py node_reference:
ColumnScalarProduct of every column, then the rule). The engine's records
equal it bit for bit; every error of the header's table is returned with
nothing written; the left inverses are those of mi_lp_get_tableau_rows; a
later solve is what it is without the call; and cpsat.branch_penalties gives
the same bounds on the engine as on the oracle.
tests/test_penalties_ref_cpu.py checks on the same nodes that the penalties
are valid bounds.
"""
import ctypes
import math

import numpy as np
import pytest

from mi_glop import abi, cpsat, engine

import jobshop
import oracle_lib
import parity_util
import penalty_cases as pn
from device_ref import bits

pytestmark = pytest.mark.gpu

ERROR_NULL, ERROR_INVALID_PROBLEM, ERROR_STATE, ERROR_DEVICE = 3, 4, 101, 100
NODES = {"ft06": lambda: jobshop.FT06, "random_6_4_7": lambda: jobshop.random_instance(6, 4, 7)}
TOLERANCE = cpsat.PENALTY_PIVOT_TOLERANCE

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


def same_records(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    for f in ("down", "up"):
        assert np.array_equal(bits(got[f]), bits(want[f])), (what, f, got[f], want[f])
    for f in ("down_col", "up_col", "down_count", "up_count"):
        assert np.array_equal(got[f], want[f]), (what, f, got[f], want[f])


@pytest.fixture(scope="module", params=sorted(NODES))
def node(request):
    """(lp, integer columns, oracle, engine handle, fractional columns): the
    node solved by both, with equal results."""
    lp, ycols = jobshop.relaxation(NODES[request.param]())
    o, ro, g, rg = parity_util.solve_both(lp, params(), lambda q: engine.LpHandle(q))
    parity_util.compare(o, ro, g, rg, lp)
    assert rg.problem_status == abi.OPTIMAL
    cols = cpsat.fractional_columns(o.primal(), ycols)
    assert len(cols) > 16, "more than one panel of candidates"
    yield lp, ycols, o, g, cols
    g.close()


def test_branching_penalties_equal_the_reference_fed_from_the_oracle(node):
    lp, ycols, o, g, cols = node
    unit = np.zeros(lp.n)
    unit[ycols] = 1.0
    want = pn.node_reference(o, lp, cols, tolerance=TOLERANCE)
    assert (want["down"] > 0).any() or (want["up"] > 0).any()
    same_records(g.branching_penalties(cols, pivot_tolerance=TOLERANCE), want, "NULL distances")
    for k in (1, 4, 16, 17):
        same_records(g.branching_penalties(cols[:k], pivot_tolerance=TOLERANCE), want[:k],
                     f"{k} columns")
    same_records(g.branching_penalties(cols, unit=unit, pivot_tolerance=TOLERANCE),
                 pn.node_reference(o, lp, cols, unit=unit, tolerance=TOLERANCE), "with units")
    rng = np.random.default_rng(5)
    down, up = rng.random(len(cols)), rng.random(len(cols))
    down[0] = up[1] = 0.0
    same_records(g.branching_penalties(cols, down, up, unit, 0.0),
                 pn.node_reference(o, lp, cols, down, up, unit, 0.0), "given distances")
    # Basic slack columns, and structural ones that are not integer, serve too.
    basis = np.asarray(o.basis())
    others = [int(c) for c in basis if c >= lp.n][:5] + \
        [int(c) for c in basis if c < lp.n and c not in set(cols)][:5]
    assert any(c >= lp.n for c in others)
    same_records(g.branching_penalties(others, pivot_tolerance=TOLERANCE),
                 pn.node_reference(o, lp, others, tolerance=TOLERANCE), "slack columns")


def test_row_penalties_take_everything_from_the_caller(node):
    lp, ycols, o, g, cols = node
    left, d, status, values = pn.node_inputs(o, lp, cols)
    down, up = values - np.floor(values), np.ceil(values) - values
    want = pn.node_reference(o, lp, cols, tolerance=TOLERANCE)
    same_records(g.row_penalties(left, d, status, down, up, None, TOLERANCE), want,
                 "the node's own inputs")
    # Other inputs than the node's: every status, a NaN, a zero distance.
    rng = np.random.default_rng(6)
    status2 = rng.integers(0, 5, lp.n + lp.m).astype(np.int8)
    d2 = rng.standard_normal(lp.n + lp.m)
    d2[rng.random(len(d2)) < 0.02] = np.nan
    unit2 = np.where(rng.random(len(d2)) < 0.5, 0.25, 0.0)
    down2 = down.copy()
    down2[0] = 0.0
    mat = pn.lp_matrix(lp)
    a = np.stack([pn.column_scalar_products(mat, np.arange(mat.N), y) for y in left])
    same_records(g.row_penalties(left, d2, status2, down2, up, unit2, 1e-7),
                 pn.reference(a, d2, status2, unit2, down2, up, 1e-7), "other inputs")


def test_left_inverses_are_those_of_tableau_rows(node):
    lp, ycols, o, g, cols = node
    basis = list(np.asarray(g.basis()))
    rows = [basis.index(c) for c in cols]
    _, want = g.tableau_rows(rows, True)
    rec, left = g.branching_penalties(cols, pivot_tolerance=TOLERANCE, with_left_inverses=True)
    assert np.array_equal(bits(left), bits(want))
    same_records(rec, g.branching_penalties(cols, pivot_tolerance=TOLERANCE), "with and without")


def _raw(g, cols, out, down=None, up=None, unit=None, tolerance=0.0, k=None):
    vp = ctypes.c_void_p
    cols = np.ascontiguousarray(cols, np.int32)

    def p(a):
        return None if a is None else a.ctypes.data_as(vp)

    return g._L.mi_lp_branching_penalties(g.h, p(cols), len(cols) if k is None else k, p(down),
                                          p(up), p(unit), ctypes.c_double(tolerance), p(out),
                                          None)


def test_errors_leave_out_untouched(node):
    lp, ycols, o, g, cols = node
    N, vp = lp.n + lp.m, ctypes.c_void_p
    state = np.asarray(g.state())
    non_basic = int(np.nonzero(state != 0)[0][0])
    out = np.zeros(4, engine.BRANCH_PENALTY)
    raw = out.view(np.uint8)
    raw[:] = 0xA5
    good = np.array(cols[:2], np.int32)
    half = np.full(2, 0.5)
    bad_unit = np.zeros(lp.n)
    bad_unit[3] = -1.0
    for what, rc, want in (
            ("a non-basic column", _raw(g, [cols[0], non_basic], out), ERROR_INVALID_PROBLEM),
            ("a column out of range", _raw(g, [cols[0], N], out), ERROR_INVALID_PROBLEM),
            ("a negative column", _raw(g, [-1], out), ERROR_INVALID_PROBLEM),
            ("k < 0", _raw(g, good, out, k=-1), ERROR_INVALID_PROBLEM),
            ("negative tolerance", _raw(g, good, out, tolerance=-1e-9), ERROR_INVALID_PROBLEM),
            ("NaN tolerance", _raw(g, good, out, tolerance=math.nan), ERROR_INVALID_PROBLEM),
            ("negative distance", _raw(g, good, out, down=np.array([0.5, -0.5]), up=half),
             ERROR_INVALID_PROBLEM),
            ("NaN distance", _raw(g, good, out, down=half, up=np.array([math.nan, 0.5])),
             ERROR_INVALID_PROBLEM),
            ("infinite distance", _raw(g, good, out, down=half, up=np.array([math.inf, 0.5])),
             ERROR_INVALID_PROBLEM),
            ("negative unit", _raw(g, good, out, unit=bad_unit), ERROR_INVALID_PROBLEM),
            ("NULL cols", g._L.mi_lp_branching_penalties(g.h, None, 1, None, None, None,
                                                         ctypes.c_double(0.0),
                                                         out.ctypes.data_as(vp), None),
             ERROR_NULL),
            ("NULL out", g._L.mi_lp_branching_penalties(g.h, good.ctypes.data_as(vp), 2, None,
                                                        None, None, ctypes.c_double(0.0), None,
                                                        None), ERROR_NULL)):
        assert rc == want, (what, rc)
        assert np.all(raw == 0xA5), what
    # mi_lp_row_penalties: its own table.
    left, d, status, values = pn.node_inputs(o, lp, cols[:2])
    bad_status = status.copy()
    bad_status[5] = 5
    args = {"y": left, "d": d, "status": status, "unit": None, "down": half, "up": half}

    def row_call(tolerance=0.0, k=2, **replace):
        a = dict(args, **replace)
        ptr = [None if a[key] is None else np.ascontiguousarray(a[key]).ctypes.data_as(vp)
               for key in ("y", "d", "status", "unit", "down", "up")]
        keep = [np.ascontiguousarray(v) for v in a.values() if v is not None]  # noqa: F841
        return g._L.mi_lp_row_penalties(g.h, ptr[0], k, ptr[1], ptr[2], ptr[3], ptr[4], ptr[5],
                                        ctypes.c_double(tolerance), out.ctypes.data_as(vp))

    for what, rc, want in (
            ("status 5", row_call(status=bad_status), ERROR_INVALID_PROBLEM),
            ("status -1", row_call(status=-bad_status.clip(0, 1)), ERROR_INVALID_PROBLEM),
            ("k < 0", row_call(k=-1), ERROR_INVALID_PROBLEM),
            ("NaN tolerance", row_call(tolerance=math.nan), ERROR_INVALID_PROBLEM),
            ("infinite unit", row_call(unit=np.full(N, math.inf)), ERROR_INVALID_PROBLEM),
            ("negative distance", row_call(up=np.array([-0.0, -1e-300])), ERROR_INVALID_PROBLEM),
            ("NULL y", row_call(y=None), ERROR_NULL),
            ("NULL d", row_call(d=None), ERROR_NULL),
            ("NULL status", row_call(status=None), ERROR_NULL),
            ("NULL distances", row_call(down=None), ERROR_NULL)):
        assert rc == want, (what, rc)
        assert np.all(raw == 0xA5), what
    # k = 0 succeeds and writes nothing; beyond k nothing is written.
    assert _raw(g, good, out, k=0) == 0 and row_call(k=0) == 0
    assert np.all(raw == 0xA5)
    assert _raw(g, good, out) == 0
    assert not np.all(raw[:64] == 0xA5) and np.all(raw[64:] == 0xA5)
    same_records(out[:2], g.branching_penalties(good), "raw call")
    assert g.branching_penalties([]).shape == (0,)


def test_before_a_solve_is_a_state_error():
    lp, _ = jobshop.relaxation(jobshop.FT06)
    g = engine.LpHandle(params())
    g.load(lp)
    out = np.zeros(1, engine.BRANCH_PENALTY)
    raw = out.view(np.uint8)
    raw[:] = 0xA5
    assert _raw(g, [0], out) == ERROR_STATE
    vp = ctypes.c_void_p
    y, d, st, dist = np.zeros(lp.m), np.zeros(lp.n + lp.m), np.zeros(lp.n + lp.m, np.int8), \
        np.zeros(1)
    assert g._L.mi_lp_row_penalties(g.h, y.ctypes.data_as(vp), 1, d.ctypes.data_as(vp),
                                    st.ctypes.data_as(vp), None, dist.ctypes.data_as(vp),
                                    dist.ctypes.data_as(vp), ctypes.c_double(0.0),
                                    out.ctypes.data_as(vp)) == ERROR_STATE
    assert np.all(raw == 0xA5)
    g.close()


def test_a_later_solve_is_unaffected():
    lp, ycols = jobshop.relaxation(jobshop.random_instance(6, 4, 7))
    o, ro, g, rg = parity_util.solve_both(lp, params(), lambda q: engine.LpHandle(q))
    cols = cpsat.fractional_columns(o.primal(), ycols)
    g.branching_penalties(cols, pivot_tolerance=TOLERANCE)
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


class OracleWithPenalties(oracle_lib.OracleLp):
    """The oracle handle with the one call it lacks, served by the numpy
    reference: what cpsat.branch_penalties needs of a handle."""

    def branching_penalties(self, cols, down_dist=None, up_dist=None, unit=None,
                            pivot_tolerance=0.0):
        return pn.node_reference(self, self.lp, cols, down_dist, up_dist, unit, pivot_tolerance)


@pytest.mark.parametrize("scaling", [False, True])
def test_cpsat_branch_penalties_on_the_oracle_and_on_the_engine(scaling):
    lp, ycols = jobshop.relaxation(jobshop.random_instance(6, 4, 7))
    out = []
    for handle in (OracleWithPenalties(params()), engine.LpHandle(params())):
        c = cpsat.LpConstraint(lp, ycols, handle, scaling=scaling)
        t = cpsat.IntegerTrail(lp.col_lb, lp.col_ub)
        assert c.solve_lp(t) and c.analyze_lp(t)
        cols = cpsat.fractional_columns(c.lp_solution, ycols, limit=20)
        t.obj_ub = c.lp_objective + 60.0
        out.append((cols, c.lp_objective, cpsat.branch_penalties(c, t, c.lp_solution, cols)))
    (cols_o, obj_o, pen_o), (cols_g, obj_g, pen_g) = out
    assert cols_o == cols_g and obj_o == obj_g and pen_o == pen_g
    assert len(pen_g) == 2 * len(cols_g)
    assert any(p["bound"] > obj_g for p in pen_g) and any(p["cutoff"] for p in pen_g)
    assert not all(p["cutoff"] for p in pen_g)
    for p in pen_g:
        assert p["cutoff"] == (p["infeasible"] or
                               math.ceil(p["bound"] - cpsat.K_CP_EPSILON) > obj_g + 60.0)
