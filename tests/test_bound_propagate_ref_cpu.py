"""The reference and the inputs of the bound-propagation tests
(tests/bound_propagate_cases.py), checked without a GPU: conditions on the
reference ALONE, so that no GPU test can pass vacuously. The hand cases'
results are asserted literally; propagate() equals a literal Python-float copy
of the header's loop on them; the node cases reach every status on every
matrix, take several rounds, stop in different rounds within one call and have
bounds that the integer rounding alone moves.
"""
import numpy as np
import pytest

import bound_implied_cases as ic
import bound_propagate_cases as pc
import bound_range_cases as bc
from device_ref import bits

HAND = ("chain", "halving", "knapsack", "negzero")


def run(name, tol, max_rounds, integers=True):
    mat, L, U, lb, ub, ints = pc.hand(name)
    return pc.propagate(mat, L, U, lb, ub, ints if integers else None, tol, pc.ITOL, max_rounds)


def test_chain():
    NL, NU, s = run("chain", 0.0, 40)
    assert s["status"].tolist() == [pc.FIXPOINT, pc.FIXPOINT, pc.INFEASIBLE, pc.INFEASIBLE]
    assert s["rounds"].tolist() == [12, 12, 6, 3]
    assert s["moves"].tolist() == [102, 102, 72, 36]
    assert s["worst"].tolist() == [0.0, 0.0, 1.0, 1.0]
    assert s["worst_col"].tolist() == [-1, -1, 5, 3]
    ramp = np.arange(12.0)
    assert np.array_equal(bits(NL[0]), bits(ramp)) and np.array_equal(bits(NL[1]), bits(ramp))
    assert np.array_equal(bits(NU[1]), bits(ramp))  # u = 11: l = u = 0 .. 11
    assert np.array_equal(bits(NU[0]), bits(ramp + 9.0))


@pytest.mark.parametrize("tol,max_rounds,status,rounds,upper",
                         [(0.0, 8, pc.ROUND_LIMIT, 8, 2.0 ** -8),
                          (0.375, 8, pc.FIXPOINT, 2, 0.5),
                          (1e-9, 100, pc.FIXPOINT, 30, 2.0 ** -29)])
def test_halving(tol, max_rounds, status, rounds, upper):
    NL, NU, s = run("halving", tol, max_rounds)
    assert (s["status"][0], s["rounds"][0]) == (status, rounds)
    assert NU[0].tolist() == [upper, upper] and NL[0].tolist() == [0.0, 0.0]
    assert s["worst_col"][0] == -1 and s["worst"][0] == 0.0


def test_knapsack():
    NL, NU, s = run("knapsack", 0.0, 8)
    assert (s["status"][0], s["rounds"][0], s["moves"][0]) == (pc.FIXPOINT, 2, 2)
    assert NU[0].tolist() == [2.0, 1.0]
    NL, NU, s = run("knapsack", 0.0, 8, integers=False)
    assert (s["status"][0], s["rounds"][0]) == (pc.FIXPOINT, 2)
    assert NU[0].tolist() == [7.0 / 3.0, 7.0 / 5.0]


def test_negative_zero_becomes_positive_zero():
    mat, L, U, lb, ub, ints = pc.hand("negzero")
    raw = ic.implied(mat, L, U, bc.ranges(mat, L, U), lb, ub)
    assert raw[0][0, 0] == -0.5
    assert np.signbit(np.ceil(raw[0][0, 0] - pc.ITOL))  # what + 0.0 is there for
    NL, NU, s = run("negzero", 0.0, 8)
    assert bits(NL[0, 0]) == bits(np.float64(0.0)) and NU[0, 0] == 5.0
    assert (s["status"][0], s["rounds"][0], s["moves"][0], s["kept"][0]) == (pc.FIXPOINT, 2, 1, 1)


@pytest.mark.parametrize("name", HAND)
def test_reference_is_the_headers_loop(name):
    mat, L, U, lb, ub, ints = pc.hand(name)
    for tol, max_rounds in ((0.0, 1), (0.0, 5), (0.0, 40), (0.375, 8)):
        for use in ((ints, None) if ints is not None else (None,)):
            NL, NU, s = pc.propagate(mat, L, U, lb, ub, use, tol, pc.ITOL, max_rounds)
            for j in range(L.shape[0]):
                l, u, status, rounds, moves, worst, worst_col = pc.propagate_scalar(
                    mat, L[j], U[j], lb, ub, use, tol, pc.ITOL, max_rounds)
                what = (name, tol, max_rounds, j)
                assert np.array_equal(bits(NL[j]), bits(np.array(l))), what
                assert np.array_equal(bits(NU[j]), bits(np.array(u))), what
                assert (s["status"][j], s["rounds"][j], s["moves"][j], s["worst_col"][j]) == \
                    (status, rounds, moves, worst_col), what
                assert bits(s["worst"][j]) == bits(np.float64(worst)), what


def test_own_crossing_stops_in_round_one_without_a_move():
    mat, L, U, lb, ub, _ = pc.hand("halving")
    L, U = L.copy(), U.copy()
    L[0, 1], U[0, 1] = 3.0, 1.0  # the own bounds cross
    free = np.full(2, np.inf)
    NL, NU, s = pc.propagate(mat, L, U, -free, free, None, 0.0, pc.ITOL, 5)
    assert (s["status"][0], s["rounds"][0], s["worst_col"][0]) == (pc.INFEASIBLE, 1, 1)
    assert s["moves"][0] == 0 and s["worst"][0] == 2.0 and s["kept"][0] == 0
    # own_crossing: the column crosses without a move beside columns that
    # move, so moves is smaller than the number of moved-or-crossing columns.
    for name in ("steps", "rows70"):
        f = pc.grid(name)[0][0]
        base_lb, base_ub = pc.node(name, f)[:2]
        sets, c = pc.own_crossing(name)
        L, U = bc.materialise(base_lb, base_ub, sets)
        NL, NU, s = pc.own_crossing_reference(name)
        assert (s["status"][2], s["rounds"][2]) == (pc.INFEASIBLE, 1), name
        assert bits(NL[2, c]) == bits(L[2, c]) and bits(NU[2, c]) == bits(U[2, c]), name
        assert NL[2, c] - NU[2, c] > 1.9 and s["moves"][2] > 0, name
        assert set(s["status"][[0, 1, 3]].tolist()) != {pc.INFEASIBLE}, name


@pytest.mark.parametrize("name", pc.CASES)
def test_one_round_is_implied_and_the_move_rule(name):
    f, tol, integers = pc.grid(name)[0]
    assert not integers
    L, U = pc.node_sets(name, f, pc.CHILDREN)
    _, _, _, row_lb, row_ub = pc.node(name, f)
    mat = ic.matrix(name)
    NL, NU = ic.implied(mat, L, U, bc.ranges(mat, L, U), row_lb, row_ub)
    with np.errstate(invalid="ignore"):
        moved = (NL - L > tol) | (U - NU > tol)
    want = (np.where(moved, NL, L), np.where(moved, NU, U))
    got = pc.trace(name, f, tol, False)[1]
    ic.same_bounds(got[:2], want, name)
    assert np.array_equal(got[2]["moves"], moved.sum(axis=1))
    assert (got[2]["rounds"] == 1).all()


@pytest.mark.parametrize("name", pc.CASES)
def test_the_traces_fold_is_implied(name):
    """implied_columns, which the traces use, against bound_implied_cases.implied
    on all 64 bits: on the node's sets, on the sets a few rounds later, and on
    the pool with its NaN, infinite and huge own bounds under every row-bound
    set."""
    mat = ic.matrix(name)
    f, tol, integers = pc.grid(name)[1]
    row_lb, row_ub = pc.node(name, f)[3:]
    later = pc.trace(name, f, tol, integers)[3]
    for L, U in (pc.node_sets(name, f, pc.CHILDREN), later[:2]):
        ref = bc.ranges(mat, L, U)
        ic.same_bounds(pc.implied_columns(mat, L, U, ref, row_lb, row_ub),
                       ic.implied(mat, L, U, ref, row_lb, row_ub), name)
    L, U = ic.pool(name)
    for which in ic.ROW_BOUND_SETS:
        ic.same_bounds(pc.implied_columns(mat, L, U, ic.ranges_reference(name),
                                          *ic.row_bounds(name, which)),
                       ic.reference(name, which), (name, which))
    for hand in HAND:
        mat, L, U, lb, ub, _ = pc.hand(hand)
        ref = bc.ranges(mat, L, U)
        ic.same_bounds(pc.implied_columns(mat, L, U, ref, lb, ub),
                       ic.implied(mat, L, U, ref, lb, ub), hand)


@pytest.mark.parametrize("name", pc.CASES)
def test_node_cases_hold_what_they_are_there_for(name):
    statuses, rounds_differ, rounded_alone = set(), False, 0
    for f, tol, integers in pc.grid(name):
        tr = pc.trace(name, f, tol, integers)
        for R in pc.ROUNDS:
            s = tr[R][2]
            statuses |= set(s["status"].tolist())
            assert (s["rounds"] <= R).all() and (s["rounds"] >= 1).all()
            limited = s["status"] == pc.ROUND_LIMIT
            assert (s["rounds"][limited] == R).all()
            assert (s["worst_col"][s["status"] != pc.INFEASIBLE] == -1).all()
            assert (s["worst"][s["status"] == pc.INFEASIBLE] > tol).all()
        last = tr[max(pc.ROUNDS)][2]
        stopped = last["rounds"][last["status"] != pc.ROUND_LIMIT]
        rounds_differ |= len(set(stopped.tolist())) > 1
        if name != "rows70":
            assert (last["rounds"] >= 3).sum() * 2 >= pc.CHILDREN, (name, f, tol, integers)
    assert statuses == {pc.ROUND_LIMIT, pc.FIXPOINT, pc.INFEASIBLE}, (name, statuses)
    assert rounds_differ, name
    # The rounding alone moves a bound: one round of the first children.
    f, tol, _ = pc.grid(name)[0]
    base_lb, base_ub, sets, row_lb, row_ub = pc.node(name, f)
    stats = {}
    pc.trace_rounds(ic.matrix(name), *pc.node_sets(name, f, 4), row_lb, row_ub,
                    pc.integer_columns(name), tol, pc.ITOL, (1,), stats=stats)
    assert stats["rounded_alone"] > 0, name


def test_a_second_panel_of_one_stops_apart_from_the_first():
    """k = 17: the seventeenth child's round count is not the largest of the
    first sixteen somewhere in the grid, so the two panels launch different
    numbers of rounds."""
    found = False
    for name in pc.CASES:
        for f, tol, integers in pc.grid(name):
            s = pc.trace(name, f, tol, integers)[30][2]
            found |= s["rounds"][16] != s["rounds"][:16].max()
    assert found


def test_lists_are_the_changed_or_crossing_columns():
    name, (f, tol) = "steps", pc.GRID[0]
    base_lb, base_ub = pc.node(name, f)[:2]
    col_starts, cols, lo, hi, s = pc.expected_lists(name, f, tol, True, 30, pc.CHILDREN)
    NL, NU, dense = pc.expected(name, f, tol, True, 30, pc.CHILDREN)
    assert np.array_equal(s["kept"], np.diff(col_starts))
    L, U = bc.materialise(base_lb, base_ub,
                          [(cols[a:b], lo[a:b], hi[a:b])
                           for a, b in zip(col_starts[:-1], col_starts[1:])])
    ic.same_bounds((L, U), (NL, NU), "materialised lists")
    assert (s["kept"] > 0).any() and (s["kept"] < len(base_lb)).all()
