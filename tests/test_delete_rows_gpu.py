"""mi_lp_delete_rows (include/mi_lp.h) through mi_glop.engine.LpHandle: in
everything a handle later returns, deleting rows is the load of the reduced LP
followed by load_basis_state of the state without the deleted rows' slacks.

Nodes, parameters and the cut rule are those of tests/test_add_rows_gpu.py.
Handle A calls delete_rows, handle B loads lp.without_rows(mask) and then the
compacted state, the CPU oracle does what B does.

  1. the purge loop: four rounds of add cuts, solve, purge the cuts whose slack
     is BASIC, solve. A, B and the oracle agree after every solve; every
     post-purge solve is OPTIMAL with 0 iterations and an unchanged state
     (observed on the oracle for all eight) and takes fewer iterations than a
     fresh handle on the same LP (113 to 197 there); delete_rows and the next
     add_rows both take path 1;
  2. three other deletions, on side handles loaded from the LP and the state
     of each of three rounds of a loop that only adds cuts: all cuts, every
     7th original row, every 11th original row plus the basic-slack cuts.
     A = B = oracle, and fewer iterations than a fresh handle (at worst 115
     against 152 on the oracle);
  3. call orders, each equal to its twin: before the first solve, after
     load_basis_state, two deletes in a row, append then delete the appended
     rows, delete d then append d, delete then set_variable_bounds, delete
     then the load of a different LP, an empty mask, the last row deleted
     and appended again, and a mask over every row (path 2) with rows appended
     afterwards;
  4. after the delete and a solve the panel calls equal B's bit for bit, and
     the stores are forgotten by the delete;
  5. the header's error table, each error leaving the next solve that of an
     untouched twin;
  6. MILP_SHARDS=2 takes path 2 with equal results; batch_solve_bounds over
     workers that deleted equals workers that loaded; cpsat.purge_cuts on the
     engine equals a test-side adapter on the oracle.
"""
import ctypes
import functools

import numpy as np
import pytest

from mi_glop import abi, cpsat, engine

import gomory_cases as gc
import jobshop
import oracle_lib
import parity_util
import test_add_rows_gpu as ar
from device_ref import bits

pytestmark = pytest.mark.gpu

ERROR_NULL, ERROR_STATE, ERROR_DEVICE = 3, 101, 100
NODES = ar.NODES
ROUNDS = 4

params = ar.params
node_lp = ar.node_lp
round_cuts = ar.round_cuts
same_solution = ar.same_solution
solved_pair = ar.solved_pair

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


def compacted_state(state, n, mask):
    state = np.asarray(state, np.int8)
    return np.concatenate([state[:n], state[n:][~np.asarray(mask, bool)]])


def twin_delete(h, mask, state):
    """The contract's two steps on an engine handle or the oracle: the load of
    the reduced LP, then, if `state` (what the next solve would start from)
    has n + m entries, load_basis_state without the deleted rows' slacks."""
    lp = h.lp
    h.load(lp.without_rows(mask))
    if state is not None and len(state) == lp.n + lp.m:
        h.load_basis_state(compacted_state(state, lp.n, mask))


def basic_slack_cuts(state, n, m, first_cut_row):
    mask = np.zeros(m, bool)
    mask[first_cut_row:] = np.asarray(state)[n + first_cut_row:] == gc.BASIC
    return mask


def fresh_iterations(lp):
    fresh = engine.LpHandle(params())
    fresh.load(lp)
    rf = fresh.solve()
    fresh.close()
    assert rf.problem_status == abi.OPTIMAL
    return rf.iterations


def solve_and_compare(a, b, o, lp):
    ra, rb, ro = a.solve(), b.solve(), o.solve()
    same_solution(a, ra, b, rb)
    parity_util.compare(o, ro, a, ra, lp)
    assert bits(np.float64(ra.objective)) == bits(np.float64(ro.objective))
    return ra


def side_deletion(lp, state, mask):
    """A, B and the oracle loaded from the round's LP and state, the deletion
    on each, one solve: agreement, and fewer iterations than a fresh handle."""
    a, b, o = engine.LpHandle(params()), engine.LpHandle(params()), oracle_lib.OracleLp(params())
    for h in (a, b, o):
        h.load(lp)
        h.load_basis_state(state)
        h.solve()
    # The state the next solve starts from is each handle's own final one.
    info = a.delete_rows(mask)
    assert info["path"] == 1 and info["rows"] == int(mask.sum())
    twin_delete(b, mask, b.state())
    twin_delete(o, mask, o.state())
    reduced = lp.without_rows(mask)
    ra = solve_and_compare(a, b, o, reduced)
    assert ra.problem_status == abi.OPTIMAL
    fresh = fresh_iterations(reduced)
    assert ra.iterations < fresh, (ra.iterations, fresh)
    a.close()
    b.close()


@pytest.mark.parametrize("name", NODES)
def test_purge_loop_equals_reloads_and_the_oracle_and_stays_warm(name):
    lp, ycols, unit = node_lp(name)
    m0 = lp.m
    o, ro, a, ra = parity_util.solve_both(lp, params(), lambda q: engine.LpHandle(q))
    parity_util.compare(o, ro, a, ra, lp)
    b = engine.LpHandle(params())
    b.load(lp)
    same_solution(a, ra, b, b.solve())
    for rnd in range(ROUNDS):
        rows = round_cuts(o, lp, ycols, unit)
        assert a.add_rows(*rows)["path"] == 1, rnd
        lp = lp.with_rows(*rows)
        b.load(lp)
        o.load(lp)
        ra = solve_and_compare(a, b, o, lp)
        assert ra.problem_status == abi.OPTIMAL, (rnd, ra.problem_status)
        state = np.asarray(a.state(), np.int8)
        # The purge: the rule of cpsat.purge_cuts.
        mask = basic_slack_cuts(state, lp.n, lp.m, m0)
        assert mask.any(), rnd
        info = a.delete_rows(mask)
        assert info["path"] == 1 and info["rows"] == int(mask.sum()), (rnd, info)
        assert 1 <= info["bytes_up"] <= lp.m + 64
        twin_delete(b, mask, state)
        twin_delete(o, mask, state)
        lp = lp.without_rows(mask)
        assert a.lp.m == lp.m and np.array_equal(a.lp.row_idx, lp.row_idx)
        kept_state = compacted_state(state, lp.n, mask)
        ra = solve_and_compare(a, b, o, lp)
        assert (ra.problem_status, ra.iterations) == (abi.OPTIMAL, 0), (rnd, ra.iterations)
        assert np.array_equal(a.state(), kept_state), rnd
        fresh = fresh_iterations(lp)
        assert ra.iterations < fresh, (rnd, ra.iterations, fresh)
    a.close()
    b.close()


@functools.lru_cache(maxsize=None)
def add_only_rounds(name):
    """Three rounds of add the round's cuts and solve, on the oracle alone and
    with nothing deleted: (rows of the LP without cuts, [(the round's LP, its
    final state)])."""
    lp, ycols, unit = node_lp(name)
    m0 = lp.m
    o = oracle_lib.OracleLp(params())
    o.load(lp)
    o.solve()
    out = []
    for _ in range(3):
        lp = lp.with_rows(*round_cuts(o, lp, ycols, unit))
        o.load(lp)
        assert o.solve().problem_status == abi.OPTIMAL
        out.append((lp, np.asarray(o.state(), np.int8)))
    return m0, out


DELETIONS = {
    "all_cuts": lambda originals, basic_cuts: ~originals,
    "old_rows": lambda originals, basic_cuts: originals & (np.arange(len(originals)) % 7 == 0),
    "mixed": lambda originals, basic_cuts:
        (originals & (np.arange(len(originals)) % 11 == 0)) | basic_cuts,
}


@pytest.mark.parametrize("what", DELETIONS)
@pytest.mark.parametrize("rnd", range(3))
@pytest.mark.parametrize("name", NODES)
def test_other_deletions_equal_reloads_and_the_oracle_and_stay_warm(name, rnd, what):
    m0, rounds = add_only_rounds(name)
    lp, state = rounds[rnd]
    mask = DELETIONS[what](np.arange(lp.m) < m0, basic_slack_cuts(state, lp.n, lp.m, m0))
    assert mask.any() and not mask.all()
    side_deletion(lp, state, mask)


@pytest.fixture(scope="module")
def purged():
    """ft06 with one round of cuts added and solved: (the LP with the cuts, the
    purge mask, unit, ycols, A purged and solved, B reloaded and solved, the
    LP without any cut, the cuts' rows)."""
    lp, ycols, unit = node_lp("ft06")
    o = oracle_lib.OracleLp(params())
    o.load(lp)
    o.solve()
    rows = round_cuts(o, lp, ycols, unit)
    ext = lp.with_rows(*rows)
    a, b = solved_pair(ext)
    state = np.asarray(a.state(), np.int8)
    mask = basic_slack_cuts(state, ext.n, ext.m, lp.m)
    assert mask.any()
    a.delete_rows(mask)
    twin_delete(b, mask, state)
    same_solution(a, a.solve(), b, b.solve())
    yield ext, mask, unit, ycols, a, b, lp, rows
    a.close()
    b.close()


def test_panel_calls_after_a_delete_equal_the_reloads(purged):
    ext, mask, unit, ycols, a, b, _, _ = purged
    lp = ext.without_rows(mask)
    rng = np.random.default_rng(3)
    rows = [0, lp.m - 1, lp.m // 2, 5]
    x = rng.uniform(-1.0, 1.0, (3, lp.n + lp.m))
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
        "gomory_cuts": lambda h: h.gomory_cuts(cols, unit, ar.ZERO_TOLERANCE, ar.DROP_TOLERANCE),
    }
    for what, call in calls.items():
        got, want = flat(call(a)), flat(call(b))
        assert len(got) == len(want) > 0, what
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), what


def test_a_delete_forgets_the_stores_and_refuses_the_getters(purged):
    ext, mask, unit, ycols, _, _, _, _ = purged
    a, b = solved_pair(ext)
    state = np.asarray(a.state())
    xa = np.asarray(a.primal())
    f = xa[ycols] - np.floor(xa[ycols])
    cols = [int(c) for c, fc in zip(ycols, f) if 1e-6 < fc < 1 - 1e-6 and state[c] == gc.BASIC]
    assert cols
    room = len(cols) * ext.n
    store_cols, store_vals = np.zeros(room, np.int32), np.zeros(room, np.float64)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for h in (a, b):
        h.gomory_cuts(cols, unit, ar.ZERO_TOLERANCE, ar.DROP_TOLERANCE)  # fills the cut store
        assert h._L.mi_lp_get_cut_rows(h.h, p(store_cols), p(store_vals)) == 0
    a.delete_rows(mask)
    twin_delete(b, mask, state)
    out = np.zeros(ext.n)
    for h in (a, b):
        assert h._L.mi_lp_get_primal(h.h, p(out)) == ERROR_STATE
        assert h._L.mi_lp_get_cut_rows(h.h, p(store_cols), p(store_vals)) == ERROR_STATE
    same_solution(a, a.solve(), b, b.solve())
    a.close()
    b.close()


def test_sequences_equal_their_load_twins(purged):
    ext, mask, _, _, _, _, lp, rows = purged
    k = len(rows[0]) - 1
    cuts = np.arange(ext.m) >= lp.m
    # Before the first solve: no device matrix yet, and no state.
    a, b = engine.LpHandle(params()), engine.LpHandle(params())
    a.load(ext)
    info = a.delete_rows(mask)
    assert info["path"] == 0 and info["rows"] == int(mask.sum()) and info["bytes_up"] == 0
    b.load(ext)
    twin_delete(b, mask, None)
    same_solution(a, a.solve(), b, b.solve())
    # After load_basis_state: that state is the one that loses its slacks.
    for h in (a, b):
        h.load(ext)
        h.solve()
    given = np.asarray(a.state(), np.int8).copy()
    first_cut_slack = ext.n + lp.m
    given[first_cut_slack:] = np.where(given[first_cut_slack:] == gc.BASIC, gc.BASIC,
                                       abi.AT_LOWER_BOUND)
    a.load_basis_state(given)
    b.load_basis_state(given)
    assert a.delete_rows(mask)["path"] == 1
    twin_delete(b, mask, given)
    same_solution(a, a.solve(), b, b.solve())
    # Two deletes in a row: some original rows, then what is left of the cuts.
    state = np.asarray(a.state(), np.int8)
    now = a.lp
    first = np.zeros(now.m, bool)
    first[[0, 7, lp.m - 1]] = True
    assert a.delete_rows(first)["path"] == 1
    twin_delete(b, first, state)
    state = compacted_state(state, now.n, first)
    second = np.arange(a.lp.m) >= lp.m - 3
    assert second.any() and a.delete_rows(second)["path"] == 1
    twin_delete(b, second, state)
    assert a.lp.m == lp.m - 3
    same_solution(a, a.solve(), b, b.solve())
    # An append, then exactly the appended rows go: the LP of the last solve.
    state = np.asarray(a.state(), np.int8)
    base = a.lp
    short = (rows[0], rows[1], rows[2], rows[3], rows[4])
    assert a.add_rows(*short)["path"] == 1
    appended = np.arange(base.m + k) >= base.m
    assert a.delete_rows(appended)["path"] == 1
    b.load(base.with_rows(*short))
    twin_delete(b, appended, state)  # n + m entries of the LP before the append: (1) alone
    same_solution(a, a.solve(), b, b.solve())
    # Delete d rows, then append d rows: the row count is that of the last solve.
    state = np.asarray(a.state(), np.int8)
    gone = np.zeros(base.m, bool)
    gone[:k] = True
    assert a.delete_rows(gone)["path"] == 1
    assert a.add_rows(*short)["path"] == 1 and a.lp.m == base.m
    twin_delete(b, gone, state)
    b.load(b.lp.with_rows(*short))
    same_solution(a, a.solve(), b, b.solve())
    # A delete, then bounds, then a solve.
    state = np.asarray(a.state(), np.int8)
    now = a.lp
    lb, ub = np.array(now.col_lb), np.array(now.col_ub)
    ub[:3] = np.minimum(ub[:3], lb[:3] + 1.0)
    last = np.arange(now.m) >= now.m - 2
    assert a.delete_rows(last)["path"] == 1
    a.set_variable_bounds(lb, ub)
    twin_delete(b, last, state)
    b.set_variable_bounds(lb, ub)
    same_solution(a, a.solve(), b, b.solve())
    # A delete, then the load of a different LP (here: the LP of the last
    # solve again, and then the LP without any cut).
    state = np.asarray(a.state(), np.int8)
    now = a.lp
    some = np.arange(now.m) % 5 == 1
    a.delete_rows(some)
    twin_delete(b, some, state)
    a.load(now)
    b.load(now)
    same_solution(a, a.solve(), b, b.solve())
    state = np.asarray(a.state(), np.int8)
    a.delete_rows(some)
    twin_delete(b, some, state)
    a.load(lp)
    b.load(lp)
    same_solution(a, a.solve(), b, b.solve())
    # An empty mask is the load of the same LP, with the state loaded again:
    # getters are refused until the next solve.
    state = np.asarray(a.state(), np.int8)
    none = np.zeros(lp.m, bool)
    info = a.delete_rows(none)
    assert (info["rows"], info["entries"]) == (0, 0) and a.lp.m == lp.m
    out = np.zeros(lp.n)
    assert a._L.mi_lp_get_primal(a.h, out.ctypes.data_as(ctypes.c_void_p)) == ERROR_STATE
    twin_delete(b, none, state)
    same_solution(a, a.solve(), b, b.solve())
    # The last row goes and comes back: the LP of the last solve again, which
    # the twin's compare finds unchanged.
    state = np.asarray(a.state(), np.int8)
    last = np.arange(lp.m) == lp.m - 1
    entry_cols = np.repeat(np.arange(lp.n), np.diff(lp.col_starts))
    in_last = lp.row_idx == lp.m - 1
    back = (np.array([0, in_last.sum()], np.int64), entry_cols[in_last].astype(np.int32),
            lp.vals[in_last], lp.row_lb[-1:], lp.row_ub[-1:])
    assert a.delete_rows(last)["path"] == 1 and a.add_rows(*back)["path"] == 1
    assert np.array_equal(a.lp.row_idx, lp.row_idx) and np.array_equal(a.lp.vals, lp.vals)
    twin_delete(b, last, state)
    b.load(b.lp.with_rows(*back))
    same_solution(a, a.solve(), b, b.solve())
    a.close()
    b.close()


def test_delete_rows_takes_a_mask_or_indices():
    lp, _, _ = node_lp("random_6_4_7")
    a, b = solved_pair(lp)
    state = np.asarray(b.state(), np.int8)
    for bad in ([lp.m], [-1], [3, 3], [2.7], np.zeros(lp.m + 1, bool)):
        with pytest.raises(ValueError):
            a.delete_rows(bad)
    info = a.delete_rows([5, 2, lp.m - 1])
    assert info["path"] == 1 and info["rows"] == 3
    mask = np.zeros(lp.m, bool)
    mask[[2, 5, lp.m - 1]] = True
    twin_delete(b, mask, state)
    assert np.array_equal(a.lp.row_idx, b.lp.row_idx) and a.lp.m == b.lp.m
    same_solution(a, a.solve(), b, b.solve())
    a.close()
    b.close()


def test_a_mask_over_every_row_is_the_load_of_the_lp_without_rows():
    lp, _, _ = node_lp("random_6_4_7")
    a, b = solved_pair(lp)
    state = np.asarray(b.state(), np.int8)
    everything = np.ones(lp.m, bool)
    info = a.delete_rows(everything)
    assert (info["path"], info["rows"], info["entries"]) == (2, lp.m, len(lp.row_idx))
    twin_delete(b, everything, state)
    assert a.lp.m == b.lp.m == 0
    out = np.zeros(lp.n)
    for h in (a, b):  # refused until the next solve, as after a load
        assert h._L.mi_lp_get_primal(h.h, out.ctypes.data_as(ctypes.c_void_p)) == ERROR_STATE
    # Rows come back onto it as onto its twin, and the solve is the twin's.
    entry_cols = np.repeat(np.arange(lp.n), np.diff(lp.col_starts))
    first = lp.row_idx == 0
    back = (np.array([0, first.sum()], np.int64), entry_cols[first].astype(np.int32),
            lp.vals[first], lp.row_lb[:1], lp.row_ub[:1])
    a.add_rows(*back)
    b.load(b.lp.with_rows(*back))
    ra, rb = a.solve(), b.solve()
    assert ra.error_code == 0
    same_solution(a, ra, b, rb)
    a.close()
    b.close()


def test_error_table_changes_nothing():
    lp, _, _ = node_lp("random_6_4_7")
    a, b = solved_pair(lp)
    mask = np.zeros(lp.m, np.uint8)
    mask[3] = 1
    fresh = engine.LpHandle(params())
    raw = lambda h, m: h._L.mi_lp_delete_rows(  # noqa: E731
        h.h, None if m is None else m.ctypes.data_as(ctypes.c_void_p), None)
    assert raw(fresh, mask) == ERROR_STATE  # before a load
    fresh.close()
    assert a._L.mi_lp_delete_rows(None, mask.ctypes.data_as(ctypes.c_void_p), None) == ERROR_NULL
    assert raw(a, None) == ERROR_NULL
    a.begin(0)  # a begun solve, parked at its first iteration
    assert raw(a, mask) == ERROR_STATE
    same_solution(a, a.finish(), b, b.solve())
    assert a.lp.m == lp.m
    same_solution(a, a.solve(), b, b.solve())
    a.close()
    b.close()


def test_column_shards_take_the_full_upload(purged, monkeypatch):
    ext, mask, _, _, _, _, _, _ = purged
    monkeypatch.setenv("MILP_SHARDS", "2")
    s, t = solved_pair(ext)
    state = np.asarray(t.state(), np.int8)
    assert s.delete_rows(mask)["path"] == 2
    twin_delete(t, mask, state)
    rs, rt = s.solve(), t.solve()
    assert rs.problem_status == abi.OPTIMAL
    same_solution(s, rs, t, rt)
    s.close()
    t.close()


def test_batch_solve_bounds_over_workers_that_deleted(purged):
    ext, mask, _, _, solved, _, _, _ = purged
    red = ext.without_rows(mask)
    # Every child starts from the purged node's state, whichever worker takes it.
    warm = np.asarray(solved.state(), np.int8)
    workers = {"deleted": [], "loaded": []}
    for _ in range(2):
        a, b = solved_pair(ext)
        state = np.asarray(b.state(), np.int8)
        a.delete_rows(mask)
        twin_delete(b, mask, state)
        workers["deleted"].append(a)
        workers["loaded"].append(b)
    rng = np.random.default_rng(5)
    count = 6
    lbs = np.tile(red.col_lb, (count, 1))
    ubs = np.tile(red.col_ub, (count, 1))
    for i in range(count):
        c = rng.integers(0, red.n)
        ubs[i, c] = min(ubs[i, c], lbs[i, c] + 1.0)
    out = {key: engine.batch_solve_bounds(w, lbs, ubs, warm) for key, w in workers.items()}
    for ra, rb in zip(out["deleted"], out["loaded"]):
        assert (ra.error_code, ra.problem_status, ra.iterations) == \
            (rb.error_code, rb.problem_status, rb.iterations)
        assert bits(np.float64(ra.objective)) == bits(np.float64(rb.objective))
    for w in workers["deleted"] + workers["loaded"]:
        w.close()


class OracleWithCutsAndPurge(ar.OracleWithCuts):
    """The oracle handle with the call it lacks: the delete by its twin."""

    def delete_rows(self, mask):
        # LpConstraint.solve_lp has told the solver that the matrix stays.
        self.notify_matrix_changed()
        twin_delete(self, np.asarray(mask, bool), np.asarray(self.state(), np.int8))
        return None


def test_cpsat_purge_cuts_on_the_oracle_and_on_the_engine():
    lp, ycols = jobshop.relaxation(jobshop.random_instance(6, 4, 7))
    out = []
    for handle in (OracleWithCutsAndPurge(params()), engine.LpHandle(params())):
        c = cpsat.LpConstraint(lp, ycols, handle)
        t = cpsat.IntegerTrail(lp.col_lb, lp.col_ub)
        assert c.solve_lp(t) and c.analyze_lp(t)
        cols = cpsat.fractional_columns(c.lp_solution, ycols, limit=20)
        cuts = cpsat.gomory_cuts(c, c.lp_solution, cols)
        cpsat.add_cuts(c, cuts)
        assert c.solve_lp(t)
        deleted, info = cpsat.purge_cuts(c, lp.m)
        assert c.lp.m == lp.m + len(cuts) - len(deleted) and c.lp is c.lp_data
        assert c.h.lp.m == c.lp.m and (deleted >= lp.m).all()
        assert c.solve_lp(t)
        out.append((deleted.tolist(), c.last.problem_status, c.last.iterations,
                    np.asarray(c.lp_solution, np.float64), info))
    (do, so, io, xo, _), (dg, sg, ig, xg, info) = out
    assert (do, so, io) == (dg, sg, ig) and len(do) > 0
    assert np.array_equal(bits(xo), bits(xg))
    assert info["path"] == 1 and info["rows"] == len(dg)
