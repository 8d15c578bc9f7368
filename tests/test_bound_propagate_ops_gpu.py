"""DeviceLp::BoundPropagatePanel(From) and BoundPropagatedColumnsFrom through
the probe (tests/devop_bound_propagate.py), against the numpy reference of
tests/bound_propagate_cases.py. Every comparison is on all 64 bits, NaNs
included, and every case asserts its record (last_bound_propagate: the column
shape that ran, the width, the rounds launched, kept, bytes): the rounds
launched are the sum over the panels of the largest `rounds` of the panel's
sets, which shows the early exit and that no round is launched after it.

The hand cases and the node cases run under MILP_IMPLIED_COLUMNS=short and
long, at every k of bound_propagate_cases.KS, in the dense and the override
form, with lists and with summaries only, at every max_rounds.
tests/test_bound_propagate_ref_cpu.py shows that these inputs hold the cases
they are there for. Then: a set alone against the same set inside k = 16 and
17, the pool's special children, own bounds that cross without a move, a
capacity one entry short, and one handle that alternates this call with the
tightened columns, ranges, violations and column dots, unsplit and with two
column shards.
"""
import functools

import numpy as np
import pytest

import bound_implied_cases as ic
import bound_propagate_cases as pc
import bound_range_cases as bc
import devop
import devop_bound_propagate as dbp
import row_panel_cases as rc
import row_violation_cases as vc
import solveops_cases as sc
from device_ref import bits, column_scalar_products

pytestmark = pytest.mark.gpu

SWITCHES = ("MILP_DENSE_BLOCK", "MILP_SHARDS", "MILP_SHARD_DEVICES", "MILP_SMALL_FUSED",
            "MILP_SMALL_BATCH", "MILP_ROWWISE_LIST", "MILP_MEDIUM", "MILP_FULL_ROWS",
            "MILP_DENSE_UNROLL", "MILP_EARLY_FLIPS", "MILP_IMPLIED_COLUMNS")
SHAPES = {"short": dbp.SHORT_COLUMNS, "long": dbp.LONG_COLUMNS}
HAND = ("chain", "halving", "knapsack", "negzero")
COL_SENTINEL = np.int32(-77)
VALUE_SENTINEL = np.float64(-7.25)


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
    yield
    _cached_handle.cache_clear()


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A device error is never part of a test here: after one, nothing more
    is started on the GPU."""
    yield
    if devop.device_error is not None:
        pytest.exit(f"device error: {devop.device_error}", returncode=3)


def matrix(name):
    return pc.hand(name)[0] if name in HAND else ic.matrix(name)


@functools.lru_cache(maxsize=None)
def _cached_handle(name, env):
    mat = matrix(name)
    return dbp.BoundPropagateDevOp(mat.m, mat.n, mat.col_starts, mat.row_idx, mat.vals)


def handle(name, env, monkeypatch, cached=True):
    """The MILP_* switches are read when a handle is created;
    MILP_IMPLIED_COLUMNS at every call, and stays set for the test."""
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    make = _cached_handle if cached else _cached_handle.__wrapped__
    shared = {key: value for key, value in env.items() if key != "MILP_IMPLIED_COLUMNS"}
    return make(name, tuple(sorted(shared.items())))


def own_shape(name):
    mat = matrix(name)
    long_columns = int(mat.col_starts[-1]) / mat.n >= ic.LONG_COLUMNS_FROM
    return dbp.LONG_COLUMNS if long_columns else dbp.SHORT_COLUMNS


def record(name, columns, summaries, integers, lists=None, kept=0, sets=None):
    """The record of a call whose reference summaries are `summaries`. lists:
    None for the dense results, else whether lists were built."""
    mat = matrix(name)
    k = len(summaries)
    rounds = down = 0
    for first, kp in rc.panels(k):
        s = summaries[first:first + kp]
        rounds += int(s["rounds"].max())
        again = bool(((s["status"] == pc.INFEASIBLE) & (s["rounds"] == 1)).any())
        down += 24 * kp * (int(s["rounds"].max()) + again)
    up = 16 * mat.m + (mat.n if integers else 0)
    if sets is None:
        up += 16 * k * mat.n
    else:
        up += 16 * mat.n + 20 * sum(len(c) for c, _, _ in sets) + 8 * (k + 1)
    if lists is None:
        down += 16 * k * mat.n
    else:
        down += (20 * kept + 32 * k) if lists else 24 * k
    return {"panels": len(rc.panels(k)), "width": rc.width(rc.panels(k)[-1][1]),
            "columns": columns, "lists": bool(lists), "rounds": rounds, "kept": kept,
            "bytes_up": up, "bytes_down": down}


def dense_buffers(k, n):
    s = np.zeros(k + 1, dbp.SUMMARY)
    s["rounds"][k], s["worst"][k] = -5, -7.25
    return {"new_lbs": np.full(k * n + 1, VALUE_SENTINEL),
            "new_ubs": np.full(k * n + 1, VALUE_SENTINEL), "summaries": s}


def check_dense_sentinels(buffers, k, n, what):
    assert bits(buffers["new_lbs"][k * n]) == bits(buffers["new_ubs"][k * n]) == \
        bits(VALUE_SENTINEL), what
    assert buffers["summaries"]["rounds"][k] == -5 and buffers["summaries"]["worst"][k] == -7.25


def list_buffers(k, kept):
    s = np.zeros(k + 1, dbp.SUMMARY)
    s["rounds"][k], s["worst"][k] = -5, -7.25
    return {"col_starts": np.full(k + 2, -5, np.int64), "cols": np.full(kept + 1, COL_SENTINEL),
            "new_lbs": np.full(kept + 1, VALUE_SENTINEL),
            "new_ubs": np.full(kept + 1, VALUE_SENTINEL), "summaries": s}


def check_list_sentinels(buffers, k, kept, what):
    assert buffers["col_starts"][k + 1] == -5, what
    assert buffers["cols"][kept] == COL_SENTINEL, what
    assert bits(buffers["new_lbs"][kept]) == bits(buffers["new_ubs"][kept]) == \
        bits(VALUE_SENTINEL), what
    assert buffers["summaries"]["rounds"][k] == -5 and buffers["summaries"]["worst"][k] == -7.25


def all_forms(d, name, columns, base_lb, base_ub, sets, row_lb, row_ub, is_integer, tol,
              max_rounds, want, what):
    """The dense form, the override form, the lists and the summaries only of
    one (sets, parameters), against the dense reference result `want`."""
    k, n = len(sets), d.n
    integers = is_integer is not None
    L, U = bc.materialise(base_lb, base_ub, sets)
    rounds = (is_integer, tol, pc.ITOL, max_rounds)
    buffers = dense_buffers(k, n)
    got = d.bound_propagate_panel(L, U, row_lb, row_ub, *rounds, buffers=buffers)
    p = d.last_bound_propagate()
    print(what, p, want[2]["rounds"].tolist())
    pc.same_result(got, want, what + " dense")
    assert p == record(name, columns, want[2], integers), (what, p)
    check_dense_sentinels(buffers, k, n, what)
    flat = bc.flatten(sets)
    buffers = dense_buffers(k, n)
    got = d.bound_propagate_panel_from(base_lb, base_ub, *flat, row_lb, row_ub, *rounds,
                                       buffers=buffers)
    pc.same_result(got, want, what + " override")
    assert d.last_bound_propagate() == record(name, columns, want[2], integers, sets=sets), what
    check_dense_sentinels(buffers, k, n, what)
    lists = pc.list_result(want, base_lb, base_ub, tol)
    kept = int(lists[0][k])
    buffers = list_buffers(k, kept)
    got = d.bound_propagated_columns_from(base_lb, base_ub, *flat, row_lb, row_ub, *rounds,
                                          buffers=buffers)
    pc.same_lists(got, lists, what + " lists")
    assert d.last_bound_propagate() == record(name, columns, want[2], integers, lists=True,
                                              kept=kept, sets=sets), what
    check_list_sentinels(buffers, k, kept, what)
    got = d.bound_propagated_columns_from(base_lb, base_ub, *flat, row_lb, row_ub, *rounds,
                                          lists=False)
    assert got[:4] == (None, None, None, None)
    pc.same_summaries(got[4], lists[4], what + " summaries only")
    assert d.last_bound_propagate() == record(name, columns, want[2], integers, lists=False,
                                              sets=sets), what


def dense_as_overrides(L, U):
    """The sets as overrides of set 0."""
    sets = []
    for j in range(L.shape[0]):
        cols = np.nonzero((bits(L[j]) != bits(L[0])) | (bits(U[j]) != bits(U[0])))[0]
        cols = cols.astype(np.int32)
        sets.append((cols, L[j, cols], U[j, cols]))
    return L[0], U[0], sets


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name", HAND)
def test_hand_cases(name, shape, monkeypatch):
    d = handle(name, {"MILP_IMPLIED_COLUMNS": shape}, monkeypatch)
    mat, L, U, row_lb, row_ub, ints = pc.hand(name)
    base_lb, base_ub, sets = dense_as_overrides(L, U)
    for tol, max_rounds in ((0.0, 1), (0.0, 8), (0.0, 40), (0.375, 8), (1e-9, 100)):
        for is_integer in ((ints, None) if ints is not None else (None,)):
            want = pc.propagate(mat, L, U, row_lb, row_ub, is_integer, tol, pc.ITOL, max_rounds)
            what = f"{name} {shape} tol={tol} R={max_rounds} ints={is_integer is not None}"
            all_forms(d, name, SHAPES[shape], base_lb, base_ub, sets, row_lb, row_ub, is_integer,
                      tol, max_rounds, want, what)
    if name == "chain":  # the figures of the issue, from the GPU
        NL, NU, s = d.bound_propagate_panel(L, U, row_lb, row_ub, None, 0.0, 0.0, 40)
        assert s["status"].tolist() == [pc.FIXPOINT, pc.FIXPOINT, pc.INFEASIBLE, pc.INFEASIBLE]
        assert s["rounds"].tolist() == [12, 12, 6, 3] and s["moves"].tolist() == [102, 102, 72, 36]
        assert s["worst"].tolist() == [0.0, 0.0, 1.0, 1.0]
        assert s["worst_col"].tolist() == [-1, -1, 5, 3]
        assert NL[0].tolist() == NL[1].tolist() == NU[1].tolist() == list(range(12))
        assert d.last_bound_propagate()["rounds"] == 12  # one panel: its slowest set
    if name == "negzero":
        NL, NU, s = d.bound_propagate_panel(L, U, row_lb, row_ub, ints, 0.0, pc.ITOL, 8)
        assert bits(NL[0, 0]) == bits(np.float64(0.0))


CASE_KS = [(name, k) for name in pc.CASES for k in pc.KS]


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name,k", CASE_KS)
def test_node_cases(name, k, shape, monkeypatch):
    d = handle(name, {"MILP_IMPLIED_COLUMNS": shape}, monkeypatch)
    for f, tol, integers in pc.grid(name):
        base_lb, base_ub, sets, row_lb, row_ub = pc.node(name, f)
        is_integer = pc.integer_columns(name) if integers else None
        for max_rounds in pc.ROUNDS:
            want = pc.expected(name, f, tol, integers, max_rounds, k)
            what = f"{name} k={k} {shape} f={f} tol={tol} ints={integers} R={max_rounds}"
            all_forms(d, name, SHAPES[shape], base_lb, base_ub, sets[:k], row_lb, row_ub,
                      is_integer, tol, max_rounds, want, what)


@pytest.mark.parametrize("name", pc.CASES)
def test_a_set_alone_has_the_bits_it_has_among_sixteen_and_seventeen(name, monkeypatch):
    d = handle(name, {}, monkeypatch)
    f, tol, integers = pc.grid(name)[-1]
    base_lb, base_ub, sets, row_lb, row_ub = pc.node(name, f)
    is_integer = pc.integer_columns(name) if integers else None
    L, U = bc.materialise(base_lb, base_ub, sets)
    rounds = (is_integer, tol, pc.ITOL, 30)
    together = {k: d.bound_propagate_panel(L[:k], U[:k], row_lb, row_ub, *rounds)
                for k in (16, 17)}
    assert d.last_bound_propagate()["columns"] == own_shape(name)
    for j in (0, 1, 7, 15, 16):
        alone = d.bound_propagate_panel(L[j:j + 1], U[j:j + 1], row_lb, row_ub, *rounds)
        assert d.last_bound_propagate()["rounds"] == alone[2]["rounds"][0]
        for k, (NL, NU, s) in together.items():
            if j < k:
                pc.same_result(alone, (NL[j:j + 1], NU[j:j + 1], s[j:j + 1]), f"{name} {j} in {k}")


@pytest.mark.parametrize("which", ic.ROW_BOUND_SETS)
@pytest.mark.parametrize("name", pc.CASES)
def test_special_children(name, which, monkeypatch):
    """A NaN own bound, l = +inf, +-2^1023 and the box, under the row-bound
    sets of the implied-bound tests, three rounds, with integer columns."""
    d = handle(name, {}, monkeypatch)
    L, U = ic.pool(name)
    k = 8
    row_lb, row_ub = ic.row_bounds(name, which)
    want = pc.special_reference(name, which)
    base_lb, base_ub, sets = ic.pool_as_overrides(name, k)
    all_forms(d, name, own_shape(name), base_lb, base_ub, sets, row_lb, row_ub,
              pc.integer_columns(name), 0.0, 3, want, f"{name} special {which}")


@pytest.mark.parametrize("name", ("steps", "rows70"))
def test_own_bounds_that_cross_without_a_move(name, monkeypatch):
    """The second count of round 1: moves leaves out the column that crosses
    without having moved."""
    d = handle(name, {}, monkeypatch)
    f, tol, integers = pc.grid(name)[0]
    base_lb, base_ub, _, row_lb, row_ub = pc.node(name, f)
    sets, column = pc.own_crossing(name)
    want = pc.own_crossing_reference(name)
    assert want[2]["status"][2] == pc.INFEASIBLE and want[2]["rounds"][2] == 1
    all_forms(d, name, own_shape(name), base_lb, base_ub, sets, row_lb, row_ub,
              pc.integer_columns(name) if integers else None, tol, 5, want, f"{name} own crossing")


def test_capacity_one_short(monkeypatch):
    name, k = "rows70", 17
    d = handle(name, {}, monkeypatch)
    f, tol, integers = pc.grid(name)[1]
    base_lb, base_ub, sets, row_lb, row_ub = pc.node(name, f)
    args = (base_lb, base_ub, *bc.flatten(sets[:k]), row_lb, row_ub,
            pc.integer_columns(name) if integers else None, tol, pc.ITOL, 30)
    want = pc.expected_lists(name, f, tol, integers, 30, k)
    kept = int(want[0][k])
    assert kept > 1
    buffers = list_buffers(k, kept)
    before = {key: value.copy() for key, value in buffers.items()}
    with pytest.raises(dbp.CapacityError) as e:
        d.bound_propagated_columns_from(*args, capacity=kept - 1, buffers=buffers)
    assert str(kept) in str(e.value)
    for key in buffers:
        assert buffers[key].tobytes() == before[key].tobytes(), key
    assert devop.device_error is None
    got = d.bound_propagated_columns_from(*args, capacity=kept, buffers=buffers)
    pc.same_lists(got, want, "exact capacity")


@pytest.mark.parametrize("env", ({}, {"MILP_SHARDS": "2"}), ids=("unsplit", "two_shards"))
def test_one_handle_alternates_every_role(env, monkeypatch):
    """One fresh handle alternates the propagation with the tightened columns,
    ranges, screening, violations and column dots: `implied` grows to four
    blocks under the new role and shrinks to nothing less for the older ones,
    and every older record stays as its own call left it."""
    name = "rows70"
    mat = bc.matrix(name)
    d = handle(name, env, monkeypatch, cached=False)
    try:
        L, U = ic.pool(name)
        pts = rc.points(name)
        y = sc.vector_pool(name)
        dots = np.stack([column_scalar_products(mat, np.arange(mat.N), v) for v in y[:5]])

        def older_records():
            return (d.last_bound_implied(), d.last_bound_ranges(), d.last_row_violations(),
                    d.last_row_panel())

        def propagate(k, entry, max_rounds, lists):
            before = older_records()
            f, tol, integers = pc.grid(name)[entry]
            base_lb, base_ub, sets, row_lb, row_ub = pc.node(name, f)
            is_integer = pc.integer_columns(name) if integers else None
            want = pc.expected(name, f, tol, integers, max_rounds, k)
            if lists:
                got = d.bound_propagated_columns_from(base_lb, base_ub, *bc.flatten(sets[:k]),
                                                      row_lb, row_ub, is_integer, tol, pc.ITOL,
                                                      max_rounds)
                pc.same_lists(got, pc.list_result(want, base_lb, base_ub, tol),
                              f"propagated k={k}")
            else:
                got = d.bound_propagate_panel(*bc.materialise(base_lb, base_ub, sets[:k]), row_lb,
                                              row_ub, is_integer, tol, pc.ITOL, max_rounds)
                pc.same_result(got, want, f"propagate k={k}")
            assert older_records() == before

        def tightened(k, tol):
            before = d.last_bound_propagate()
            want = ic.expected(name, "mid", k, tol)
            got = d.bound_tightened_panel(L[:k], U[:k], *ic.row_bounds(name, "mid"), tol)
            ic.same_lists(got, want, f"tightened k={k}")
            assert d.last_bound_propagate() == before

        def tightened_from(k):
            base_lb, base_ub, sets = ic.pool_as_overrides(name, k)
            NL, NU = ic.first(ic.reference(name, "mid"), k)
            want = ic.keep_reference(L[:k], U[:k], NL, NU, 0.0, base=(base_lb, base_ub))
            got = d.bound_tightened_panel_from(base_lb, base_ub, *bc.flatten(sets),
                                               *ic.row_bounds(name, "mid"), 0.0)
            ic.same_lists(got, want, f"tightened from k={k}")

        def ranges(k):
            before = d.last_bound_propagate()
            bc.same_ranges(d.bound_ranges_panel(L[:k], U[:k]), bc.first(bc.reference(name), k),
                           f"ranges k={k}")
            assert d.last_bound_propagate() == before

        def violations(k, which):
            got = d.row_violations_panel(pts[:k], *vc.bounds(name, which))
            vc.same_result(got, vc.expected(name, which, k), f"violations k={k} {which}")

        def column_dots():
            got = d.column_dots_panel(y[:5])
            assert np.array_equal(bits(got), bits(dots))

        for _ in range(2):
            propagate(1, 0, 30, False)
            ranges(2)
            tightened(33, 0.0)
            propagate(17, 1, 30, True)
            violations(2, "split")
            column_dots()
            tightened_from(17)
            propagate(16, 5, 3, True)
            tightened(5, 0.375)
            violations(33, "crossed")
            propagate(4, 7, 30, False)
            ranges(33)
    finally:
        d.close()
