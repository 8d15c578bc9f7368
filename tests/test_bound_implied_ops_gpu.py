"""DeviceLp::BoundImpliedPanel(From) and BoundTightenedPanel(From) through the
probe (tests/devop_bound_implied.py), against the numpy reference of
tests/bound_implied_cases.py (implied, keep_reference). Every comparison is on
all 64 bits, NaNs included, and every case asserts its record
(last_bound_implied: the column shape that ran, the width, kept, bytes).

rows70, steps, groups and wide run with k bound sets for every panel width,
for padding and for several panels, under MILP_IMPLIED_COLUMNS=short and
long (both kernel shapes on every matrix: columns of length 0 and 1 under
long, the full column under short) and under every row-bound set, in the
dense and in the override form; the lists at every tolerance.
tests/test_bound_implied_ref_cpu.py shows that these inputs hold the cases they
are there for. Then: the shape the engine takes by itself, override lists of
their own, summaries only, a capacity one entry short, and one handle that
alternates this call with ranges, violations and column dots, unsplit and with
two column shards.
"""
import functools

import numpy as np
import pytest

import bound_implied_cases as ic
import bound_range_cases as bc
import devop
import devop_bound_implied as dbi
import row_panel_cases as rc
import row_violation_cases as vc
import solveops_cases as sc
from device_ref import bits, column_scalar_products

pytestmark = pytest.mark.gpu

SWITCHES = ("MILP_DENSE_BLOCK", "MILP_SHARDS", "MILP_SHARD_DEVICES", "MILP_SMALL_FUSED",
            "MILP_SMALL_BATCH", "MILP_ROWWISE_LIST", "MILP_MEDIUM", "MILP_FULL_ROWS",
            "MILP_DENSE_UNROLL", "MILP_EARLY_FLIPS", "MILP_IMPLIED_COLUMNS")
SHAPES = {"short": dbi.SHORT_COLUMNS, "long": dbi.LONG_COLUMNS}
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


@functools.lru_cache(maxsize=None)
def _cached_handle(name, env):
    mat = ic.matrix(name)
    return dbi.BoundImpliedDevOp(mat.m, mat.n, mat.col_starts, mat.row_idx, mat.vals)


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
    return dbi.LONG_COLUMNS if ic.long_by_itself(name) else dbi.SHORT_COLUMNS


def shape_record(name, k, columns):
    return {"panels": len(rc.panels(k)), "width": rc.width(rc.panels(k)[-1][1]),
            "columns": columns}


def up_bytes(name, k, sets=None):
    mat = ic.matrix(name)
    return 16 * mat.m + (16 * k * mat.n if sets is None else ic.override_bytes(name, sets))


def dense_record(name, k, columns, sets=None):
    return dict(shape_record(name, k, columns), lists=False, kept=0,
                bytes_up=up_bytes(name, k, sets), bytes_down=16 * k * ic.matrix(name).n)


def list_record(name, k, columns, kept, lists=True, sets=None):
    return dict(shape_record(name, k, columns), lists=lists, kept=kept,
                bytes_up=up_bytes(name, k, sets),
                bytes_down=(20 * kept + 32 * k) if lists else 24 * k)


def sentinel_buffers(k, kept):
    summaries = np.zeros(k + 1, dbi.SUMMARY)
    summaries["count"][k], summaries["worst"][k], summaries["worst_row"][k] = -5, -7.25, -77
    return {"col_starts": np.full(k + 2, -5, np.int64), "cols": np.full(kept + 1, COL_SENTINEL),
            "new_lbs": np.full(kept + 1, VALUE_SENTINEL),
            "new_ubs": np.full(kept + 1, VALUE_SENTINEL), "summaries": summaries}


def check_sentinels(buffers, k, kept, what):
    assert buffers["col_starts"][k + 1] == -5, what
    assert buffers["cols"][kept] == COL_SENTINEL, what
    assert bits(buffers["new_lbs"][kept]) == bits(buffers["new_ubs"][kept]) == \
        bits(VALUE_SENTINEL), what
    s = buffers["summaries"][k]
    assert (s["count"], s["worst_row"]) == (-5, -77) and s["worst"] == -7.25, what


CASE_KS = [(name, k) for name in ic.CASES for k in ic.KS]


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name,k", CASE_KS)
def test_dense_bounds(name, k, shape, monkeypatch):
    """The dense form under every row-bound set and the override form of the
    same k bound sets, under a forced column shape, against the reference and
    against each other; one sentinel behind each output."""
    d = handle(name, {"MILP_IMPLIED_COLUMNS": shape}, monkeypatch)
    n = d.n
    L, U = ic.pool(name)
    for which in ic.ROW_BOUND_SETS:
        what = f"{name} k={k} {shape} {which}"
        lb, ub = ic.row_bounds(name, which)
        want = ic.first(ic.reference(name, which), k)
        buffers = {"new_lbs": np.full(k * n + 1, VALUE_SENTINEL),
                   "new_ubs": np.full(k * n + 1, VALUE_SENTINEL)}
        got = d.bound_implied_panel(L[:k], U[:k], lb, ub, buffers=buffers)
        p = d.last_bound_implied()
        print(what, p)
        ic.same_bounds(got, want, what)
        assert p == dense_record(name, k, SHAPES[shape]), (what, p)
        assert bits(buffers["new_lbs"][k * n]) == bits(buffers["new_ubs"][k * n]) == \
            bits(VALUE_SENTINEL), what
    base_lb, base_ub, sets = ic.pool_as_overrides(name, k)
    lb, ub = ic.row_bounds(name, "mid")
    over = d.bound_implied_panel_from(base_lb, base_ub, *bc.flatten(sets), lb, ub)
    ic.same_bounds(over, ic.first(ic.reference(name, "mid"), k), f"{name} k={k} overrides")
    assert d.last_bound_implied() == dense_record(name, k, SHAPES[shape], sets=sets)


@pytest.mark.parametrize("name", ic.CASES)
def test_shape_taken_by_itself(name, monkeypatch):
    """Without the switch, and with auto: long from 32 structural entries per
    structural column (wide), short below (the others)."""
    for env in ({}, {"MILP_IMPLIED_COLUMNS": "auto"}):
        d = handle(name, env, monkeypatch)
        L, U = ic.pool(name)
        got = d.bound_implied_panel(L[:5], U[:5], *ic.row_bounds(name, "mid"))
        ic.same_bounds(got, ic.first(ic.reference(name, "mid"), 5), name)
        assert d.last_bound_implied() == dense_record(name, 5, own_shape(name))
    assert {own_shape(n) for n in ic.CASES} == set(SHAPES.values())


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("which", bc.OVERRIDE_SETS)
@pytest.mark.parametrize("name", bc.CASES)
def test_override_sets(name, which, shape, monkeypatch):
    """Override lists of their own (a branching node, special values, a panel
    boundary): the override form equals the reference and the dense form on
    the materialised sets; its lists keep the changed columns too."""
    d = handle(name, {"MILP_IMPLIED_COLUMNS": shape}, monkeypatch)
    base_lb, base_ub, sets = bc.override_set(name, which)
    k = len(sets)
    flat = bc.flatten(sets)
    lb, ub = ic.row_bounds(name, "mid")
    L, U, NL, NU = ic.override_reference(name, which)
    what = f"{name} {which} {shape}"
    got = d.bound_implied_panel_from(base_lb, base_ub, *flat, lb, ub)
    ic.same_bounds(got, (NL, NU), what)
    assert d.last_bound_implied() == dense_record(name, k, SHAPES[shape], sets=sets)
    ic.same_bounds(d.bound_implied_panel(L, U, lb, ub), got, what + " against the dense form")
    for tol in ic.TOLERANCES:
        ref = ic.keep_reference(L, U, NL, NU, tol, base=(base_lb, base_ub))
        kept = int(ref[0][k])
        buffers = sentinel_buffers(k, kept)
        res = d.bound_tightened_panel_from(base_lb, base_ub, *flat, lb, ub, tol, capacity=kept,
                                           buffers=buffers)
        p = d.last_bound_implied()
        ic.same_lists(res, ref, what)
        check_sentinels(buffers, k, kept, what)
        assert p == list_record(name, k, SHAPES[shape], kept, sets=sets), (what, p)
        # Every overridden column is in its child's list, whether it moved or not.
        for j, (cols, lo, hi) in enumerate(sets):
            differs = (bits(lo) != bits(base_lb[cols])) | (bits(hi) != bits(base_ub[cols]))
            mine = res[1][res[0][j]:res[0][j + 1]]
            assert set(cols[differs].tolist()) <= set(mine.tolist()), (what, j)
        dense = d.bound_tightened_panel(L, U, lb, ub, tol)
        want = ic.keep_reference(L, U, NL, NU, tol)
        ic.same_lists(dense, want, what + " dense form")
        assert d.last_bound_implied() == list_record(name, k, SHAPES[shape], int(want[0][k]))


def summaries_from_lists(got, tol, what):
    """count = list length; worst and worst_row recomputed from the listed
    bounds alone."""
    starts, cols, lo, hi, summaries = got
    for j in range(len(summaries)):
        mine = cols[starts[j]:starts[j + 1]]
        with np.errstate(invalid="ignore", over="ignore"):
            cross = lo[starts[j]:starts[j + 1]] - hi[starts[j]:starts[j + 1]]
        assert summaries["count"][j] == len(mine), (what, j)
        assert np.all(np.diff(mine) > 0), (what, j)
        crossing = cross > tol
        if not crossing.any():
            assert summaries["worst_row"][j] == -1 and bits(summaries["worst"][j]) == 0, (what, j)
            continue
        worst = cross[crossing].max()
        assert bits(summaries["worst"][j]) == bits(worst), (what, j)
        assert summaries["worst_row"][j] == mine[np.nonzero(crossing & (cross == worst))[0][0]], \
            (what, j)


@pytest.mark.parametrize("name,k", CASE_KS)
def test_lists(name, k, monkeypatch):
    """k bound sets under every row-bound set and every tolerance: lists,
    summaries, sentinels, record; the shape the engine takes by itself, and at
    tolerance 0 the other one too. Then the override form of the same sets."""
    L, U = ic.pool(name)
    other = "short" if ic.long_by_itself(name) else "long"
    for env, columns in (({}, own_shape(name)), ({"MILP_IMPLIED_COLUMNS": other}, SHAPES[other])):
        d = handle(name, env, monkeypatch)
        for which in ic.ROW_BOUND_SETS:
            for tol in (ic.tolerances(name) if not env else (0.0,)):
                what = f"{name} k={k} {which} tol={tol!r} {columns}"
                want = ic.expected(name, which, k, tol)
                kept = int(want[0][k])
                buffers = sentinel_buffers(k, kept)
                got = d.bound_tightened_panel(L[:k], U[:k], *ic.row_bounds(name, which), tol,
                                              capacity=kept, buffers=buffers)
                p = d.last_bound_implied()
                print(what, p)
                ic.same_lists(got, want, what)
                check_sentinels(buffers, k, kept, what)
                assert p == list_record(name, k, columns, kept), (what, p)
                summaries_from_lists(got, tol, what)
    base_lb, base_ub, sets = ic.pool_as_overrides(name, k)
    NL, NU = ic.first(ic.reference(name, "mid"), k)
    for tol in ic.tolerances(name):
        want = ic.keep_reference(L[:k], U[:k], NL, NU, tol, base=(base_lb, base_ub))
        got = d.bound_tightened_panel_from(base_lb, base_ub, *bc.flatten(sets),
                                           *ic.row_bounds(name, "mid"), tol)
        ic.same_lists(got, want, f"{name} k={k} override form tol={tol!r}")
        assert d.last_bound_implied() == list_record(name, k, SHAPES[other], int(want[0][k]),
                                                     sets=sets)
    # Without finite row bounds a child's list is exactly what it changed: a
    # count > 0 beside worst_row == -1.
    want = ic.keep_reference(L[:k], U[:k], L[:k], U[:k], 0.0, base=(base_lb, base_ub))
    got = d.bound_tightened_panel_from(base_lb, base_ub, *bc.flatten(sets),
                                       *ic.row_bounds(name, "free"), 0.0)
    ic.same_lists(got, want, f"{name} k={k} override form, free rows")


@pytest.mark.parametrize("name,k", [("rows70", 17), ("groups", 5), ("wide", 33)])
def test_summaries_only(name, k, monkeypatch):
    """The same summaries, 24 bytes per child down, and what an earlier call
    returned is untouched."""
    d = handle(name, {}, monkeypatch)
    L, U = ic.pool(name)
    lb, ub = ic.row_bounds(name, "mid")
    want = ic.expected(name, "mid", k, 0.0)
    kept = int(want[0][k])
    buffers = sentinel_buffers(k, kept)
    first = d.bound_tightened_panel(L[:k], U[:k], lb, ub, 0.0, capacity=kept, buffers=buffers)
    ic.same_lists(first, want, f"{name} lists first")
    for which in ic.ROW_BOUND_SETS:
        for tol in ic.TOLERANCES:
            summaries = np.zeros(k + 1, dbi.SUMMARY)
            summaries["worst_row"][k] = -77
            got = d.bound_tightened_panel(L[:k], U[:k], *ic.row_bounds(name, which), tol,
                                          lists=False, buffers={"summaries": summaries})
            assert got[:4] == (None, None, None, None)
            bc.same_summaries(got[4], ic.expected(name, which, k, tol)[4],
                              f"{name} {which} {tol} summaries")
            assert summaries["worst_row"][k] == -77
            assert d.last_bound_implied() == list_record(name, k, own_shape(name), 0, lists=False)
    ic.same_lists(first, want, f"{name} lists after the summaries-only calls")
    check_sentinels(buffers, k, kept, name)
    base_lb, base_ub, sets = ic.pool_as_overrides(name, k)
    got = d.bound_tightened_panel_from(base_lb, base_ub, *bc.flatten(sets), lb, ub, 0.0,
                                       lists=False)
    NL, NU = ic.first(ic.reference(name, "mid"), k)
    bc.same_summaries(got[4], ic.keep_reference(L[:k], U[:k], NL, NU, 0.0,
                                                base=(base_lb, base_ub))[4],
                      "override summaries only")
    assert d.last_bound_implied() == list_record(name, k, own_shape(name), 0, lists=False,
                                                 sets=sets)


def test_capacity_one_short(monkeypatch):
    name, k = "rows70", 17
    d = handle(name, {}, monkeypatch)
    L, U = ic.pool(name)
    lb, ub = ic.row_bounds(name, "mid")
    want = ic.expected(name, "mid", k, 0.0)
    kept = int(want[0][k])
    assert kept > 1
    buffers = sentinel_buffers(k, kept)
    before = {key: value.copy() for key, value in buffers.items()}
    with pytest.raises(dbi.CapacityError) as e:
        d.bound_tightened_panel(L[:k], U[:k], lb, ub, 0.0, capacity=kept - 1, buffers=buffers)
    assert str(kept) in str(e.value)
    for key in buffers:
        assert buffers[key].tobytes() == before[key].tobytes(), key
    assert devop.device_error is None
    got = d.bound_tightened_panel(L[:k], U[:k], lb, ub, 0.0, capacity=kept, buffers=buffers)
    ic.same_lists(got, want, "exact capacity")


@pytest.mark.parametrize("env", ({}, {"MILP_SHARDS": "2"}), ids=("unsplit", "two_shards"))
def test_one_handle_alternates_every_role(env, monkeypatch):
    """One fresh handle alternates the implied bounds with ranges, screening,
    violations and column dots: `implied` and the third block of `flat` grow
    under the new role, `rows` keeps three blocks between the two phases, and
    counts, offsets, the kept indices, the row bounds and the bases are then
    used by the older calls. Each call's record is its own."""
    name = "rows70"
    mat = bc.matrix(name)
    d = handle(name, env, monkeypatch, cached=False)
    try:
        L, U = ic.pool(name)
        pts = rc.points(name)
        y = sc.vector_pool(name)
        dots = np.stack([column_scalar_products(mat, np.arange(mat.N), v) for v in y[:5]])

        def implied(k, which):
            got = d.bound_implied_panel(L[:k], U[:k], *ic.row_bounds(name, which))
            ic.same_bounds(got, ic.first(ic.reference(name, which), k), f"implied k={k}")
            assert d.last_bound_implied() == dense_record(name, k, dbi.SHORT_COLUMNS)

        def tightened(k, tol):
            before = d.last_bound_ranges()
            want = ic.expected(name, "mid", k, tol)
            got = d.bound_tightened_panel(L[:k], U[:k], *ic.row_bounds(name, "mid"), tol)
            ic.same_lists(got, want, f"tightened k={k}")
            assert d.last_bound_implied() == list_record(name, k, dbi.SHORT_COLUMNS,
                                                         int(want[0][k]))
            assert d.last_bound_ranges() == before

        def tightened_from(k):
            base_lb, base_ub, sets = ic.pool_as_overrides(name, k)
            NL, NU = ic.first(ic.reference(name, "mid"), k)
            want = ic.keep_reference(L[:k], U[:k], NL, NU, 0.0, base=(base_lb, base_ub))
            got = d.bound_tightened_panel_from(base_lb, base_ub, *bc.flatten(sets),
                                               *ic.row_bounds(name, "mid"), 0.0)
            ic.same_lists(got, want, f"tightened from k={k}")

        def ranges(k):
            before = d.last_bound_implied()
            bc.same_ranges(d.bound_ranges_panel(L[:k], U[:k]), bc.first(bc.reference(name), k),
                           f"ranges k={k}")
            assert d.last_bound_implied() == before

        def screening(k, which):
            want = bc.expected(name, which, k)
            got = d.bound_infeasible_panel(L[:k], U[:k], *bc.row_bounds(name, which))
            bc.same_result(got, want, f"screening k={k} {which}")

        def violations(k, which):
            before = d.last_bound_implied()
            got = d.row_violations_panel(pts[:k], *vc.bounds(name, which))
            vc.same_result(got, vc.expected(name, which, k), f"violations k={k} {which}")
            assert d.last_bound_implied() == before

        def column_dots():
            got = d.column_dots_panel(y[:5])
            assert np.array_equal(bits(got), bits(dots))

        for _ in range(2):
            implied(1, "mid")
            ranges(2)
            tightened(33, 0.0)
            violations(2, "split")
            implied(33, "crossed")
            column_dots()
            tightened_from(17)
            screening(5, "split")
            tightened(5, 0.375)
            violations(33, "crossed")
            ranges(33)
            implied(17, "mid")
        row_violations = d.last_row_violations()
        bound_ranges = d.last_bound_ranges()
        tightened(17, 0.0)
        assert d.last_row_violations() == row_violations and d.last_bound_ranges() == bound_ranges
    finally:
        d.close()
