"""DeviceLp::BoundRangesPanel(From) and BoundInfeasiblePanel(From) through the
probe (tests/devop_bound_ranges.py), against the numpy reference of
tests/bound_range_cases.py (ranges, filter_reference). Every comparison is on
all 64 bits, NaNs included, and every case asserts its record
(last_bound_ranges).

rows70, steps and groups run with k bound sets for every panel width, for
padding and for several panels, in the dense and in the override form; tall
(258 tiles) the screening with k = 1, 4 and 5; each screening over every
row-bound set. tests/test_bound_ranges_ref_cpu.py shows that these inputs hold
the cases they are there for. Then: summaries only, a capacity one entry
short, and one handle that alternates ranges, row sums, violations and sparse
rows, unsplit and with two column shards, so that every shared buffer grows
under the new role and is then used under an older one.
"""
import functools

import numpy as np
import pytest

import bound_range_cases as bc
import devop
import devop_bound_ranges as dbr
import panel_sparse_cases as psc
import row_panel_cases as rc
import row_violation_cases as vc
import solveops_cases as sc
from device_ref import bits, column_scalar_products

pytestmark = pytest.mark.gpu

SWITCHES = ("MILP_DENSE_BLOCK", "MILP_SHARDS", "MILP_SHARD_DEVICES", "MILP_SMALL_FUSED",
            "MILP_SMALL_BATCH", "MILP_ROWWISE_LIST", "MILP_MEDIUM", "MILP_FULL_ROWS",
            "MILP_DENSE_UNROLL", "MILP_EARLY_FLIPS")
ROW_SENTINEL = np.int32(-77)
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
    mat = bc.matrix(name)
    return dbr.BoundRangesDevOp(mat.m, mat.n, mat.col_starts, mat.row_idx, mat.vals)


def handle(name, env, monkeypatch, cached=True):
    """The MILP_* switches are read when a handle is created."""
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    make = _cached_handle if cached else _cached_handle.__wrapped__
    return make(name, tuple(sorted(env.items())))


def shape_record(k):
    return {"panels": len(rc.panels(k)), "width": rc.width(rc.panels(k)[-1][1])}


def dense_record(name, k, counts=True, up_bytes=0):
    m = bc.matrix(name).m
    return dict(shape_record(k), lists=False, kept=0, bytes_down=(24 if counts else 16) * k * m,
                overrides_up_bytes=up_bytes)


def screen_record(k, kept, lists=True, up_bytes=0):
    return dict(shape_record(k), lists=lists, kept=kept,
                bytes_down=(12 * kept + 32 * k) if lists else 24 * k, overrides_up_bytes=up_bytes)


def sentinel_buffers(k, kept):
    summaries = np.zeros(k + 1, dbr.SUMMARY)
    summaries["count"][k], summaries["worst"][k], summaries["worst_row"][k] = -5, -7.25, -77
    return {"row_starts": np.full(k + 2, -5, np.int64),
            "rows": np.full(kept + 1, ROW_SENTINEL), "activities": np.full(kept + 1, VALUE_SENTINEL),
            "summaries": summaries}


def check_sentinels(buffers, k, kept, what):
    assert buffers["row_starts"][k + 1] == -5, what
    assert buffers["rows"][kept] == ROW_SENTINEL, what
    assert bits(buffers["activities"][kept]) == bits(VALUE_SENTINEL), what
    s = buffers["summaries"][k]
    assert (s["count"], s["worst_row"]) == (-5, -77) and s["worst"] == -7.25, what


CASE_KS = [(name, k) for name in bc.CASES for k in bc.KS]
SCREEN_KS = [(name, k) for name in bc.SCREEN_CASES for k in bc.ks(name)]


@pytest.mark.parametrize("name,k", CASE_KS)
def test_dense_ranges(name, k, monkeypatch):
    """The dense form and the override form of the same k bound sets against
    the reference and against each other; one sentinel behind each output."""
    d = handle(name, {}, monkeypatch)
    m = d.m
    L, U = bc.pool(name)
    want = bc.first(bc.reference(name), k)
    buffers = {"lo": np.full(k * m + 1, VALUE_SENTINEL), "hi": np.full(k * m + 1, VALUE_SENTINEL),
               "counts": np.full(2 * k * m + 1, ROW_SENTINEL)}
    got = d.bound_ranges_panel(L[:k], U[:k], buffers=buffers)
    p = d.last_bound_ranges()
    print(name, k, p)
    bc.same_ranges(got, want, f"{name} k={k} dense")
    assert p == dense_record(name, k), p
    assert bits(buffers["lo"][k * m]) == bits(buffers["hi"][k * m]) == bits(VALUE_SENTINEL)
    assert buffers["counts"][2 * k * m] == ROW_SENTINEL
    without = d.bound_ranges_panel(L[:k], U[:k], counts=False)
    bc.same_ranges(without[:2], want[:2], f"{name} k={k} without counts")
    assert without[2] is None and d.last_bound_ranges() == dense_record(name, k, counts=False)
    base_lb, base_ub, sets = bc.pool_as_overrides(name, k)
    over = d.bound_ranges_panel_from(base_lb, base_ub, *bc.flatten(sets))
    bc.same_ranges(over, want, f"{name} k={k} overrides of child 0")
    bc.same_ranges(over, got, f"{name} k={k} override form against the dense form")
    assert d.last_bound_ranges() == dense_record(name, k,
                                                 up_bytes=bc.override_bytes(name, sets))


@pytest.mark.parametrize("which", bc.OVERRIDE_SETS)
@pytest.mark.parametrize("name", bc.CASES)
def test_override_sets(name, which, monkeypatch):
    """Override lists of their own (a branching node, special values, a panel
    boundary): ranges and screening against the reference on the materialised
    sets and against the dense form on them."""
    d = handle(name, {}, monkeypatch)
    base_lb, base_ub, sets = bc.override_set(name, which)
    k = len(sets)
    flat = bc.flatten(sets)
    up = bc.override_bytes(name, sets)
    want = bc.override_reference(name, which)
    got = d.bound_ranges_panel_from(base_lb, base_ub, *flat)
    bc.same_ranges(got, want, f"{name} {which}")
    assert d.last_bound_ranges() == dense_record(name, k, up_bytes=up)
    L, U = bc.materialise(base_lb, base_ub, sets)
    bc.same_ranges(d.bound_ranges_panel(L, U), got, f"{name} {which} against the dense form")
    for bound_set in ("split", "edges_tol", "crossed"):
        what = f"{name} {which} {bound_set}"
        lb, ub, tol = bc.row_bounds(name, bound_set)
        ref = bc.filter_reference(want, lb, ub, tol)
        kept = int(ref[0][k])
        buffers = sentinel_buffers(k, kept)
        res = d.bound_infeasible_panel_from(base_lb, base_ub, *flat, lb, ub, tol, capacity=kept,
                                            buffers=buffers)
        p = d.last_bound_ranges()
        bc.same_result(res, ref, what)
        check_sentinels(buffers, k, kept, what)
        assert p == screen_record(k, kept, up_bytes=up), (what, p)
        dense = d.bound_infeasible_panel(L, U, lb, ub, tol)
        bc.same_result(dense, res, what + " against the dense form")
        assert d.last_bound_ranges() == screen_record(k, kept)


def summaries_from_lists(got, what):
    """count = list length; worst and worst_row recomputed from the listed
    amounts alone."""
    starts, rows, amounts, summaries = got
    for j in range(len(summaries)):
        mine = rows[starts[j]:starts[j + 1]]
        g = amounts[starts[j]:starts[j + 1]]
        assert summaries["count"][j] == len(mine), (what, j)
        assert np.all(np.diff(mine) > 0), (what, j)
        if len(mine) == 0:
            assert summaries["worst_row"][j] == -1 and bits(summaries["worst"][j]) == 0, (what, j)
            continue
        assert bits(summaries["worst"][j]) == bits(g.max()), (what, j)
        assert summaries["worst_row"][j] == mine[np.nonzero(g == g.max())[0][0]], (what, j)


@pytest.mark.parametrize("name,k", SCREEN_KS)
def test_screening(name, k, monkeypatch):
    """k bound sets under every row-bound set: lists, summaries, sentinels,
    record; the override form of the same sets where the pool is small."""
    d = handle(name, {}, monkeypatch)
    L, U = bc.pool(name)
    for which in bc.ROW_BOUND_SETS:
        what = f"{name} k={k} {which}"
        lb, ub, tol = bc.row_bounds(name, which)
        want = bc.expected(name, which, k)
        kept = int(want[0][k])
        buffers = sentinel_buffers(k, kept)
        got = d.bound_infeasible_panel(L[:k], U[:k], lb, ub, tol, capacity=kept, buffers=buffers)
        p = d.last_bound_ranges()
        print(what, p)
        bc.same_result(got, want, what)
        check_sentinels(buffers, k, kept, what)
        assert p == screen_record(k, kept), (what, p)
        summaries_from_lists(got, what)
        assert not np.isnan(got[2]).any() and np.all(got[2] > tol), what
    if name != "tall":
        base_lb, base_ub, sets = bc.pool_as_overrides(name, k)
        lb, ub, tol = bc.row_bounds(name, "split")
        got = d.bound_infeasible_panel_from(base_lb, base_ub, *bc.flatten(sets), lb, ub, tol)
        bc.same_result(got, bc.expected(name, "split", k), f"{name} k={k} override form")
        kept = int(bc.expected(name, "split", k)[0][k])
        assert d.last_bound_ranges() == screen_record(k, kept,
                                                      up_bytes=bc.override_bytes(name, sets))


@pytest.mark.parametrize("name,k", [("rows70", 17), ("groups", 5), ("tall", 5)])
def test_summaries_only(name, k, monkeypatch):
    """The same summaries, 24 bytes per child down, and what an earlier call
    returned is untouched."""
    d = handle(name, {}, monkeypatch)
    L, U = bc.pool(name)
    lb, ub, tol = bc.row_bounds(name, "split")
    want = bc.expected(name, "split", k)
    kept = int(want[0][k])
    buffers = sentinel_buffers(k, kept)
    first = d.bound_infeasible_panel(L[:k], U[:k], lb, ub, tol, capacity=kept, buffers=buffers)
    bc.same_result(first, want, f"{name} lists first")
    for which in ("split", "crossed", "free"):
        b = bc.row_bounds(name, which)
        summaries = np.zeros(k + 1, dbr.SUMMARY)
        summaries["worst_row"][k] = -77
        got = d.bound_infeasible_panel(L[:k], U[:k], *b, lists=False,
                                       buffers={"summaries": summaries})
        assert got[:3] == (None, None, None)
        bc.same_summaries(got[3], bc.expected(name, which, k)[3], f"{name} {which} summaries")
        assert summaries["worst_row"][k] == -77
        assert d.last_bound_ranges() == screen_record(k, 0, lists=False)
    bc.same_result(first, want, f"{name} lists after the summaries-only calls")
    check_sentinels(buffers, k, kept, name)
    if name != "tall":
        base_lb, base_ub, sets = bc.pool_as_overrides(name, k)
        got = d.bound_infeasible_panel_from(base_lb, base_ub, *bc.flatten(sets), lb, ub, tol,
                                            lists=False)
        bc.same_summaries(got[3], want[3], "override summaries only")
        assert d.last_bound_ranges() == screen_record(
            k, 0, lists=False, up_bytes=bc.override_bytes(name, sets))


def test_capacity_one_short(monkeypatch):
    name, k = "rows70", 17
    d = handle(name, {}, monkeypatch)
    L, U = bc.pool(name)
    lb, ub, tol = bc.row_bounds(name, "split")
    kept = int(bc.expected(name, "split", k)[0][k])
    assert kept > 1
    buffers = sentinel_buffers(k, kept)
    buffers["rows"][:] = ROW_SENTINEL
    before = {key: value.copy() for key, value in buffers.items()}
    with pytest.raises(dbr.CapacityError) as e:
        d.bound_infeasible_panel(L[:k], U[:k], lb, ub, tol, capacity=kept - 1, buffers=buffers)
    assert str(kept) in str(e.value)
    for key in buffers:
        assert buffers[key].tobytes() == before[key].tobytes(), key
    assert devop.device_error is None
    got = d.bound_infeasible_panel(L[:k], U[:k], lb, ub, tol, capacity=kept, buffers=buffers)
    bc.same_result(got, bc.expected(name, "split", k), "exact capacity")


@pytest.mark.parametrize("env", ({}, {"MILP_SHARDS": "2"}), ids=("unsplit", "two_shards"))
def test_one_handle_alternates_every_role(env, monkeypatch):
    """One fresh handle alternates ranges, row sums, violations and sparse
    rows: `rows` (three blocks), `flat` (two arrays up, three blocks down) and
    the upper-bound buffer grow under the ranges' role, and counts, offsets
    and the kept indices are then used by the older calls. Each call's record
    is its own: the others stay as their last call left them."""
    name = "rows70"
    mat = bc.matrix(name)
    d = handle(name, env, monkeypatch, cached=False)
    try:
        L, U = bc.pool(name)
        pts, sums = rc.points(name), rc.reference(name)
        y = sc.vector_pool(name)
        dots = np.stack([column_scalar_products(mat, np.arange(mat.N), v) for v in y[:5]])
        structural = np.arange(mat.N) < mat.n
        sparse_want = psc.filtered(dots, structural, 0.0)

        def ranges(k):
            bc.same_ranges(d.bound_ranges_panel(L[:k], U[:k]), bc.first(bc.reference(name), k),
                           f"ranges k={k}")
            assert d.last_bound_ranges() == dense_record(name, k)

        def ranges_from(k):
            base_lb, base_ub, sets = bc.pool_as_overrides(name, k)
            got = d.bound_ranges_panel_from(base_lb, base_ub, *bc.flatten(sets))
            bc.same_ranges(got, bc.first(bc.reference(name), k), f"ranges from k={k}")

        def screening(k, which):
            want = bc.expected(name, which, k)
            got = d.bound_infeasible_panel(L[:k], U[:k], *bc.row_bounds(name, which))
            bc.same_result(got, want, f"screening k={k} {which}")
            assert d.last_bound_ranges() == screen_record(k, int(want[0][k]))

        def violations(k, which):
            before = d.last_bound_ranges()
            got = d.row_violations_panel(pts[:k], *vc.bounds(name, which))
            vc.same_result(got, vc.expected(name, which, k), f"violations k={k} {which}")
            assert d.last_bound_ranges() == before

        def sparse_rows():
            got = d.column_dots_panel_sparse(y[:5], 0.0, structural)
            for g, w in zip(got[:2], sparse_want[:2]):
                assert np.array_equal(g, w)
            assert np.array_equal(bits(got[2]), bits(sparse_want[2]))

        def row_sums(k):
            before = d.last_bound_ranges()
            assert np.array_equal(bits(d.row_sums_panel(pts[:k])), bits(sums[:k]))
            assert d.last_bound_ranges() == before

        for _ in range(2):
            ranges(1)
            row_sums(2)
            screening(33, "crossed")
            violations(2, "split")
            ranges(33)
            sparse_rows()
            ranges_from(17)
            row_sums(17)
            screening(5, "split")
            violations(33, "crossed")
        row_panel = d.last_row_panel()
        row_violations = d.last_row_violations()
        screening(17, "edges_tol")
        assert d.last_row_panel() == row_panel and d.last_row_violations() == row_violations
    finally:
        d.close()
