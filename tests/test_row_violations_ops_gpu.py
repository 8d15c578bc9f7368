"""DeviceLp::RowViolationsPanel and RowViolationsPanelFrom through the probe
(tests/devop_row_violations.py), against the dense reference filtered in numpy
with the header's rule (row_violation_cases.filter_reference). Every
comparison is on all 64 bits, NaNs included.

rows70 and steps (less than one tile of rows) run with k points for every
panel width, for padding and for several panels; tall (258 tiles: more than
one step of the offsets scan, a partial last tile) with k = 1, 4 and 5; each
over every bound set. tests/test_row_violations_ref_cpu.py shows that these
inputs hold the cases they are there for. last_row_violations must report the
panels, the width, the kept entries and the bytes that came down. Then: the
override form, summaries only, a capacity one entry short, the summaries
against the lists, two column shards, the shared workspace buffers under each
of their roles, and that a call leaves the solve state and the row-sum record
alone.
"""
import functools

import numpy as np
import pytest

import devop
import devop_panel_sparse
import devop_row_violations as drv
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
DROP = 1e-11


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
    mat = vc.matrix(name)
    return drv.RowViolationsDevOp(mat.m, mat.n, mat.col_starts, mat.row_idx, mat.vals)


def handle(name, env, monkeypatch, cached=True):
    """The MILP_* switches are read when a handle is created."""
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    make = _cached_handle if cached else _cached_handle.__wrapped__
    return make(name, tuple(sorted(env.items())))


def sentinel_buffers(k, kept):
    """Room for exactly `kept` entries and k summaries, one sentinel behind
    each."""
    summaries = np.zeros(k + 1, drv.SUMMARY)
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


def expected_record(k, kept, lists=True, up_bytes=0):
    last = rc.panels(k)[-1][1]
    return {"panels": len(rc.panels(k)), "width": rc.width(last), "lists": lists, "kept": kept,
            "bytes_down": (12 * kept + (8 + 24) * k) if lists else 24 * k,
            "overrides_up_bytes": up_bytes}


def test_geometry():
    """tall is sized by the two constants of the sparse-row kernels, which
    the violation kernels share."""
    g = devop_panel_sparse.geometry()
    assert (g["tile_columns"], g["offsets_step_tiles"]) == (vc.TILE_ROWS, vc.OFFSETS_STEP_TILES)
    assert vc.satisfies_geometry(vc.TALL_M, g["tile_columns"], g["offsets_step_tiles"])


CASE_KS = [(name, k) for name in vc.CASES for k in vc.ks(name)]


@pytest.mark.parametrize("name,k", CASE_KS)
def test_dense_points(name, k, monkeypatch):
    """k points under every bound set: lists, summaries, sentinels, record."""
    d = handle(name, {}, monkeypatch)
    x = vc.points(name)[:k]
    for which in vc.BOUND_SETS:
        what = f"{name} k={k} {which}"
        lb, ub, tol = vc.bounds(name, which)
        want = vc.expected(name, which, k)
        kept = int(want[0][k])
        buffers = sentinel_buffers(k, kept)
        got = d.row_violations_panel(x, lb, ub, tol, capacity=kept, buffers=buffers)
        p = d.last_row_violations()
        print(what, p)
        vc.same_result(got, want, what)
        check_sentinels(buffers, k, kept, what)
        assert p == expected_record(k, kept), (what, p)
        summaries_from_lists(got, lb, ub, what)


def summaries_from_lists(got, lb, ub, what):
    """count = list length; worst and worst_row recomputed from the listed
    activities alone."""
    starts, rows, vals, summaries = got
    for j in range(len(summaries)):
        mine = rows[starts[j]:starts[j + 1]]
        assert summaries["count"][j] == len(mine), (what, j)
        if len(mine) == 0:
            assert summaries["worst_row"][j] == -1 and bits(summaries["worst"][j]) == 0, (what, j)
            continue
        _, _, amount = vc.amounts(vals[starts[j]:starts[j + 1]], lb[mine], ub[mine])
        assert bits(summaries["worst"][j]) == bits(amount.max()), (what, j)
        assert summaries["worst_row"][j] == mine[np.nonzero(amount == amount.max())[0][0]], (what, j)


@pytest.mark.parametrize("which", rc.OVERRIDE_SETS)
@pytest.mark.parametrize("name", ("rows70", "steps"))
def test_override_points(name, which, monkeypatch):
    """The override form equals the numpy filter of the materialised points'
    reference and the dense form on them; the bytes that went up."""
    d = handle(name, {}, monkeypatch)
    base, sets = rc.override_set(name, which)
    k = len(sets)
    starts, cols, vals = rc.flatten(sets)
    for bound_set in ("split", "edges_tol", "free"):
        what = f"{name} {which} {bound_set}"
        lb, ub, tol = vc.bounds(name, bound_set)
        want = vc.filter_reference(rc.override_reference(name, which), lb, ub, tol)
        kept = int(want[0][k])
        buffers = sentinel_buffers(k, kept)
        got = d.row_violations_panel_from(base, starts, cols, vals, lb, ub, tol, capacity=kept,
                                          buffers=buffers)
        p = d.last_row_violations()
        vc.same_result(got, want, what)
        check_sentinels(buffers, k, kept, what)
        assert p == expected_record(k, kept, up_bytes=rc.override_bytes(name, which)), (what, p)
        dense = d.row_violations_panel(rc.materialise(base, sets), lb, ub, tol)
        vc.same_result(dense, got, what + " against the dense form")
        assert d.last_row_violations() == expected_record(k, kept)


@pytest.mark.parametrize("name,k", [("rows70", 17), ("steps", 5), ("tall", 5)])
def test_summaries_only(name, k, monkeypatch):
    """The same summaries, 24 bytes per point down, and what an earlier call
    returned is untouched."""
    d = handle(name, {}, monkeypatch)
    x = vc.points(name)[:k]
    lb, ub, tol = vc.bounds(name, "split")
    want = vc.expected(name, "split", k)
    kept = int(want[0][k])
    buffers = sentinel_buffers(k, kept)
    first = d.row_violations_panel(x, lb, ub, tol, capacity=kept, buffers=buffers)
    vc.same_result(first, want, f"{name} lists first")
    for which in ("split", "one_sided", "free"):
        b = vc.bounds(name, which)
        summaries = np.zeros(k + 1, drv.SUMMARY)
        summaries["worst_row"][k] = -77
        got = d.row_violations_panel(x, *b, lists=False, buffers={"summaries": summaries})
        assert got[:3] == (None, None, None)
        vc.same_summaries(got[3], vc.expected(name, which, k)[3], f"{name} {which} summaries")
        assert summaries["worst_row"][k] == -77
        assert d.last_row_violations() == expected_record(k, 0, lists=False)
    vc.same_result(first, want, f"{name} lists after the summaries-only calls")
    check_sentinels(buffers, k, kept, name)
    if name == "rows70":
        base, sets = rc.override_set(name, "k17")
        ref = vc.filter_reference(rc.override_reference(name, "k17"), lb, ub, tol)
        got = d.row_violations_panel_from(base, *rc.flatten(sets), lb, ub, tol, lists=False)
        vc.same_summaries(got[3], ref[3], "override summaries only")
        assert d.last_row_violations() == expected_record(
            17, 0, lists=False, up_bytes=rc.override_bytes(name, "k17"))


def test_capacity_one_short(monkeypatch):
    name, k = "rows70", 17
    d = handle(name, {}, monkeypatch)
    lb, ub, tol = vc.bounds(name, "split")
    kept = int(vc.expected(name, "split", k)[0][k])
    assert kept > 1
    buffers = sentinel_buffers(k, kept)
    buffers["rows"][:] = ROW_SENTINEL
    before = {key: value.copy() for key, value in buffers.items()}
    with pytest.raises(drv.CapacityError) as e:
        d.row_violations_panel(vc.points(name)[:k], lb, ub, tol, capacity=kept - 1,
                               buffers=buffers)
    assert str(kept) in str(e.value)
    for key in buffers:
        assert buffers[key].tobytes() == before[key].tobytes(), key
    assert devop.device_error is None
    got = d.row_violations_panel(vc.points(name)[:k], lb, ub, tol, capacity=kept, buffers=buffers)
    vc.same_result(got, vc.expected(name, "split", k), "exact capacity")


def test_two_column_shards(monkeypatch):
    """The operation stays on the unsplit handle, as RowSumsPanel does."""
    name = "rows70"
    d = handle(name, {"MILP_SHARDS": "2"}, monkeypatch)
    for k in (5, 17):
        for which in ("split", "edges0"):
            want = vc.expected(name, which, k)
            got = d.row_violations_panel(vc.points(name)[:k], *vc.bounds(name, which))
            vc.same_result(got, want, f"two shards k={k} {which}")
            assert d.last_row_violations() == expected_record(k, int(want[0][k]))
    base, sets = rc.override_set(name, "k17")
    lb, ub, tol = vc.bounds(name, "split")
    want = vc.filter_reference(rc.override_reference(name, "k17"), lb, ub, tol)
    vc.same_result(d.row_violations_panel_from(base, *rc.flatten(sets), lb, ub, tol), want,
                   "two shards overrides")


def test_shared_buffers_grow_under_each_role(monkeypatch):
    """One fresh handle alternates a wide violations call, a narrow one, the
    sparse rows and the dense row sums: counts, offsets, the kept indices and
    `flat` grow under one call's role and are then used by another's."""
    name = "rows70"
    mat = vc.matrix(name)
    d = handle(name, {}, monkeypatch, cached=False)
    try:
        pts, ref = vc.points(name), vc.reference(name)
        y = sc.vector_pool(name)
        dots = np.stack([column_scalar_products(mat, np.arange(mat.N), v) for v in y[:5]])
        structural = np.arange(mat.N) < mat.n
        sparse_want = psc.filtered(dots, structural, 0.0)

        def violations(k, which):
            got = d.row_violations_panel(pts[:k], *vc.bounds(name, which))
            vc.same_result(got, vc.expected(name, which, k), f"violations k={k} {which}")

        def sparse_rows():
            got = d.column_dots_panel_sparse(y[:5], 0.0, structural)
            for g, w in zip(got[:2], sparse_want[:2]):
                assert np.array_equal(g, w)
            assert np.array_equal(bits(got[2]), bits(sparse_want[2]))

        def row_sums(k):
            assert np.array_equal(bits(d.row_sums_panel(pts[:k])), bits(ref[:k]))

        for _ in range(2):
            violations(33, "crossed")
            violations(2, "split")
            sparse_rows()
            row_sums(17)
        violations(33, "split")
    finally:
        d.close()


def test_violations_leave_solve_state_alone(monkeypatch):
    name = "rows70"
    mat, pts = vc.matrix(name), vc.points(name)
    d = handle(name, {}, monkeypatch, cached=False)
    try:
        d.set_mask(np.ones(mat.N, bool))
        rows = np.array([3, 17, 40, 41, 69], np.int32)
        rho = pts[0][:mat.m]
        d.update_row_row_wise(rows, rho, 2, DROP)
        pos, val = d.fetch_update_row()
        coeff = d.download_coefficients()
        paths = d.paths()
        assert len(pos) > 0
        d.row_sums_panel(pts[:5])
        row_panel = d.last_row_panel()
        lb, ub, tol = vc.bounds(name, "split")
        d.row_violations_panel(pts[:17], lb, ub, tol)
        base, sets = rc.override_set(name, "k17")
        d.row_violations_panel_from(base, *rc.flatten(sets), lb, ub, tol)
        d.row_violations_panel(pts[:4], lb, ub, tol, lists=False)
        pos2, val2 = d.fetch_update_row()
        assert np.array_equal(pos2, pos)
        assert np.array_equal(bits(val2), bits(val))
        assert np.array_equal(bits(d.download_coefficients()), bits(coeff))
        assert d.paths() == paths
        assert d.last_row_panel() == row_panel
        rcs = pts[4]
        d.dual_begin(rcs, np.zeros(mat.N, np.uint8), np.ones(mat.N))
        got = d.row_violations_panel(pts[:4], lb, ub, tol)
        vc.same_result(got, vc.expected(name, "split", 4), "violations in dual mode")
        assert np.array_equal(bits(d.dual_download_reduced_costs()), bits(rcs))
    finally:
        d.close()
