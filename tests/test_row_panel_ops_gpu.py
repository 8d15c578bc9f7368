"""DeviceLp::RowSumsPanel and RowSumsPanelFrom through the probe
(tests/devop_row_panel.py), bit for bit against RefState.row_sums of
tests/device_ref.py and against the one-vector kernel behind the probe's
row_sums entry. Every comparison is on all 64 bits, NaNs included.

Every matrix of tests/row_panel_cases.py runs with k points for every panel
width, for padding and for several panels; last_row_panel must report the
panels, the width and the kernel path, and for the override form the bytes
that went up. tests/test_row_panel_ref_cpu.py shows that these inputs tell
summation orders apart. Then: nothing is written behind the k-th row, two
column shards, a large call followed by a small one on the same handle, and
that a panel leaves the update row and the dual-mode reduced costs alone.
"""
import functools

import numpy as np
import pytest

import devop
import devop_row_panel
import row_panel_cases as rc
from device_ref import bits

pytestmark = pytest.mark.gpu

SWITCHES = ("MILP_DENSE_BLOCK", "MILP_SHARDS", "MILP_SHARD_DEVICES", "MILP_SMALL_FUSED",
            "MILP_SMALL_BATCH", "MILP_ROWWISE_LIST", "MILP_MEDIUM", "MILP_FULL_ROWS",
            "MILP_DENSE_UNROLL", "MILP_EARLY_FLIPS")
SENTINEL = np.float64(-7.25)
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
    mat = rc.matrix(name)
    return devop_row_panel.RowPanelDevOp(mat.m, mat.n, mat.col_starts, mat.row_idx, mat.vals)


def handle(name, env, monkeypatch, cached=True):
    """The MILP_* switches are read when a handle is created."""
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    make = _cached_handle if cached else _cached_handle.__wrapped__
    return make(name, tuple(sorted(env.items())))


def same_bits(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {want.size} differ, first at {tuple(bad[0])}: "
                           f"device {got[tuple(bad[0])].hex()} reference "
                           f"{want[tuple(bad[0])].hex()}")


def expected_record(k, up_bytes=0):
    last = rc.panels(k)[-1][1]
    return {"panels": len(rc.panels(k)), "width": rc.width(last), "kernel": "direct",
            "overrides_up_bytes": up_bytes}


def with_sentinel(mat, k):
    """A flat k x m output with one more row behind it."""
    return np.full((k + 1) * mat.m, SENTINEL)


def check_sentinel(out, mat, k, what):
    assert np.all(bits(out[k * mat.m:]) == bits(SENTINEL)), what


def test_geometry():
    g = devop_row_panel.geometry()
    assert g["rows_per_workgroup"] == {1: 256, 4: 64, 16: 16}
    # The kernel reads its rows directly: the steps matrix of row_panel_cases
    # stands in for the matrix around a staging chunk.
    assert g["chunk"] == 0 and "steps" in rc.CASES


@pytest.mark.parametrize("k", rc.KS)
@pytest.mark.parametrize("name", rc.CASES)
def test_dense_points(name, k, monkeypatch):
    """k points against the reference, and point by point against the
    one-vector kernel (sign 1, no skip)."""
    mat = rc.matrix(name)
    d = handle(name, rc.environment(name), monkeypatch)
    x = rc.points(name)[:k]
    out = with_sentinel(mat, k)
    got = d.row_sums_panel(x, out=out)
    p = d.last_row_panel()
    print(name, "k", k, p)
    same_bits(got, rc.reference(name)[:k], f"{name} k={k}")
    check_sentinel(out, mat, k, f"{name} k={k}")
    assert p == expected_record(k), (name, k, p)
    one = np.stack([d.row_sums(x[j], False, 1.0) for j in range(k)])
    same_bits(got, one, f"{name} k={k} against row_sums")
    if k >= 3:
        assert np.all(bits(got[rc.ALL_POS_ZERO]) == 0) and np.all(bits(got[rc.ALL_NEG_ZERO]) == 0)
    if k >= 8:
        assert np.isnan(got[rc.WITH_NAN]).sum() >= 2 and np.isinf(got[rc.WITH_INF]).sum() >= 2


@pytest.mark.parametrize("which", rc.OVERRIDE_SETS)
@pytest.mark.parametrize("name", rc.CASES)
def test_override_points(name, which, monkeypatch):
    """The override form against the reference on the materialised points and
    against the dense form on them; the bytes that went up."""
    mat = rc.matrix(name)
    d = handle(name, rc.environment(name), monkeypatch)
    base, sets = rc.override_set(name, which)
    k = len(sets)
    starts, cols, vals = rc.flatten(sets)
    out = with_sentinel(mat, k)
    got = d.row_sums_panel_from(base, starts, cols, vals, out=out).copy()
    p = d.last_row_panel()
    print(name, which, p)
    same_bits(got, rc.override_reference(name, which), f"{name} {which}")
    check_sentinel(out, mat, k, f"{name} {which}")
    assert p == expected_record(k, rc.override_bytes(name, which)), (name, which, p)
    dense = d.row_sums_panel(rc.materialise(base, sets))
    same_bits(got, dense, f"{name} {which} against the dense form")
    assert d.last_row_panel() == expected_record(k)


def test_no_overrides_at_all(monkeypatch):
    """starts all zero, cols and vals NULL: k copies of the base's sums."""
    name = "rows70"
    mat = rc.matrix(name)
    d = handle(name, {}, monkeypatch)
    base, _ = rc.override_set(name, "mixed")
    got = d.row_sums_panel_from(base, np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0))
    want = rc.override_reference(name, "mixed")[0]
    same_bits(got, np.stack([want] * 3), "rows70 without overrides")
    assert d.last_row_panel() == expected_record(3, 8 * mat.N + 8 * 4)


def test_two_column_shards(monkeypatch):
    """The operation stays on the unsplit handle, as RowSums does."""
    name = "rows70"
    d = handle(name, {"MILP_SHARDS": "2"}, monkeypatch)
    for k in (5, 17):
        same_bits(d.row_sums_panel(rc.points(name)[:k]), rc.reference(name)[:k],
                  f"{name} two shards k={k}")
        assert d.last_row_panel() == expected_record(k)
    base, sets = rc.override_set(name, "k17")
    same_bits(d.row_sums_panel_from(base, *rc.flatten(sets)), rc.override_reference(name, "k17"),
              f"{name} two shards overrides")


def test_large_then_small_on_one_handle(monkeypatch):
    """The grow-only buffers hold a 16-wide panel's points when a narrower
    panel follows: its padding is written anew and the stale points are not
    read."""
    name = "rows70"
    d = handle(name, {}, monkeypatch, cached=False)
    try:
        pts, ref = rc.points(name), rc.reference(name)
        same_bits(d.row_sums_panel(pts[:33]), ref[:33], "k=33 first")
        for k in (2, 1, 5):
            same_bits(d.row_sums_panel(pts[8:8 + k]), ref[8:8 + k], f"k={k} after k=33")
            assert d.last_row_panel() == expected_record(k)
        base, sets = rc.override_set(name, "k17")
        same_bits(d.row_sums_panel_from(base, *rc.flatten(sets)),
                  rc.override_reference(name, "k17"), "k17 overrides")
        base, sets = rc.override_set(name, "four")
        same_bits(d.row_sums_panel_from(base, *rc.flatten(sets)),
                  rc.override_reference(name, "four"), "four overrides after k17")
        same_bits(d.row_sums_panel(pts[:1]), ref[:1], "k=1 last")
    finally:
        d.close()


def test_panel_leaves_solve_state_alone(monkeypatch):
    name = "rows70"
    mat, pts = rc.matrix(name), rc.points(name)
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
        base, sets = rc.override_set(name, "k17")
        d.row_sums_panel_from(base, *rc.flatten(sets))
        pos2, val2 = d.fetch_update_row()
        assert np.array_equal(pos2, pos)
        same_bits(val2, val, "list values after a panel")
        same_bits(d.download_coefficients(), coeff, "coefficients after a panel")
        assert d.paths() == paths
        rcs = pts[4]
        d.dual_begin(rcs, np.zeros(mat.N, np.uint8), np.ones(mat.N))
        same_bits(d.row_sums_panel(pts[:4]), rc.reference(name)[:4], "panel in dual mode")
        same_bits(d.dual_download_reduced_costs(), rcs, "reduced costs after a panel")
    finally:
        d.close()
