"""DeviceLp::ColumnDotsPanelSparse through the probe, exactly equal to the
dense reference (tests/device_ref.py column_scalar_products) filtered in
numpy: keep = mask & (|ref| > tolerance), columns ascending per row.

Every case of tests/panel_sparse_cases.py runs with k vectors for every panel
width, for padding and for several panels, under every mask and tolerance of
that module: row_starts and columns are compared as integers, values on
64-bit patterns; last_panel_sparse must report the kernels the case was
written for, kept = row_starts[k], and at most 12 bytes per kept entry plus
64 per vector brought down (nothing that grows with N).
tests/test_panel_sparse_ref_cpu.py shows that these masks and tolerances make
the filter keep some entries and drop others. Then: the dense block forced
and off, two column shards, buffers untouched beyond the result, a capacity
one short, the solve state left alone, dense and sparse panels in turn over
their shared buffers, and NaN / +-inf results.
"""
import functools

import numpy as np
import pytest

import devop
import devop_panel_sparse as dps
import panel_sparse_cases as sc
from device_ref import bits, column_scalar_products

pytestmark = pytest.mark.gpu

SWITCHES = ("MILP_DENSE_BLOCK", "MILP_SHARDS", "MILP_SHARD_DEVICES", "MILP_SMALL_FUSED",
            "MILP_SMALL_BATCH", "MILP_ROWWISE_LIST", "MILP_MEDIUM", "MILP_FULL_ROWS")
KS = (1, 3, 4, 5, 16, 17, 33)
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
    mat = sc.matrix(name)
    return dps.SparsePanelDevOp(mat.m, mat.n, mat.col_starts, mat.row_idx, mat.vals)


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


def same_rows(got, want, what):
    """(row_starts, cols, vals) against the filtered reference, exactly."""
    for g, w, part in zip(got[:2], want[:2], ("row_starts", "cols")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, part, g[:8], w[:8])
    same_bits(got[2], want[2], what)


def expected_panel(name, env, k):
    """The kernel choice of the dense panel (test_panel_ops_gpu.py states the
    same rule): one wave per column for `wave`, the dense-block kernel for the
    dense cases when forced, panels of 16 padded to a width of 1, 4 or 16."""
    last = k - 16 * ((k - 1) // 16)
    dense = name.startswith("dense") and env.get("MILP_DENSE_BLOCK") == "force"
    return {"sparse": "long_columns" if name == "wave" else "short_columns", "dense": dense,
            "panels": (k + 15) // 16, "width": 1 if last == 1 else (4 if last <= 4 else 16)}


def run_sparse(d, name, env, k, which, tolerance, what):
    want = sc.filtered(sc.reference(name)[:k], sc.mask(name, which), tolerance)
    keep = None if which == "all" and k % 2 else sc.mask(name, which)  # NULL = all, or the words
    got = d.column_dots_panel_sparse(sc.vectors(name)[:k], tolerance, keep)
    p = d.last_panel_sparse()
    print(what, p)
    same_rows(got, want, what)
    kept = int(want[0][k])
    assert p.pop("kept") == kept == got[0][k], what
    assert p.pop("bytes_down") <= 12 * kept + 64 * k, what
    assert p == expected_panel(name, env, k), (what, p)


def run_table(name, env, k, monkeypatch):
    d = handle(name, env, monkeypatch)
    for which in sc.MASKS:
        for tname, t in sc.tolerances(name, which).items():
            run_sparse(d, name, env, k, which, t, f"{name} k={k} mask={which} tol={tname}")
    return d


def test_the_kernels_have_the_geometry_the_long_case_assumes():
    g = dps.geometry()
    print(g)
    N = sc.matrix("long").N
    assert sc.satisfies_geometry(N, g["tile_columns"], g["offsets_step_tiles"]), (N, g)
    assert sc.matrix("edge").N < g["tile_columns"]


CASE_KS = [(name, k) for name in sorted(sc.CASES) for k in KS if k <= sc.CASES[name][3]]


@pytest.mark.parametrize("name,k", CASE_KS)
def test_sparse_panel_case(name, k, monkeypatch):
    run_table(name, sc.CASES[name][2], k, monkeypatch)


def test_dense_columns_through_the_csc_kernel(monkeypatch):
    # The same full columns without the dense block: the same rows.
    for k in (5, 17):
        run_table("dense23", {"MILP_DENSE_BLOCK": "off"}, k, monkeypatch)


@pytest.mark.parametrize("name", ["quad", "edge"])
def test_two_column_shards(name, monkeypatch):
    for k in (3, 17):
        run_table(name, {"MILP_SHARDS": "2"}, k, monkeypatch)


def test_nothing_is_written_beyond_the_result(monkeypatch):
    for name in ("quad", "dense13"):
        env = sc.CASES[name][2]
        d = handle(name, env, monkeypatch)
        N, k = sc.matrix(name).N, 3
        which, t = "random", sc.tolerances(name, "random")["median"]
        want = sc.filtered(sc.reference(name)[:k], sc.mask(name, which), t)
        kept = int(want[0][k])
        assert 0 < kept < k * N
        for fill in (np.float64(-7.25), np.float64("nan")):
            starts = np.full(k + 6, -7, np.int64)
            cols = np.full(k * N + 7, -7, np.int32)
            vals = np.full(k * N + 7, fill)
            got = d.column_dots_panel_sparse(sc.vectors(name)[:k], t, sc.mask(name, which),
                                             row_starts=starts, cols=cols, vals=vals)
            same_rows(got, want, f"{name} in place")
            assert np.all(starts[k + 1:] == -7) and np.all(cols[kept:] == -7), name
            assert np.all(bits(vals[kept:]) == bits(fill)), name


def test_capacity_one_short_is_an_error_and_writes_nothing(monkeypatch):
    name, k = "quad", 5
    d = handle(name, sc.CASES[name][2], monkeypatch)
    which, t = "structural", 0.0
    want = sc.filtered(sc.reference(name)[:k], sc.mask(name, which), t)
    kept = int(want[0][k])
    cols = np.full(kept, -7, np.int32)
    vals = np.full(kept, -7.25)
    with pytest.raises(dps.CapacityError):
        d.column_dots_panel_sparse(sc.vectors(name)[:k], t, sc.mask(name, which),
                                   capacity=kept - 1, cols=cols, vals=vals)
    assert np.all(cols == -7) and np.all(vals == -7.25)
    assert devop.device_error is None
    got = d.column_dots_panel_sparse(sc.vectors(name)[:k], t, sc.mask(name, which),
                                     capacity=kept, cols=cols, vals=vals)
    same_rows(got, want, "exact capacity")


def test_sparse_panel_leaves_solve_state_alone(monkeypatch):
    name = "quad"
    mat, y, ref = sc.matrix(name), sc.vectors(name), sc.reference(name)
    d = handle(name, {}, monkeypatch, cached=False)
    try:
        d.set_mask(np.ones(mat.N, bool))
        rows = np.array([3, 17, 40, 41, 90], np.int32)
        d.update_row_row_wise(rows, y[0], 2, DROP)
        pos, val = d.fetch_update_row()
        coeff = d.download_coefficients()
        paths = d.paths()
        assert len(pos) > 0
        t = sc.tolerances(name, "random")["median"]
        d.column_dots_panel_sparse(y[:5], t, sc.mask(name, "random"))
        d.column_dots_panel_sparse(y[:17], 0.0)
        pos2, val2 = d.fetch_update_row()
        assert np.array_equal(pos2, pos)
        same_bits(val2, val, "list values after a sparse panel")
        same_bits(d.download_coefficients(), coeff, "coefficients after a sparse panel")
        assert d.paths() == paths
        rc = np.resize(y[1], mat.N)
        d.dual_begin(rc, np.zeros(mat.N, np.uint8), np.ones(mat.N))
        same_rows(d.column_dots_panel_sparse(y[:4], t, sc.mask(name, "random")),
                  sc.filtered(ref[:4], sc.mask(name, "random"), t), "sparse panel in dual mode")
        same_bits(d.dual_download_reduced_costs(), rc, "reduced costs after a sparse panel")
    finally:
        d.close()


def test_dense_and_sparse_panels_share_their_buffers(monkeypatch):
    for name in ("quad", "dense13"):
        d = handle(name, sc.CASES[name][2], monkeypatch)
        y, ref = sc.vectors(name), sc.reference(name)
        t = sc.tolerances(name, "all")["median"]
        for k_sparse, k_dense in ((17, 5), (3, 17)):
            same_rows(d.column_dots_panel_sparse(y[:k_sparse], t),
                      sc.filtered(ref[:k_sparse], sc.mask(name, "all"), t), f"{name} sparse")
            same_bits(d.column_dots_panel(y[:k_dense]), ref[:k_dense], f"{name} dense after sparse")
            dense_record = d.last_panel()
            same_rows(d.column_dots_panel_sparse(y[:k_sparse], 0.0, sc.mask(name, "random")),
                      sc.filtered(ref[:k_sparse], sc.mask(name, "random"), 0.0),
                      f"{name} sparse after dense")
            assert d.last_panel() == dense_record  # the sparse call keeps its own record


def test_nan_results_are_dropped_and_infinite_ones_kept(monkeypatch):
    name = "edge"
    mat = sc.matrix(name)
    y = sc.vectors(name)[:2].copy()
    y[0, 3], y[0, 20], y[1, 11] = np.inf, -np.inf, -np.inf
    cols = np.arange(mat.N)
    with np.errstate(invalid="ignore"):
        ref = np.stack([column_scalar_products(mat, cols, v) for v in y])
    assert np.isnan(ref[0]).any() and np.isposinf(ref[0]).any() and np.isneginf(ref).any()
    d = handle(name, {}, monkeypatch)
    for which in ("all", "random"):
        for t in (0.0, 1.0, np.finfo(np.float64).max, np.inf):
            want = sc.filtered(ref, sc.mask(name, which), t)
            got = d.column_dots_panel_sparse(y, t, sc.mask(name, which))
            same_rows(got, want, f"non-finite mask={which} tol={t}")
            assert not np.isnan(got[2]).any()
            if t < np.inf:
                assert np.isinf(got[2]).sum() == (np.isinf(ref) & sc.mask(name, which)).sum() > 0
            else:
                assert got[0][2] == 0
