"""DeviceLp::ColumnCutsPanel through the probe, exactly equal to the numpy
reference of tests/gomory_cases.py (device_ref.column_scalar_products, the rule
of include/mi_lp.h mi_lp_row_gomory_cuts, column_scalar_products again, one
subtraction and the filter).

Every case of tests/gomory_cases.py runs with k vectors for every panel width,
for padding and for several panels, under both variants of the per-column
inputs and each drop tolerance: row_starts and columns are compared as
integers, coefficients and summaries on 64-bit patterns; the call without
lists must give the same summaries; last_cuts must report the kernels the case
was written for, the tiles of the case and at most 40 bytes per vector, 64 per
panel and 12 per kept entry brought down (nothing that grows with N).
tests/test_gomory_ref_cpu.py shows that the inputs contain the tie, the zero
second pass, the NaN, the tolerance hits and the bad columns the kernels have
to get right. Then: no units at all, an overflow that makes NaN coefficients,
the dense block forced and off, records beyond k left alone, and cut, dense,
sparse and penalty panels in turn over their shared buffers.
"""
import functools

import numpy as np
import pytest

import devop
import devop_cuts as dc
import gomory_cases as gc
import panel_sparse_cases as sc
import penalty_cases as pn
from device_ref import bits

pytestmark = pytest.mark.gpu

SWITCHES = ("MILP_DENSE_BLOCK", "MILP_SHARDS", "MILP_SHARD_DEVICES", "MILP_SMALL_FUSED",
            "MILP_SMALL_BATCH", "MILP_ROWWISE_LIST", "MILP_MEDIUM", "MILP_FULL_ROWS")


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
    return dc.CutsDevOp(mat.m, mat.n, mat.col_starts, mat.row_idx, mat.vals)


def handle(name, env, monkeypatch):
    """The MILP_* switches are read when a handle is created."""
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    return _cached_handle(name, tuple(sorted(env.items())))


def same_summaries(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    for f in ("max_abs", "min_abs"):
        bad = np.nonzero(bits(got[f]) != bits(want[f]))[0]
        assert len(bad) == 0, (f"{what} {f}: {len(bad)} of {len(want)} differ, first at "
                               f"{bad[0]}: device {got[f][bad[0]].hex()} reference "
                               f"{want[f][bad[0]].hex()}")
    for f in ("count", "bad_count", "max_col", "min_col"):
        assert np.array_equal(got[f], want[f]), (what, f, got[f], want[f])


def same_cuts(got, want, what):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]), (what, "row_starts", got[0], want[0])
    assert np.array_equal(got[1], want[1]), (what, "columns")
    bad = np.nonzero(bits(got[2]) != bits(want[2]))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(want[2])} coefficients differ, first at "
                           f"entry {bad[0]} (column {want[1][bad[0]]}): device "
                           f"{got[2][bad[0]].hex()} reference {want[2][bad[0]].hex()}")
    same_summaries(got[3], want[3].astype(dc.SUMMARY), what)


def expected_record(name, env, k, lists, kept):
    """The kernel choice of the dense panel (test_panel_ops_gpu.py states the
    same rule) and the tiles of the case."""
    last = k - 16 * ((k - 1) // 16)
    dense = name.startswith("dense") and env.get("MILP_DENSE_BLOCK") == "force"
    tiles, tiles_n = gc.tiles(name)
    return {"sparse": "long_columns" if name == "wave" else "short_columns", "dense": dense,
            "panels": (k + 15) // 16, "width": 1 if last == 1 else (4 if last <= 4 else 16),
            "tiles": tiles, "structural_tiles": tiles_n, "lists": lists, "kept": kept}


def check_record(d, name, env, k, lists, kept, what):
    record = d.last_cuts()
    print(what, record)
    panels = (k + 15) // 16
    assert record.pop("bytes_down") <= 40 * k + 64 * panels + 12 * kept, what
    assert record == expected_record(name, env, k, lists, kept), (what, record)


def run(d, name, env, k, variant, drop, what):
    p = gc.inputs(name, variant)
    tolerance = gc.drop_tolerances(name, variant)[drop]
    want = gc.prefix(gc.expected(name, variant, drop), k)
    args = (gc.vectors(name)[:k], p["status"], p["unit"], p["f0"][:k], p["row_unit"][:k],
            p["zero_tolerance"], tolerance)
    got = d.column_cuts_panel(*args)
    same_cuts(got, want, what)
    check_record(d, name, env, k, True, int(want[0][k]), what)
    alone = d.column_cuts_panel(*args, lists=False)
    assert alone[0] is None and alone[1] is None and alone[2] is None
    same_summaries(alone[3], want[3].astype(dc.SUMMARY), what + " summaries only")
    check_record(d, name, env, k, False, 0, what + " summaries only")
    return got


CASE_KS = [(name, k) for name in gc.NAMES for k in gc.KS if k <= gc.max_k(name)]


@pytest.mark.parametrize("name,k", CASE_KS)
def test_cuts_case(name, k, monkeypatch):
    env = gc.environment(name)
    d = handle(name, env, monkeypatch)
    for variant in gc.VARIANTS:
        for drop in gc.DROPS:
            run(d, name, env, k, variant, drop, f"{name} k={k} variant={variant} drop={drop}")


@pytest.mark.parametrize("name", gc.NAMES)
def test_without_units(name, monkeypatch):
    env = gc.environment(name)
    d = handle(name, env, monkeypatch)
    mat = sc.matrix(name)
    k = min(5, gc.max_k(name))
    p = gc.inputs(name, "a")
    _, bad, c = gc.reference(mat, gc.vectors(name)[:k], p["status"], None, p["f0"][:k],
                             p["row_unit"][:k], p["zero_tolerance"], a=gc.alpha(name)[:k])
    want = gc.cut_lists(c, 0.0) + (gc.summarize(c, 0.0, bad),)
    got = d.column_cuts_panel(gc.vectors(name)[:k], p["status"], None, p["f0"][:k],
                              p["row_unit"][:k], p["zero_tolerance"], 0.0)
    same_cuts(got, want, f"{name} without units")
    with_units = gc.prefix(gc.expected(name, "a", "zero"), k)
    assert not np.array_equal(bits(got[2]), bits(with_units[2]))  # the units mattered


def test_an_overflow_gives_nan_coefficients_that_are_dropped_and_counted(monkeypatch):
    # alpha * unit overflows on the integer columns of vector 0: t = inf,
    # f = inf - inf = NaN, g = NaN; the slack part carries it through the
    # second pass, and c is NaN on the columns that meet such a row.
    name, k = "edge", 3
    d = handle(name, gc.environment(name), monkeypatch)
    mat = sc.matrix(name)
    p = gc.inputs(name, "a")
    y = np.array(gc.vectors(name)[[0, 4, 5]])
    y[0] *= np.ldexp(1.0, 1010)
    _, bad, c = gc.reference(mat, y, p["status"], p["unit"], p["f0"][:k], p["row_unit"][:k], 0.0)
    assert np.isnan(c[0]).any() and not np.isnan(c[1:]).any() and np.isinf(c[0]).any()
    want = gc.cut_lists(c, 0.0) + (gc.summarize(c, 0.0, bad),)
    assert want[3]["bad_count"][0] == np.isnan(c[0]).sum() + bad[0] > bad[0]
    got = d.column_cuts_panel(y, p["status"], p["unit"], p["f0"][:k], p["row_unit"][:k], 0.0, 0.0)
    same_cuts(got, want, "overflow")


def test_dense_columns_through_both_kernels(monkeypatch):
    # The same full columns with the dense block forced and off: the same cuts.
    for mode in ("force", "off"):
        env = {"MILP_DENSE_BLOCK": mode}
        d = handle("dense13", env, monkeypatch)
        for k in (5, 17):
            for variant in gc.VARIANTS:
                run(d, "dense13", env, k, variant, "median",
                    f"dense13 {mode} k={k} variant={variant}")


def test_records_beyond_k_are_untouched(monkeypatch):
    name, k = "quad", 5
    d = handle(name, gc.environment(name), monkeypatch)
    p = gc.inputs(name, "a")
    out = np.zeros(k + 3, dc.SUMMARY)
    raw = out.view(np.uint8)
    raw[:] = 0xA5
    got = d.column_cuts_panel(gc.vectors(name)[:k], p["status"], p["unit"], p["f0"][:k],
                              p["row_unit"][:k], p["zero_tolerance"], 0.0, summaries=out)
    same_cuts(got, gc.prefix(gc.expected(name, "a", "zero"), k), "in place")
    assert np.all(raw[k * 32:] == 0xA5)


def test_cut_dense_sparse_and_penalty_panels_share_their_buffers(monkeypatch):
    for name in ("quad", "dense13"):
        env = gc.environment(name)
        d = handle(name, env, monkeypatch)
        y, ref = sc.vectors(name), sc.reference(name)
        t = sc.tolerances(name, "all")["median"]
        q = pn.inputs(name, "a")
        for k_cut, k_dense, k_sparse, k_pen in ((17, 5, 3, 4), (3, 17, 16, 33)):
            run(d, name, env, k_cut, "a", "median", f"{name} cuts first")
            got = d.column_dots_panel(y[:k_dense])
            assert np.array_equal(bits(got), bits(ref[:k_dense])), f"{name} dense after cuts"
            dense_record = d.last_panel()
            run(d, name, env, k_cut, "b", "zero", f"{name} cuts after dense")
            starts, cols, vals = d.column_dots_panel_sparse(y[:k_sparse], t)
            want = sc.filtered(ref[:k_sparse], sc.mask(name, "all"), t)
            assert np.array_equal(starts, want[0]) and np.array_equal(cols, want[1])
            assert np.array_equal(bits(vals), bits(want[2])), f"{name} sparse after cuts"
            sparse_record = d.last_panel_sparse()
            run(d, name, env, k_cut, "a", "hit", f"{name} cuts after sparse")
            pen = d.column_penalties_panel(pn.vectors(name)[:k_pen], q["d"], q["status"],
                                           q["unit"], q["down"][:k_pen], q["up"][:k_pen],
                                           q["tolerance"])
            want_pen = pn.expected(name, "a")[:k_pen]
            for f in want_pen.dtype.names:
                assert np.array_equal(np.ascontiguousarray(pen[f]).view(np.uint8),
                                      np.ascontiguousarray(want_pen[f]).view(np.uint8)), \
                    f"{name} penalties after cuts: {f}"
            penalty_record = d.last_penalties()
            run(d, name, env, k_cut, "b", "median", f"{name} cuts after penalties")
            # The cuts keep their own record.
            assert d.last_panel() == dense_record and d.last_panel_sparse() == sparse_record
            assert d.last_penalties() == penalty_record
