"""DeviceLp::ColumnPenaltiesPanel through the probe, exactly equal to the numpy
reference of tests/penalty_cases.py (device_ref.column_scalar_products followed
by the rule of include/mi_lp.h mi_lp_row_penalties).

Every case of tests/penalty_cases.py runs with k vectors for every panel width,
for padding and for several panels, under both variants of the per-column
inputs: the penalties are compared on 64-bit patterns, columns and counts as
integers; last_penalties must report the kernels the case was written for, the
tiles of the case and at most 32 bytes per vector plus 64 per panel brought
down (nothing that grows with N). tests/test_penalties_ref_cpu.py shows that
the inputs contain the ties, the empty direction, the NaN, the tolerance hit
and the unit-decided minima the kernels have to get right. Then: no units at
all, the dense block forced and off, two column shards, records beyond k left
alone, and dense, sparse and penalty panels in turn over their shared buffers.
"""
import functools

import numpy as np
import pytest

import devop
import devop_penalties as dpn
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
    return dpn.PenaltiesDevOp(mat.m, mat.n, mat.col_starts, mat.row_idx, mat.vals)


def handle(name, env, monkeypatch):
    """The MILP_* switches are read when a handle is created."""
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    return _cached_handle(name, tuple(sorted(env.items())))


def same_records(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    for f in ("down", "up"):
        bad = np.nonzero(bits(got[f]) != bits(want[f]))[0]
        assert len(bad) == 0, (f"{what} {f}: {len(bad)} of {len(want)} differ, first at "
                               f"{bad[0]}: device {got[f][bad[0]].hex()} reference "
                               f"{want[f][bad[0]].hex()}")
    for f in ("down_col", "up_col", "down_count", "up_count"):
        assert np.array_equal(got[f], want[f]), (what, f, got[f], want[f])


def expected_record(name, env, k):
    """The kernel choice of the dense panel (test_panel_ops_gpu.py states the
    same rule) and the tiles of the case."""
    last = k - 16 * ((k - 1) // 16)
    dense = name.startswith("dense") and env.get("MILP_DENSE_BLOCK") == "force"
    return {"sparse": "long_columns" if name == "wave" else "short_columns", "dense": dense,
            "panels": (k + 15) // 16, "width": 1 if last == 1 else (4 if last <= 4 else 16),
            "tiles": pn.tiles(name)}


def run(d, name, env, k, variant, what, units=True, shards=1):
    p = pn.inputs(name, variant)
    unit = p["unit"] if units else None
    want = pn.expected(name, variant)[:k] if units else pn.reference(
        pn.alpha(name)[:k], p["d"], p["status"], None, p["down"][:k], p["up"][:k],
        p["tolerance"])
    got = d.column_penalties_panel(pn.vectors(name)[:k], p["d"], p["status"], unit,
                                   p["down"][:k], p["up"][:k], p["tolerance"])
    record = d.last_penalties()
    print(what, record)
    same_records(got, want, what)
    panels = (k + 15) // 16
    assert record.pop("bytes_down") <= shards * (32 * k + 64 * panels), what
    if shards == 1:
        assert record == expected_record(name, env, k), (what, record)
    return got


CASE_KS = [(name, k) for name in pn.NAMES for k in pn.KS if k <= pn.max_k(name)]


@pytest.mark.parametrize("name,k", CASE_KS)
def test_penalties_case(name, k, monkeypatch):
    env = pn.environment(name)
    d = handle(name, env, monkeypatch)
    for variant in pn.VARIANTS:
        run(d, name, env, k, variant, f"{name} k={k} variant={variant}")


@pytest.mark.parametrize("name", pn.NAMES)
def test_without_units(name, monkeypatch):
    env = pn.environment(name)
    d = handle(name, env, monkeypatch)
    k = min(5, pn.max_k(name))
    with_units = pn.expected(name, "a")[:k]
    got = run(d, name, env, k, "a", f"{name} without units", units=False)
    assert not np.array_equal(bits(got["down"]), bits(with_units["down"])) or \
        not np.array_equal(bits(got["up"]), bits(with_units["up"]))  # the units mattered


def test_dense_columns_through_both_kernels(monkeypatch):
    # The same full columns with the dense block forced and off: the same records.
    for mode in ("force", "off"):
        env = {"MILP_DENSE_BLOCK": mode}
        d = handle("dense13", env, monkeypatch)
        for k in (5, 17):
            for variant in pn.VARIANTS:
                run(d, "dense13", env, k, variant, f"dense13 {mode} k={k} variant={variant}")


@pytest.mark.parametrize("name", ["quad", "edge"])
def test_two_column_shards(name, monkeypatch):
    env = dict(pn.environment(name), MILP_SHARDS="2")
    d = handle(name, env, monkeypatch)
    for k in (3, 17):
        for variant in pn.VARIANTS:
            run(d, name, env, k, variant, f"{name} two shards k={k} variant={variant}", shards=2)


def test_records_beyond_k_are_untouched(monkeypatch):
    name, k = "quad", 5
    d = handle(name, pn.environment(name), monkeypatch)
    p = pn.inputs(name, "a")
    out = np.zeros(k + 3, dpn.RECORD)
    raw = out.view(np.uint8)
    raw[:] = 0xA5
    got = d.column_penalties_panel(pn.vectors(name)[:k], p["d"], p["status"], p["unit"],
                                   p["down"][:k], p["up"][:k], p["tolerance"], out=out)
    same_records(got, pn.expected(name, "a")[:k], "in place")
    assert np.all(raw[k * 32:] == 0xA5)


def test_dense_sparse_and_penalty_panels_share_their_buffers(monkeypatch):
    for name in ("quad", "dense13"):
        env = pn.environment(name)
        d = handle(name, env, monkeypatch)
        y, ref = sc.vectors(name), sc.reference(name)
        t = sc.tolerances(name, "all")["median"]
        for k_pen, k_dense, k_sparse in ((17, 5, 3), (3, 17, 16)):
            run(d, name, env, k_pen, "a", f"{name} penalties first")
            got = d.column_dots_panel(y[:k_dense])
            assert np.array_equal(bits(got), bits(ref[:k_dense])), f"{name} dense after penalties"
            dense_record = d.last_panel()
            run(d, name, env, k_pen, "b", f"{name} penalties after dense")
            starts, cols, vals = d.column_dots_panel_sparse(y[:k_sparse], t)
            want = sc.filtered(ref[:k_sparse], sc.mask(name, "all"), t)
            assert np.array_equal(starts, want[0]) and np.array_equal(cols, want[1])
            assert np.array_equal(bits(vals), bits(want[2])), f"{name} sparse after penalties"
            sparse_record = d.last_panel_sparse()
            run(d, name, env, k_pen, "a", f"{name} penalties after sparse")
            # The penalties keep their own record.
            assert d.last_panel() == dense_record and d.last_panel_sparse() == sparse_record
