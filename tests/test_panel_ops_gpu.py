"""DeviceLp::ColumnDotsPanel through the probe, bit for bit against
tests/device_ref.py column_scalar_products.

Every case of tests/panel_cases.py (short columns, long columns, the dense
block at every tail and step parity) runs with k vectors for every panel
width, for padding and for several panels; all k * N results are compared on
64-bit patterns and last_panel must report the kernels the case was written
for. tests/test_panel_ref_cpu.py shows that these inputs separate summation
orders. Then: the dense block switched off, two column shards, that a panel
leaves the update row, the paths record and the dual-mode reduced costs
alone, and that nothing beyond k * N results is written.
"""
import functools

import numpy as np
import pytest

import devop
import devop_panel
import panel_cases as pc
from device_ref import bits

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
    mat = pc.matrix(name)
    return devop_panel.PanelDevOp(mat.m, mat.n, mat.col_starts, mat.row_idx, mat.vals)


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


def expected_panel(name, env, k):
    last = k - 16 * ((k - 1) // 16)
    dense = name.startswith("dense") and env.get("MILP_DENSE_BLOCK") == "force"
    return {"sparse": "long_columns" if name == "wave" else "short_columns", "dense": dense,
            "panels": (k + 15) // 16, "width": 1 if last == 1 else (4 if last <= 4 else 16)}


def run_panel(name, env, k, monkeypatch):
    d = handle(name, env, monkeypatch)
    got = d.column_dots_panel(pc.vectors(name)[:k])
    p = d.last_panel()
    print(name, env, "k", k, p)
    same_bits(got, pc.reference(name)[:k], f"{name} k={k}")
    assert p == expected_panel(name, env, k), (name, k, p)
    return d


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_panel_case(name, k, monkeypatch):
    run_panel(name, pc.CASES[name][2], k, monkeypatch)


def test_dense_columns_through_the_csc_kernel(monkeypatch):
    # The same full columns without the dense block: same bits.
    for k in (5, 17):
        run_panel("dense23", {"MILP_DENSE_BLOCK": "off"}, k, monkeypatch)


def test_two_column_shards(monkeypatch):
    for k in (3, 17):
        run_panel("quad", {"MILP_SHARDS": "2"}, k, monkeypatch)


def test_panel_leaves_solve_state_alone(monkeypatch):
    name = "quad"
    mat, y = pc.matrix(name), pc.vectors(name)
    d = handle(name, {}, monkeypatch, cached=False)
    try:
        d.set_mask(np.ones(mat.N, bool))
        rows = np.array([3, 17, 40, 41, 90], np.int32)
        d.update_row_row_wise(rows, y[0], 2, DROP)
        pos, val = d.fetch_update_row()
        coeff = d.download_coefficients()
        paths = d.paths()
        assert len(pos) > 0
        d.column_dots_panel(y[:5])
        d.column_dots_panel(y[:17])
        pos2, val2 = d.fetch_update_row()
        assert np.array_equal(pos2, pos)
        same_bits(val2, val, "list values after a panel")
        same_bits(d.download_coefficients(), coeff, "coefficients after a panel")
        assert d.paths() == paths
        rc = np.resize(y[1], mat.N)
        d.dual_begin(rc, np.zeros(mat.N, np.uint8), np.ones(mat.N))
        same_bits(d.column_dots_panel(y[:4]), pc.reference(name)[:4], "panel in dual mode")
        same_bits(d.dual_download_reduced_costs(), rc, "reduced costs after a panel")
    finally:
        d.close()


def test_nothing_is_written_beyond_k_rows(monkeypatch):
    for name in ("quad", "dense13"):
        d = handle(name, pc.CASES[name][2], monkeypatch)
        N = pc.matrix(name).N
        for fill in (np.float64(-7.25), np.float64("nan")):
            out = np.full(4 * N + 7, fill)
            d.column_dots_panel(pc.vectors(name)[:3], out=out)
            same_bits(out[:3 * N].reshape(3, N), pc.reference(name)[:3], f"{name} k=3")
            assert np.all(bits(out[3 * N:]) == bits(fill)), name
