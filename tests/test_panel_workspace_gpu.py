"""The two directions of the panel calls on ONE handle, through the probe
(tests/devop_row_panel.py): DeviceLp::ColumnDotsPanel / ColumnDotsPanelSparse
(k vectors -> column dots) and RowSumsPanel / RowSumsPanelFrom (k points ->
row sums) share the three shape-named buffers of the panel workspace, each
direction keeping something else in each of them. The calls alternate so that
every buffer grows under each of its roles and is then used by the other
direction, at a smaller and at a larger size.

Every result is compared on all 64 bits with the numpy references the case
files use (device_ref.column_scalar_products, RefState.row_sums), and after
every call the call's record must show ceil(k / 16) panels and the width of
the last one. `quad` (panel_cases, m = 96, N = 256) and `rows70`
(row_panel_cases, m = 70, N = 300) differ in the ratio of m to N. What a case
file lacks for the other direction's matrix is drawn here with a fixed seed
from the file's own generator (solveops_cases._family, panel_cases._values).
With two column shards the row sums stay on the unsplit handle while the
column dots go through the shards: both workspaces are live.
"""
import functools

import numpy as np
import pytest

import devop
import devop_row_panel
import panel_cases as pc
import panel_sparse_cases as psc
import row_panel_cases as rc
import solveops_cases as sc
from device_ref import RefState, bits, column_scalar_products

pytestmark = pytest.mark.gpu

SWITCHES = ("MILP_DENSE_BLOCK", "MILP_SHARDS", "MILP_SHARD_DEVICES", "MILP_SMALL_FUSED",
            "MILP_SMALL_BATCH", "MILP_ROWWISE_LIST", "MILP_MEDIUM", "MILP_FULL_ROWS",
            "MILP_DENSE_UNROLL", "MILP_EARLY_FLIPS")
CASES = ("quad", "rows70")
MAX_K = 33
OVERRIDE_K = 17
QUAD_POINT_SEED, QUAD_OVERRIDE_SEED = 710000, 720000
# (call, k): the directions alternate and every role of every buffer grows.
SEQUENCE = (("row_sums_panel", 1), ("column_dots_panel", 16), ("row_sums_panel_from", 17),
            ("column_dots_panel_sparse", 5), ("column_dots_panel", 33), ("row_sums_panel", 33),
            ("column_dots_panel", 1))


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A device error is never part of a test here: after one, nothing more
    is started on the GPU."""
    yield
    if devop.device_error is not None:
        pytest.exit(f"device error: {devop.device_error}", returncode=3)


def matrix(name):
    return pc.matrix(name) if name == "quad" else rc.matrix(name)


@functools.lru_cache(maxsize=None)
def vectors(name):
    """(MAX_K, m), read-only: the case file's own for quad, solveops_cases'
    pool of the same family for rows70."""
    y = pc.vectors(name) if name == "quad" else sc.vector_pool(name)
    assert y.shape == (MAX_K, matrix(name).m) and not y.flags.writeable
    return y


@functools.lru_cache(maxsize=None)
def dots_reference(name):
    """(MAX_K, N), read-only."""
    if name == "quad":
        return pc.reference(name)
    mat = matrix(name)
    out = np.stack([column_scalar_products(mat, np.arange(mat.N), y) for y in vectors(name)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def points(name):
    """(MAX_K, N), read-only: the case file's own for rows70 (NaN, inf and
    all-zero points included), row_panel_cases' family for quad."""
    if name != "quad":
        return rc.points(name)
    N = matrix(name).N
    x = np.stack([sc._family(np.random.default_rng(QUAD_POINT_SEED + j), N) for j in range(MAX_K)])
    x.setflags(write=False)
    return x


def _row_sums(name, x):
    ref = RefState(matrix(name))
    with np.errstate(invalid="ignore"):
        out = np.stack([ref.row_sums(p, None, 1.0) for p in x])
    assert sc.only_input_nans(out), name
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sums_reference(name):
    """(MAX_K, m), read-only."""
    return rc.reference(name) if name != "quad" else _row_sums(name, points(name))


@functools.lru_cache(maxsize=None)
def overrides(name):
    """(base, OVERRIDE_K sets of (cols, vals)): row_panel_cases' "k17" set for
    rows70, the same recipe for quad."""
    if name != "quad":
        return rc.override_set(name, "k17")
    N = matrix(name).N
    rng = np.random.default_rng(QUAD_OVERRIDE_SEED)
    base = sc._family(rng, N)
    base.setflags(write=False)
    sets = []
    for _ in range(OVERRIDE_K):
        count = int(rng.integers(1, 6))
        sets.append((rng.permutation(N)[:count].astype(np.int32), pc._values(rng, count)))
    return base, sets


@functools.lru_cache(maxsize=None)
def override_reference(name):
    """(OVERRIDE_K, m), read-only; point j does not depend on the others, so
    the first k rows are the reference of the first k sets."""
    if name != "quad":
        return rc.override_reference(name, "k17")
    base, sets = overrides(name)
    return _row_sums(name, rc.materialise(base, sets))


def make_handle(name, env, monkeypatch):
    """The MILP_* switches are read when a handle is created."""
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    mat = matrix(name)
    return devop_row_panel.RowPanelDevOp(mat.m, mat.n, mat.col_starts, mat.row_idx, mat.vals)


def same_bits(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {want.size} differ, first at {tuple(bad[0])}: "
                           f"device {got[tuple(bad[0])].hex()} reference "
                           f"{want[tuple(bad[0])].hex()}")


def panels_and_width(k):
    return {"panels": len(rc.panels(k)), "width": rc.width(rc.panels(k)[-1][1])}


def check_record(record, k, what):
    got = {key: record[key] for key in ("panels", "width")}
    assert got == panels_and_width(k), (what, record)


def run_step(d, name, call, k):
    what = f"{name} {call} k={k}"
    mat = matrix(name)
    if call == "row_sums_panel":
        same_bits(d.row_sums_panel(points(name)[:k]), sums_reference(name)[:k], what)
        p = d.last_row_panel()
        check_record(p, k, what)
        assert p["kernel"] == "direct" and p["overrides_up_bytes"] == 0, (what, p)
    elif call == "row_sums_panel_from":
        base, sets = overrides(name)
        starts, cols, vals = rc.flatten(sets[:k])
        same_bits(d.row_sums_panel_from(base, starts, cols, vals), override_reference(name)[:k],
                  what)
        p = d.last_row_panel()
        check_record(p, k, what)
        assert p["kernel"] == "direct", (what, p)
        assert p["overrides_up_bytes"] == 8 * mat.N + 12 * len(cols) + 8 * (k + 1), (what, p)
    elif call == "column_dots_panel":
        same_bits(d.column_dots_panel(vectors(name)[:k]), dots_reference(name)[:k], what)
        check_record(d.last_panel(), k, what)
    else:
        assert call == "column_dots_panel_sparse"
        structural = np.arange(mat.N) < mat.n
        want = psc.filtered(dots_reference(name)[:k], structural, 0.0)
        got = d.column_dots_panel_sparse(vectors(name)[:k], 0.0, structural)
        for g, w, part in zip(got[:2], want[:2], ("row_starts", "cols")):
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, part, g[:8], w[:8])
        same_bits(got[2], want[2], what)
        p = d.last_panel_sparse()
        check_record(p, k, what)
        assert p["kept"] == int(want[0][k]) > 0, (what, p)


@pytest.mark.parametrize("name", CASES)
def test_the_directions_alternate_and_every_role_grows(name, monkeypatch):
    d = make_handle(name, {}, monkeypatch)
    try:
        for call, k in SEQUENCE:
            run_step(d, name, call, k)
    finally:
        d.close()


@pytest.mark.parametrize("name", CASES)
def test_two_column_shards(name, monkeypatch):
    d = make_handle(name, {"MILP_SHARDS": "2"}, monkeypatch)
    try:
        for k in (5, 17):
            for call, _ in SEQUENCE:
                run_step(d, name, call, k)
    finally:
        d.close()
