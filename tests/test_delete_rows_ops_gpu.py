"""DeviceLp::DeleteRows through the probe, bit for bit against a fresh handle
created from the reduced matrix.

For every case of tests/delete_cases.py the handle that ran the case's steps
(deletes, and appends in the sequences) and the fresh one must hold the same
device matrix in every array: CSC, CSR, the dense column list and the dense
block (fetch_matrix), which must also be the numpy reference's. last_delete
must report the compaction on the device (path 1), the move shapes the case's
own column and row lengths ask for, and between 1 and m + 64 bytes sent up,
whatever nnz is. On the same pairs of handles a handful of older operations
must agree bit for bit and in the kernels they report: pricing, row sums, the
column-dot panel and the row-sum panel. With MILP_SHARDS=2 the delete is the
full upload (path 2) and the operations still agree; with no row kept it is
the full upload too, equal to a fresh handle without rows.
"""
import functools

import numpy as np
import pytest

import delete_cases as dc
import devop
import devop_matrix_delete as dmd

pytestmark = pytest.mark.gpu

SWITCHES = ("MILP_DENSE_BLOCK", "MILP_SHARDS", "MILP_SHARD_DEVICES", "MILP_SMALL_FUSED",
            "MILP_SMALL_BATCH", "MILP_ROWWISE_LIST", "MILP_MEDIUM", "MILP_FULL_ROWS")
MATRIX = ("starts", "rows", "vals", "t_starts", "t_cols", "t_vals", "dense_cols", "dense_block")


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
    yield
    _pair.cache_clear()


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A device error is never part of a test here: after one, nothing more
    is started on the GPU."""
    yield
    if devop.device_error is not None:
        pytest.exit(f"device error: {devop.device_error}", returncode=3)


def run_steps(c):
    """A handle created from the case's A on which its steps ran, and the
    (step index, rows before, last_delete) of every delete."""
    a = dmd.DeleteDevOp(c.m, c.n, c.col_starts, c.row_idx, c.vals)
    records = []
    for i, (kind, arg) in enumerate(c.steps):
        if kind == "append":
            a.append_rows(*arg)
            continue
        _, r, _, _ = dc.triplets(c, i)
        before = a.m
        a.delete_rows(arg, int(np.count_nonzero(arg[r])))
        records.append((i, before, a.last_delete()))
    return a, records


@functools.lru_cache(maxsize=None)
def _pair(name):
    """(edited handle, its delete records, fresh handle); the MILP_* switches
    of the case are in the environment (pair())."""
    c = dc.case(name)
    a, records = run_steps(c)
    m, starts, rows, vals = dc.reduced_csc(c)
    b = dmd.DeleteDevOp(m, c.n, starts, rows, vals)
    return a, records, b


def pair(name, monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for key, value in dc.case(name).env.items():
        monkeypatch.setenv(key, value)
    return _pair(name)


def same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("name", dc.NAMES)
def test_compacted_matrix_is_the_fresh_upload(name, monkeypatch):
    c = dc.case(name)
    a, records, b = pair(name, monkeypatch)
    assert (a.m, a.N, a.nnz) == (b.m, b.N, b.nnz)
    m, starts, _, _ = dc.reduced_csc(c)
    full = int(np.count_nonzero(np.diff(starts) == m))  # at most these are dense columns
    got, fresh = a.fetch_matrix(full), b.fetch_matrix(full)
    for key in MATRIX:
        assert same(got[key], fresh[key]), key
    m_want, want = dc.scratch(c)
    assert m_want == a.m
    for key in MATRIX[:6]:
        assert same(got[key], want[key]), key
    assert len(records) == sum(kind == "delete" for kind, _ in c.steps)
    for i, before, rec in records:
        mask = c.steps[i][1]
        _, r, _, _ = dc.triplets(c, i)
        assert rec["path"] == 1 and rec["rows"] == int(mask.sum())
        assert rec["entries"] == int(np.count_nonzero(mask[r]))
        assert 1 <= rec["bytes_up"] <= before + 64
        assert (rec["column_shapes"], rec["row_shapes"]) == dc.move_shapes(c, i)
    if c.env.get("MILP_DENSE_BLOCK") == "force":
        # Column 3 misses row 2 alone before; the delete makes it full, and it
        # enters the dense block beside the columns that were full already.
        now_full = np.flatnonzero(np.diff(starts) == m)
        assert 3 not in np.flatnonzero(np.diff(c.col_starts) == c.m)
        assert now_full[:4].tolist() == [0, 1, 2, 3]
        assert got["dense_cols"].tolist() == now_full.tolist()
        assert len(got["dense_block"]) == len(now_full) * a.m


def older_operations(handles, m, big_n):
    rng = np.random.default_rng(11)
    y = rng.uniform(-2.0, 2.0, m)
    cost = rng.uniform(-2.0, 2.0, big_n)
    x = rng.uniform(-2.0, 2.0, big_n)
    panel_y = rng.uniform(-2.0, 2.0, (5, m))
    panel_x = rng.uniform(-2.0, 2.0, (5, big_n))
    results = []
    for d in handles:
        d.set_mask(np.ones(big_n, bool))
        results.append({"pricing": d.pricing(cost, y), "column_dots": d.last_column_dots(),
                        "row_sums": d.row_sums(x, False, -1.0),
                        "panel": d.column_dots_panel(panel_y), "last_panel": d.last_panel(),
                        "row_panel": d.row_sums_panel(panel_x),
                        "last_row_panel": d.last_row_panel()})
    got, fresh = results
    for key in ("pricing", "row_sums", "panel", "row_panel"):
        assert same(got[key], fresh[key]), key
    for key in ("column_dots", "last_panel", "last_row_panel"):
        assert got[key] == fresh[key], key


@pytest.mark.parametrize("name", dc.NAMES)
def test_older_operations_agree_on_the_pair(name, monkeypatch):
    a, _, b = pair(name, monkeypatch)
    older_operations((a, b), a.m, a.N)


def test_column_shards_take_the_full_upload(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    monkeypatch.setenv("MILP_SHARDS", "2")
    c = dc.case("rows_513")
    a, records = run_steps(c)
    assert [rec["path"] for _, _, rec in records] == [2]
    for i, _, rec in records:
        assert rec["rows"] == int(c.steps[i][1].sum())
    m, starts, rows, vals = dc.reduced_csc(c)
    b = dmd.DeleteDevOp(m, c.n, starts, rows, vals)
    got, fresh = a.fetch_matrix(), b.fetch_matrix()
    for key in MATRIX:
        assert same(got[key], fresh[key]), key
    older_operations((a, b), a.m, a.N)


def test_no_row_kept_takes_the_full_upload(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    c = dc.case("shapes")
    a = dmd.DeleteDevOp(c.m, c.n, c.col_starts, c.row_idx, c.vals)
    a.delete_rows(np.ones(c.m, bool), len(c.row_idx))
    rec = a.last_delete()
    assert (rec["path"], rec["rows"], rec["entries"]) == (2, c.m, len(c.row_idx))
    b = dmd.DeleteDevOp(0, c.n, np.zeros(c.n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    assert (a.m, a.N, a.nnz) == (0, c.n, 0)
    got, fresh = a.fetch_matrix(), b.fetch_matrix()
    for key in MATRIX:
        assert same(got[key], fresh[key]), key
