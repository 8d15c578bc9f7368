"""DeviceLp::AppendRows through the probe, bit for bit against a fresh handle
created from the extended matrix.

For every case of tests/append_cases.py the handle that appended and the fresh
one must hold the same device matrix in every array: CSC, CSR, the dense
column list and the dense block (fetch_matrix), which must also be the numpy
reference's. last_append must report the device merge (path 1), the move
kernels the case was written for, and at most 24 (e + k) + 16 (k + 1) + 64
bytes sent up, whatever nnz is. On the same pairs of handles a handful of
older operations must agree bit for bit and in the kernels they report:
pricing, row sums, both update rows (a new row among the filtered rows), the
column-dot panel and the row-sum panel.
"""
import functools

import numpy as np
import pytest

import append_cases as ac
import devop
import devop_matrix as dm

pytestmark = pytest.mark.gpu

SWITCHES = ("MILP_DENSE_BLOCK", "MILP_SHARDS", "MILP_SHARD_DEVICES", "MILP_SMALL_FUSED",
            "MILP_SMALL_BATCH", "MILP_ROWWISE_LIST", "MILP_MEDIUM", "MILP_FULL_ROWS")
MATRIX = ("starts", "rows", "vals", "t_starts", "t_cols", "t_vals", "dense_cols", "dense_block")
OPS_CASES = ("k17", "column_lengths", "two_appends", "dense_block", "m0")


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


@functools.lru_cache(maxsize=None)
def _pair(name):
    """(appended handle, its last_append records, fresh handle); the MILP_*
    switches of the case are in the environment (pair())."""
    c = ac.case(name)
    a = dm.MatrixDevOp(c.m, c.n, c.col_starts, c.row_idx, c.vals)
    records = []
    for rs, cols, vals in c.appends:
        a.append_rows(rs, cols, vals)
        records.append(a.last_append())
    m, starts, rows, vals = ac.extended_csc(c)
    b = dm.MatrixDevOp(m, c.n, starts, rows, vals)
    return a, records, b


def pair(name, monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for key, value in ac.case(name).env.items():
        monkeypatch.setenv(key, value)
    return _pair(name)


def same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("name", ac.NAMES)
def test_appended_matrix_is_the_fresh_upload(name, monkeypatch):
    c = ac.case(name)
    a, records, b = pair(name, monkeypatch)
    assert (a.m, a.N, a.nnz) == (b.m, b.N, b.nnz)
    got, fresh = a.fetch_matrix(), b.fetch_matrix()
    for key in MATRIX:
        assert same(got[key], fresh[key]), key
    m, r, cl, v = ac.triplets(c)
    want = ac.scratch(m, c.n, r, cl, v)
    for key in MATRIX[:6]:
        assert same(got[key], want[key]), key
    for (rs, _, _), rec in zip(c.appends, records):
        k, e = len(rs) - 1, int(rs[-1])
        assert rec["path"] == 1 and rec["rows"] == k and rec["entries"] == e
        assert 0 < rec["bytes_up"] <= 24 * (e + k) + 16 * (k + 1) + 64
        shapes = dm.MOVE_COLUMN_PER_THREAD | (dm.MOVE_COLUMN_PER_WORKGROUP if c.long_columns else 0)
        assert rec["move_shapes"] == shapes


def test_dense_block_keeps_the_columns_every_new_row_hits(monkeypatch):
    c = ac.case("dense_block")
    a, _, b = pair("dense_block", monkeypatch)
    got = a.fetch_matrix()
    _, starts, _, _ = ac.extended_csc(c)
    still_full = np.flatnonzero(np.diff(starts) == a.m)
    assert got["dense_cols"].tolist() == still_full.tolist() == [0, 1, 2]
    assert len(got["dense_block"]) == 3 * a.m


@pytest.mark.parametrize("name", OPS_CASES)
def test_older_operations_agree_on_the_pair(name, monkeypatch):
    c = ac.case(name)
    a, _, b = pair(name, monkeypatch)
    m, big_n = a.m, a.N
    rng = np.random.default_rng(11)
    y = rng.uniform(-2.0, 2.0, m)
    cost = rng.uniform(-2.0, 2.0, big_n)
    x = rng.uniform(-2.0, 2.0, big_n)
    rho = rng.uniform(-2.0, 2.0, m)
    filtered = sorted({0, c.m, m - 1})  # c.m: the first new row
    panel_y = rng.uniform(-2.0, 2.0, (5, m))
    panel_x = rng.uniform(-2.0, 2.0, (5, big_n))
    results = []
    for d in (a, b):
        d.set_mask(np.ones(big_n, bool))
        out = {"pricing": d.pricing(cost, y), "column_dots": d.last_column_dots(),
               "row_sums": d.row_sums(x, False, -1.0)}
        d.update_row_row_wise(filtered, rho, 2, 1e-11)
        out["row_wise"] = d.fetch_update_row()
        out["row_wise_paths"] = d.paths()
        d.update_row_column_wise(rho, 1e-11)
        out["column_wise"] = d.fetch_update_row()
        out["column_wise_paths"] = d.paths()
        out["panel"] = d.column_dots_panel(panel_y)
        out["last_panel"] = d.last_panel()
        out["row_panel"] = d.row_sums_panel(panel_x)
        out["last_row_panel"] = d.last_row_panel()
        results.append(out)
    got, fresh = results
    for key in ("pricing", "row_sums", "panel", "row_panel"):
        assert same(got[key], fresh[key]), key
    for key in ("row_wise", "column_wise"):
        assert same(got[key][0], fresh[key][0]) and same(got[key][1], fresh[key][1]), key
        assert len(got[key][0]) > 0, key
    for key in ("column_dots", "row_wise_paths", "column_wise_paths", "last_panel",
                "last_row_panel"):
        assert got[key] == fresh[key], key
