"""The numpy reference of the row append (tests/append_cases.py) against a
matrix built from scratch, and LinearProgram.with_rows against the same.

merge() follows the device's scheme (rank, count, scan, move, scatter);
scratch() sorts the triplets of the extended matrix. They must agree array for
array, CSC and CSR, on every case, and the case table must hold the shapes the
GPU tests rely on. No GPU is used.
"""
import numpy as np
import pytest

import append_cases as ac
from mi_glop.lp import LinearProgram

ARRAYS = ("starts", "rows", "vals", "t_starts", "t_cols", "t_vals")


@pytest.mark.parametrize("name", ac.NAMES)
def test_merge_equals_the_matrix_built_from_scratch(name):
    c = ac.case(name)
    m, got = ac.merged(c)
    m2, r, cl, v = ac.triplets(c)
    assert m == m2 == c.m + sum(len(a[0]) - 1 for a in c.appends)
    want = ac.scratch(m, c.n, r, cl, v)
    for key in ARRAYS:
        assert got[key].dtype == want[key].dtype, key
        assert got[key].tobytes() == want[key].tobytes(), key


@pytest.mark.parametrize("name", ac.NAMES)
def test_with_rows_is_the_extended_lp(name):
    c = ac.case(name)
    lp = LinearProgram(c.m, c.n, c.col_starts, c.row_idx, c.vals, np.zeros(c.n), np.ones(c.n),
                       np.zeros(c.m), np.ones(c.m), np.ones(c.n))
    for i, (rs, cols, vals) in enumerate(c.appends):
        k = len(rs) - 1
        lp = lp.with_rows(rs, cols, vals, np.full(k, -1.0 - i), np.full(k, np.inf))
    m, starts, rows, vals = ac.extended_csc(c)
    assert lp.m == m and lp.n == c.n and lp.validate()
    assert lp.col_starts.tobytes() == starts.tobytes()
    assert lp.row_idx.dtype == np.int32 and lp.row_idx.tobytes() == rows.tobytes()
    assert lp.vals.tobytes() == vals.tobytes()
    assert len(lp.row_lb) == len(lp.row_ub) == m
    assert lp.row_lb[c.m] == -1.0 and lp.row_ub[-1] == np.inf


def test_the_cases_reach_the_kernels_limits():
    ks = {len(a[0]) - 1 for c in ac.CASES for a in c.appends}
    assert {1, 2, 17, 65} <= ks
    assert any(c.m == 0 for c in ac.CASES) and any(len(c.appends) == 2 for c in ac.CASES)
    assert any(c.n % 64 != 0 and c.n > 2 * ac.TILE for c in ac.CASES)
    assert any(c.n > ac.TILE * ac.THREADS for c in ac.CASES)
    lengths = np.diff(ac.case("column_lengths").col_starts)
    assert {0, 31, 32, 33} <= set(lengths.tolist()) and lengths.max() > 2 * ac.THREADS
    for c in ac.CASES:
        assert c.long_columns == bool(np.diff(c.col_starts).max(initial=0) > ac.SHORT_COLUMN)
    c = ac.case("k17")
    rs, cols, _ = c.appends[0]
    per_col = np.bincount(cols, minlength=c.n)
    # All rows but the empty one; the full row alone; it, the first and the last.
    assert per_col[0] == 16 and per_col[1] == 1 and per_col[2] == 3
    big = ac.case("k65")
    per_col = np.bincount(big.appends[0][1], minlength=big.n)
    # In no row, in the first and the last row only, in all k rows.
    assert per_col[0] == 0 and per_col[50] == 2 and per_col[99] == 65
    assert c.col_starts[4] == c.col_starts[3] and per_col[3] > 0  # an empty column gains
    assert 0 in np.diff(rs) and c.n in np.diff(rs)  # an empty row, a full row
    d = ac.case("dense_block")
    full = np.flatnonzero(np.diff(d.col_starts) == d.m)
    _, starts, _, _ = ac.extended_csc(d)
    still = np.flatnonzero(np.diff(starts) == d.m + 2)
    assert len(full) == 6 and 0 < len(still) < len(full)
