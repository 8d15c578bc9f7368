"""The numpy reference of DeviceLp::DeleteRows (tests/delete_cases.py):
compact(), the device's scheme on the arrays of [A | I], against scratch(),
[A | I] built from the triplets of the reduced A, array for array on every
case; LinearProgram.without_rows against the same triplets; and the cases
themselves against the limits they were written for."""
import numpy as np
import pytest

import delete_cases as dc
from mi_glop.lp import LinearProgram

KEYS = ("starts", "rows", "vals", "t_starts", "t_cols", "t_vals")


def same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("name", dc.NAMES)
def test_compact_is_the_matrix_from_scratch(name):
    c = dc.case(name)
    m, got = dc.compacted(c)
    m_want, want = dc.scratch(c)
    assert m == m_want
    for key in KEYS:
        assert same(got[key], want[key]), key
    # [A | I]: every row ends in its slack, every slack column holds its row.
    n = c.n
    assert np.array_equal(got["t_cols"][got["t_starts"][1:] - 1], n + np.arange(m))
    assert np.array_equal(got["rows"][got["starts"][n:-1]], np.arange(m))


@pytest.mark.parametrize("name", [c.name for c in dc.CASES if c.steps[0][0] == "delete"])
def test_without_rows_is_the_reduced_lp(name):
    c = dc.case(name)
    mask = c.steps[0][1]
    rng = np.random.default_rng(3)
    lp = LinearProgram(c.m, c.n, c.col_starts, c.row_idx, c.vals, np.zeros(c.n), np.ones(c.n),
                       rng.uniform(-1, 0, c.m), rng.uniform(0, 1, c.m), rng.uniform(-1, 1, c.n))
    got = lp.without_rows(mask)
    m, starts, rows, vals = dc.reduced_csc(c, 1)
    assert got.m == m and got.n == c.n
    assert same(got.col_starts, starts) and same(got.row_idx, rows) and same(got.vals, vals)
    assert same(got.row_lb, lp.row_lb[~mask]) and same(got.row_ub, lp.row_ub[~mask])
    assert same(got.col_lb, lp.col_lb) and same(got.obj, lp.obj)


def test_without_rows_refuses_a_mask_of_another_length():
    c = dc.case("first_row")
    lp = LinearProgram(c.m, c.n, c.col_starts, c.row_idx, c.vals, np.zeros(c.n), np.ones(c.n),
                       np.zeros(c.m), np.ones(c.m), np.zeros(c.n))
    with pytest.raises(ValueError):
        lp.without_rows(np.zeros(c.m + 1, bool))


def test_the_cases_reach_the_limits_they_name():
    c = dc.case("column_lengths")
    lengths = np.diff(c.col_starts)
    assert lengths[:5].tolist() == [31, 32, 33, 600, 300]
    mask = c.steps[0][1]
    assert mask[[255, 256, 511, 512]].all() and mask[600:856].all() and not mask[856:].any()
    assert dc.move_shapes(c, 0) == (3, 1)
    c = dc.case("row_lengths")
    _, r, _, _ = dc.triplets(c, 0)
    assert (np.bincount(r, minlength=c.m) + 1)[[0, 2, 3, 4]].tolist() == [31, 32, 33, 600]
    assert dc.move_shapes(c, 0) == (1, 3)
    for name, m in (("rows_257", 257), ("rows_513", 513)):
        c = dc.case(name)
        assert c.m == m and np.flatnonzero(c.steps[0][1]).max() < dc.TILE
    c = dc.case("many_tiles")
    assert c.m > dc.TILE * dc.THREADS and c.n > dc.TILE * dc.THREADS
    assert np.diff(c.col_starts).max() <= 2
    for name, kept in (("dense_block_4", 8), ("dense_block_tail", 7)):
        c = dc.case(name)
        m, starts, _, _ = dc.reduced_csc(c)
        assert m == kept
        assert np.flatnonzero(np.diff(c.col_starts) == c.m).tolist() == [0, 1, 2]
        assert np.flatnonzero(np.diff(starts) == m).tolist()[:4] == [0, 1, 2, 3]
    c = dc.case("shapes")
    m, starts, _, _ = dc.reduced_csc(c)
    assert np.diff(starts)[0] == 0 and np.diff(c.col_starts)[0] > 0      # loses every entry
    assert np.diff(starts)[1] == np.diff(c.col_starts)[1] > 0            # loses none
    assert np.diff(c.col_starts)[2] == 0                                  # empty before
    assert 3 not in c.row_idx and c.steps[0][1][3]                        # only its slack
    c = dc.case("full_rows")
    _, r, _, _ = dc.triplets(c, 0)
    full = np.flatnonzero(np.bincount(r, minlength=c.m) == c.n)
    assert 5 in full and 6 in full and c.steps[0][1][5] and not c.steps[0][1][6]
