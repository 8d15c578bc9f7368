"""mi_lp_get_tableau_rows_sparse / mi_lp_row_combinations_sparse /
mi_lp_get_sparse_rows (include/mi_lp.h) through mi_glop.engine.LpHandle.

The expected rows are the oracle's: GetUnitRowLeftInverse(row), then
ColumnScalarProduct of every column of [A | I] with it (tests/device_ref.py),
filtered in numpy by the column mode (the non-basic mask from the ORACLE's
state) and |value| > tolerance, columns ascending. row_starts and columns are
compared as integers, values on 64-bit patterns. One test compares with the
engine's own dense call instead and says so. Then the structure of the rows,
the side effects (the next solve equals the oracle's) and every error of the
header's list.
"""
import ctypes

import numpy as np
import pytest

from mi_glop import abi, engine

import lp_gen
import parity_util
from device_ref import Matrix, bits, column_scalar_products

pytestmark = pytest.mark.gpu

ERROR_NULL, ERROR_INVALID_PROBLEM, ERROR_STATE, ERROR_DEVICE = 3, 4, 101, 100
BASIC = 0  # MI_LP_BASIC
MODES = ("all", "structural", "non_basic", "structural_non_basic")

_device_error = []


@pytest.fixture(autouse=True)
def _stop_after_a_device_error(monkeypatch):
    """A device error is never part of a test here (MI_LP_ERROR_DEVICE has no
    test of its own for that reason): after one, nothing more is started on
    the GPU."""
    check = engine.LpHandle._check

    def recording_check(self, rc, what):
        if rc == ERROR_DEVICE:
            _device_error.append(f"{what}: {self.last_error()}")
        return check(self, rc, what)

    monkeypatch.setattr(engine.LpHandle, "_check", recording_check)
    yield
    if _device_error:
        pytest.exit(f"device error: {_device_error[0]}", returncode=3)


def _matrix(lp):
    rows = [([], []) for _ in range(lp.m)]
    for c in range(lp.n):
        for e in range(lp.col_starts[c], lp.col_starts[c + 1]):
            rows[lp.row_idx[e]][0].append(c)
            rows[lp.row_idx[e]][1].append(lp.vals[e])
    return Matrix(lp.m, lp.n, [(np.array(c, np.int32), np.array(v, np.float64))
                               for c, v in rows])


def _both(lp, **kw):
    return parity_util.solve_both(lp, abi.default_params(**kw), lambda q: engine.LpHandle(q))


def same_bits(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {want.size} differ, first at {tuple(bad[0])}: "
                           f"engine {got[tuple(bad[0])].hex()} reference "
                           f"{want[tuple(bad[0])].hex()}")


def column_mask(mode, n, state):
    keep = np.ones(len(state), bool)
    if "structural" in mode:
        keep &= np.arange(len(state)) < n
    if "non_basic" in mode:
        keep &= np.asarray(state) != BASIC
    return keep


def filtered(dense, keep, tolerance):
    sel = keep[None, :] & (np.abs(dense) > tolerance)
    starts = np.zeros(len(dense) + 1, np.int64)
    np.cumsum(sel.sum(axis=1), out=starts[1:])
    cols = [np.nonzero(s)[0] for s in sel]
    return (starts, np.concatenate(cols).astype(np.int32),
            np.concatenate([dense[j][c] for j, c in enumerate(cols)]))


def same_rows(got, want, what):
    assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0]), (what, "row_starts")
    assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1]), (what, "cols")
    same_bits(got[2], want[2], what)


@pytest.mark.parametrize("dual", [0, 1])
def test_sparse_tableau_rows_parity(dual):
    lp = lp_gen.random_sparse_lp(60, 200, 0.08, 11)
    o, ro, g, rg = _both(lp, use_dual_simplex=dual)
    parity_util.compare(o, ro, g, rg, lp)
    mat = _matrix(lp)
    cols = np.arange(mat.N)
    left = np.stack([o.unit_row_left_inverse(r)[0] for r in range(lp.m)])
    dense = np.stack([column_scalar_products(mat, cols, y) for y in left])
    state = o.state()
    for rows in (np.arange(0, lp.m, 7), np.arange(lp.m)):
        for mode in MODES:
            keep = column_mask(mode, lp.n, state)
            assert 0 < keep.sum() and (mode == "all" or keep.sum() < mat.N)
            for t in (0.0, 1e-9):
                want = filtered(dense[rows], keep, t)
                what = f"{len(rows)} rows, {mode}, tolerance {t}"
                assert 0 < want[0][-1] < keep.sum() * len(rows), what
                got = g.tableau_rows_sparse(rows, t, mode, with_left_inverses=True)
                same_rows(got[:3], want, what)
                same_bits(got[3], left[rows], f"left inverses, {what}")
                same_rows(g.tableau_rows_sparse(rows, t, mode), want, "without left inverses")
                same_rows(g.row_combinations_sparse(left[rows], t, mode), want,
                          f"row combinations, {what}")
    same_rows(g.row_combinations_sparse(left[5], 0.0, "non_basic"),
              filtered(dense[5:6], column_mask("non_basic", lp.n, state), 0.0), "one vector")


def test_sparse_rows_scatter_to_the_engines_dense_rows():
    # The one comparison with the engine's own dense call.
    lp = lp_gen.random_sparse_lp(60, 200, 0.08, 11)
    g = engine.LpHandle(abi.default_params())
    g.load(lp)
    assert g.solve().problem_status == abi.OPTIMAL
    rows = np.arange(lp.m)
    dense = g.tableau_rows(rows)
    starts, cols, vals = g.tableau_rows_sparse(rows, 0.0, "all")
    scattered = np.zeros_like(dense)
    listed = np.zeros(dense.shape, bool)
    for j in range(len(rows)):
        c = cols[starts[j]:starts[j + 1]]
        assert np.all(np.diff(c) > 0)
        scattered[j, c] = vals[starts[j]:starts[j + 1]]
        listed[j, c] = True
    assert np.array_equal(listed, dense != 0.0)  # dropped: exactly the +-0.0 entries
    assert (~listed).any() and np.all(dense[~listed] == 0.0)
    same_bits(scattered[listed], dense[listed], "kept values")
    g.close()


def test_structure_of_sparse_tableau_rows():
    # The LP of test_tableau_rows_gpu.py::test_tableau_rows_are_b_inverse_a.
    lp = lp_gen.random_sparse_lp(20, 50, 0.2, 8)
    g = engine.LpHandle(abi.default_params())
    g.load(lp)
    assert g.solve().problem_status == abi.OPTIMAL
    basis = g.basis()
    rows = np.arange(lp.m)
    for mode in ("non_basic", "structural_non_basic"):
        starts, cols, vals = g.tableau_rows_sparse(rows, 0.0, mode)
        assert len(cols) > 0 and not np.isin(cols, basis).any()
        if mode == "structural_non_basic":
            assert np.all(cols < lp.n)
    starts, cols, vals = g.tableau_rows_sparse(rows, 1e-9, "all")
    for r in rows:
        c, v = cols[starts[r]:starts[r + 1]], vals[starts[r]:starts[r + 1]]
        at = np.nonzero(c == basis[r])[0]
        assert len(at) == 1, (r, basis[r])
        np.testing.assert_allclose(v[at[0]], 1.0, rtol=0.0, atol=1e-9)
    g.close()


def test_side_effects_are_those_of_unit_row_left_inverse():
    lp = lp_gen.random_sparse_lp(60, 200, 0.08, 11)
    o, ro, g, rg = _both(lp, use_dual_simplex=1)
    rows = np.arange(0, lp.m, 7)
    g.tableau_rows_sparse(rows, 1e-9, "non_basic")
    g.row_combinations_sparse(np.ones((3, lp.m)), 0.0, "structural")
    for r in rows:
        o.unit_row_left_inverse(r)
    x = o.primal()
    lb, ub = np.array(lp.col_lb), np.array(lp.col_ub)
    moved = [c for c in range(lp.n) if np.isfinite(lb[c]) and x[c] > lb[c] + 1e-3][:6]
    assert moved
    for c in moved:
        ub[c] = 0.5 * (lb[c] + x[c])
    for h in (o, g):
        h.set_variable_bounds(lb, ub)
    ro2, rg2 = o.solve(), g.solve()
    assert ro2.iterations > 0
    parity_util.compare(o, ro2, g, rg2, lp)


@pytest.fixture()
def solved():
    lp = lp_gen.random_sparse_lp(20, 50, 0.2, 8)
    g = engine.LpHandle(abi.default_params())
    g.load(lp)
    g.solve()
    yield g, lp
    g.close()


_vp = ctypes.c_void_p


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


def _raw_rows(g, rows, k, tolerance, filt, starts, left=None):
    return g._L.mi_lp_get_tableau_rows_sparse(g.h, _ptr(rows), k, ctypes.c_double(tolerance), filt,
                                              _ptr(starts), _ptr(left))


def _raw_comb(g, y, k, tolerance, filt, starts):
    return g._L.mi_lp_row_combinations_sparse(g.h, _ptr(y), k, ctypes.c_double(tolerance), filt,
                                              _ptr(starts))


def _raw_get(g, cols, vals):
    return g._L.mi_lp_get_sparse_rows(g.h, _ptr(cols), _ptr(vals))


def test_error_null(solved):
    g, lp = solved
    L = g._L
    y, rows, starts = np.zeros(lp.m), np.zeros(1, np.int32), np.zeros(2, np.int64)
    assert L.mi_lp_row_combinations_sparse(None, _ptr(y), 1, ctypes.c_double(0.0), 0,
                                           _ptr(starts)) == ERROR_NULL
    assert _raw_comb(g, None, 1, 0.0, 0, starts) == ERROR_NULL
    assert _raw_comb(g, y, 1, 0.0, 0, None) == ERROR_NULL
    assert L.mi_lp_get_tableau_rows_sparse(None, _ptr(rows), 1, ctypes.c_double(0.0), 0,
                                           _ptr(starts), None) == ERROR_NULL
    assert _raw_rows(g, None, 1, 0.0, 0, starts) == ERROR_NULL
    assert _raw_rows(g, rows, 1, 0.0, 0, None) == ERROR_NULL
    assert _raw_rows(g, rows, 1, 0.0, 0, starts, None) == 0  # left_inverses may be NULL
    cols, vals = np.zeros(lp.n + lp.m, np.int32), np.zeros(lp.n + lp.m)
    assert L.mi_lp_get_sparse_rows(None, _ptr(cols), _ptr(vals)) == ERROR_NULL
    assert _raw_get(g, None, vals) == ERROR_NULL
    assert _raw_get(g, cols, None) == ERROR_NULL
    assert _raw_get(g, cols, vals) == 0


def test_error_state():
    lp = lp_gen.random_sparse_lp(20, 50, 0.2, 8)
    g = engine.LpHandle(abi.default_params())
    g.load(lp)
    y, rows, starts = np.zeros(lp.m), np.zeros(1, np.int32), np.full(2, -7, np.int64)
    cols, vals = np.full(lp.n + lp.m, -7, np.int32), np.full(lp.n + lp.m, -3.5)
    # Before a solve; and no sparse call has stored anything yet.
    assert _raw_rows(g, rows, 1, 0.0, 0, starts) == ERROR_STATE
    assert _raw_comb(g, y, 1, 0.0, 0, starts) == ERROR_STATE
    assert _raw_get(g, cols, vals) == ERROR_STATE
    g.solve()
    assert _raw_get(g, cols, vals) == ERROR_STATE
    assert np.all(starts == -7) and np.all(cols == -7) and np.all(vals == -3.5)
    s, c, v = g.tableau_rows_sparse([0], 0.0, "all")
    assert len(c) > 0 and _raw_get(g, cols, vals) == 0
    assert np.array_equal(cols[:len(c)], c)
    # A reload forgets the stored rows.
    g.load(lp)
    assert _raw_get(g, cols, vals) == ERROR_STATE
    g.solve()
    assert _raw_get(g, cols, vals) == ERROR_STATE
    g.close()


def test_error_invalid_writes_nothing_and_keeps_the_stored_rows(solved):
    g, lp = solved
    N = lp.n + lp.m
    stored = g.tableau_rows_sparse([1, 4], 1e-9, "non_basic")
    kept = len(stored[1])
    assert kept > 0
    y = np.ones((3, lp.m))
    bad_calls = []
    for rows in ([0, lp.m], [-1, 0], [1, 2, lp.m + 5]):  # a row out of range
        r = np.array(rows, np.int32)
        bad_calls.append(lambda s, left, r=r: _raw_rows(g, r, len(r), 0.0, 0, s, left))
    for t in (-1e-300, -1.0, float("-inf"), float("nan")):  # negative and NaN tolerances
        bad_calls.append(lambda s, left, t=t: _raw_rows(g, np.zeros(3, np.int32), 3, t, 0, s, left))
        bad_calls.append(lambda s, left, t=t: _raw_comb(g, y, 3, t, 0, s))
    for filt in (4, 8, 1 | 4, 0x80000000):  # unknown filter bits
        bad_calls.append(lambda s, left, f=filt: _raw_rows(g, np.zeros(3, np.int32), 3, 0.0, f, s,
                                                           left))
        bad_calls.append(lambda s, left, f=filt: _raw_comb(g, y, 3, 0.0, f, s))
    bad_calls.append(lambda s, left: _raw_rows(g, np.zeros(3, np.int32), -1, 0.0, 0, s, left))  # k < 0
    bad_calls.append(lambda s, left: _raw_comb(g, y, -1, 0.0, 0, s))
    for call in bad_calls:
        starts = np.full(5, -7, np.int64)
        left = np.full(3 * lp.m, -3.5)
        assert call(starts, left) == ERROR_INVALID_PROBLEM
        assert np.all(starts == -7) and np.all(left == -3.5)
        # The stored result is still there, unchanged.
        cols, vals = np.full(N * 2, -7, np.int32), np.full(N * 2, -3.5)
        assert _raw_get(g, cols, vals) == 0
        assert np.array_equal(cols[:kept], stored[1]) and np.all(cols[kept:] == -7)
        same_bits(vals[:kept], stored[2], "stored values")
        assert np.all(vals[kept:] == -3.5)


def test_k_zero_is_ok_and_stores_an_empty_result(solved):
    g, lp = solved
    assert len(g.tableau_rows_sparse([1, 4], 0.0, "all")[1]) > 0
    y, rows = np.zeros(lp.m), np.zeros(1, np.int32)
    cols, vals = np.full(8, -7, np.int32), np.full(8, -3.5)
    for call in (lambda s: _raw_rows(g, rows, 0, 0.0, 0, s), lambda s: _raw_comb(g, y, 0, 0.0, 3, s)):
        starts = np.full(3, -7, np.int64)
        assert call(starts) == 0
        assert starts[0] == 0 and np.all(starts[1:] == -7)
        assert _raw_get(g, cols, vals) == 0  # the empty result: nothing is copied
        assert np.all(cols == -7) and np.all(vals == -3.5)
    for got in (g.tableau_rows_sparse([]), g.row_combinations_sparse(np.zeros((0, lp.m)))):
        assert [len(a) for a in got] == [1, 0, 0] and got[0][0] == 0
        assert (got[0].dtype, got[1].dtype, got[2].dtype) == (np.int64, np.int32, np.float64)
    s, c, v, left = g.tableau_rows_sparse([], with_left_inverses=True)
    assert left.shape == (0, lp.m)


def test_infinite_tolerance_gives_empty_rows(solved):
    g, lp = solved
    s, c, v = g.tableau_rows_sparse(np.arange(lp.m), float("inf"), "all")
    assert np.all(s == 0) and len(s) == lp.m + 1 and len(c) == 0 and len(v) == 0
