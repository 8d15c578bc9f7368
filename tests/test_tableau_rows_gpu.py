"""mi_lp_get_tableau_rows / mi_lp_row_combinations (include/mi_lp.h) through
mi_glop.engine.LpHandle.

A tableau row is pinned by two pieces of Glop's public surface: the oracle's
GetUnitRowLeftInverse(row), then ColumnScalarProduct of every column of
[A | I] with it (tests/device_ref.py). The engine's k rows of one call equal
that bit for bit; an independent check compares them with numpy's
B^-1 [A | I]; the call has the side effects of k unit_row_left_inverse calls
and no others (the next solve equals the oracle's); every error of the
header's table is returned.
"""
import ctypes

import numpy as np
import pytest

from mi_glop import abi, engine

import lp_gen
import oracle_lib
import parity_util
from device_ref import Matrix, bits, column_scalar_products

pytestmark = pytest.mark.gpu

ERROR_NULL, ERROR_INVALID_PROBLEM, ERROR_STATE, ERROR_DEVICE = 3, 4, 101, 100

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


@pytest.mark.parametrize("dual", [0, 1])
def test_tableau_rows_parity(dual):
    lp = lp_gen.random_sparse_lp(60, 200, 0.08, 11)
    o, ro, g, rg = _both(lp, use_dual_simplex=dual)
    parity_util.compare(o, ro, g, rg, lp)
    mat = _matrix(lp)
    cols = np.arange(mat.N)
    left = np.stack([o.unit_row_left_inverse(r)[0] for r in range(lp.m)])
    want = np.stack([column_scalar_products(mat, cols, y) for y in left])
    for rows in (np.arange(0, lp.m, 7), np.arange(lp.m)):
        got, got_left = g.tableau_rows(rows, True)
        same_bits(got_left, left[rows], f"left inverses of {len(rows)} rows")
        same_bits(got, want[rows], f"{len(rows)} tableau rows")
        same_bits(g.tableau_rows(rows), want[rows], "without left inverses")
        same_bits(g.row_combinations(left[rows]), want[rows], "row combinations")
    same_bits(g.row_combinations(left[5]), want[5:6], "one vector")


def test_tableau_rows_are_b_inverse_a():
    # The LP and the tolerance of test_boundary.py::test_dictionary_is_b_inverse_a.
    lp = lp_gen.random_sparse_lp(20, 50, 0.2, 8)
    g = engine.LpHandle(abi.default_params())
    g.load(lp)
    assert g.solve().problem_status == abi.OPTIMAL
    a = np.zeros((lp.m, lp.n + lp.m))
    for j in range(lp.n):
        for e in range(lp.col_starts[j], lp.col_starts[j + 1]):
            a[lp.row_idx[e], j] = lp.vals[e]
    a[:, lp.n:] = np.eye(lp.m)
    b = a[:, g.basis()]
    np.testing.assert_allclose(g.tableau_rows(np.arange(lp.m)), np.linalg.solve(b, a), atol=1e-9)


def test_side_effects_are_those_of_unit_row_left_inverse():
    lp = lp_gen.random_sparse_lp(60, 200, 0.08, 11)
    o, ro, g, rg = _both(lp, use_dual_simplex=1)
    rows = np.arange(0, lp.m, 7)
    g.tableau_rows(rows)
    g.row_combinations(np.ones((3, lp.m)))
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


@pytest.fixture(scope="module")
def solved():
    lp = lp_gen.random_sparse_lp(20, 50, 0.2, 8)
    g = engine.LpHandle(abi.default_params())
    g.load(lp)
    g.solve()
    yield g, lp
    g.close()


def _raw(g, rows, out, left=None):
    rows = np.ascontiguousarray(rows, np.int32)
    return g._L.mi_lp_get_tableau_rows(g.h, rows.ctypes.data_as(ctypes.c_void_p), len(rows),
                                       out.ctypes.data_as(ctypes.c_void_p), left)


def test_error_null(solved):
    g, lp = solved
    N = lp.n + lp.m
    L, vp = g._L, ctypes.c_void_p
    out, y, rows = np.zeros(N), np.zeros(lp.m), np.zeros(1, np.int32)
    assert L.mi_lp_row_combinations(None, y.ctypes.data_as(vp), 1, out.ctypes.data_as(vp)) == ERROR_NULL
    assert L.mi_lp_row_combinations(g.h, None, 1, out.ctypes.data_as(vp)) == ERROR_NULL
    assert L.mi_lp_row_combinations(g.h, y.ctypes.data_as(vp), 1, None) == ERROR_NULL
    assert L.mi_lp_get_tableau_rows(None, rows.ctypes.data_as(vp), 1, out.ctypes.data_as(vp),
                                    None) == ERROR_NULL
    assert L.mi_lp_get_tableau_rows(g.h, None, 1, out.ctypes.data_as(vp), None) == ERROR_NULL
    assert L.mi_lp_get_tableau_rows(g.h, rows.ctypes.data_as(vp), 1, None, None) == ERROR_NULL
    assert _raw(g, rows, out, None) == 0  # left_inverses may be NULL


def test_error_state():
    lp = lp_gen.random_sparse_lp(20, 50, 0.2, 8)
    g = engine.LpHandle(abi.default_params())
    g.load(lp)
    vp = ctypes.c_void_p
    out, y = np.zeros(lp.n + lp.m), np.zeros(lp.m)
    assert _raw(g, [0], out) == ERROR_STATE
    assert g._L.mi_lp_row_combinations(g.h, y.ctypes.data_as(vp), 1,
                                       out.ctypes.data_as(vp)) == ERROR_STATE
    g.close()


def test_error_invalid_writes_nothing(solved):
    g, lp = solved
    N, vp = lp.n + lp.m, ctypes.c_void_p
    for rows in ([0, lp.m], [-1, 0], [1, 2, lp.m + 5]):
        out = np.full(len(rows) * N, -3.5)
        left = np.full(len(rows) * lp.m, -3.5)
        assert _raw(g, rows, out, left.ctypes.data_as(vp)) == ERROR_INVALID_PROBLEM
        assert np.all(out == -3.5) and np.all(left == -3.5)
    out, y = np.full(N, -3.5), np.zeros(lp.m)
    assert g._L.mi_lp_get_tableau_rows(g.h, np.zeros(1, np.int32).ctypes.data_as(vp), -1,
                                       out.ctypes.data_as(vp), None) == ERROR_INVALID_PROBLEM
    assert g._L.mi_lp_row_combinations(g.h, y.ctypes.data_as(vp), -1,
                                       out.ctypes.data_as(vp)) == ERROR_INVALID_PROBLEM
    assert np.all(out == -3.5)


def test_k_zero_is_ok_and_empty(solved):
    g, lp = solved
    N, vp = lp.n + lp.m, ctypes.c_void_p
    out, y = np.full(N, -3.5), np.zeros(lp.m)
    assert g._L.mi_lp_get_tableau_rows(g.h, np.zeros(1, np.int32).ctypes.data_as(vp), 0,
                                       out.ctypes.data_as(vp), None) == 0
    assert g._L.mi_lp_row_combinations(g.h, y.ctypes.data_as(vp), 0, out.ctypes.data_as(vp)) == 0
    assert np.all(out == -3.5)
    assert g.tableau_rows([]).shape == (0, N)
    assert g.row_combinations(np.zeros((0, lp.m))).shape == (0, N)
