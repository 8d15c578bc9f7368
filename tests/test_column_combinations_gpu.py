"""mi_lp_column_combinations / mi_lp_column_combinations_from (include/mi_lp.h)
through mi_glop.engine.LpHandle, on solved LPs of tests/lp_gen.py.

Both calls equal, bit for bit, RefState.row_sums (tests/device_ref.py) over
the loaded matrix; the (k, n) and 1-D input forms work; a round trip with the
tableau rows ties the two halves together without the reference; every error
of the header's table is returned and leaves `out` alone; and a handle that
made the calls solves on exactly as one that never did.
"""
import ctypes

import numpy as np
import pytest

from mi_glop import abi, engine

import lp_gen
from device_ref import Matrix, RefState, bits

pytestmark = pytest.mark.gpu

ERROR_NULL, ERROR_INVALID_PROBLEM, ERROR_STATE, ERROR_DEVICE = 3, 4, 101, 100
U = 2.0 ** -53

_device_error = []


@pytest.fixture(autouse=True)
def _stop_after_a_device_error(monkeypatch):
    """A device error is never part of a test here: after one, nothing more
    is started on the GPU."""
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


def same_bits(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {want.size} differ, first at {tuple(bad[0])}: "
                           f"engine {got[tuple(bad[0])].hex()} reference "
                           f"{want[tuple(bad[0])].hex()}")


def _solved(m=60, n=200, density=0.08, seed=11, **kw):
    lp = lp_gen.random_sparse_lp(m, n, density, seed)
    g = engine.LpHandle(abi.default_params(**kw))
    g.load(lp)
    assert g.solve().problem_status == abi.OPTIMAL
    return g, lp


@pytest.fixture(scope="module")
def solved():
    g, lp = _solved()
    yield g, lp, _matrix(lp)
    g.close()


def _points(lp, g, k, seed):
    """Roundings and neighbours of x*: the primal with its slacks set to minus
    the activities, columns rounded, zeroed or moved."""
    rng = np.random.default_rng(seed)
    star = np.concatenate([g.primal(), -g.activities()])
    x = np.tile(star, (k, 1))
    for j in range(k):
        cols = rng.permutation(lp.n + lp.m)[:1 + 3 * j]
        x[j, cols] = np.round(x[j, cols] + rng.normal(size=len(cols)))
    x[k - 1, :: 3] = 0.0
    return x


@pytest.mark.parametrize("k", [1, 3, 17])
def test_dense_call_against_the_reference(solved, k):
    g, lp, mat = solved
    ref = RefState(mat)
    x = _points(lp, g, k, 70 + k)
    want = np.stack([ref.row_sums(p, None, 1.0) for p in x])
    got = g.column_combinations(x)
    assert got.shape == (k, lp.m)
    same_bits(got, want, f"k={k}")
    # Structural columns only: the slacks are zero.
    xs = x[:, :lp.n]
    padded = np.concatenate([xs, np.zeros((k, lp.m))], axis=1)
    want_s = np.stack([ref.row_sums(p, None, 1.0) for p in padded])
    same_bits(g.column_combinations(xs), want_s, f"k={k}, (k, n) input")
    same_bits(g.column_combinations(x[0]), want[:1], "1-D input, n+m")
    same_bits(g.column_combinations(xs[0]), want_s[:1], "1-D input, n")
    with pytest.raises(ValueError):
        g.column_combinations(np.zeros((2, lp.n + 1)))


def test_override_call_against_the_reference(solved):
    g, lp, mat = solved
    N = lp.n + lp.m
    ref = RefState(mat)
    rng = np.random.default_rng(81)
    base = np.concatenate([g.primal(), -g.activities()])
    overrides = []
    for j in range(18):
        cols = rng.permutation(N)[:j % 5].astype(np.int32)
        overrides.append((cols, np.round(rng.normal(size=len(cols)) * 4.0)))
    overrides[3] = (np.array([N - 1, 0], np.int32), np.array([0.0, -0.0]))
    x = np.tile(base, (len(overrides), 1))
    for j, (cols, vals) in enumerate(overrides):
        x[j, cols] = vals
    want = np.stack([ref.row_sums(p, None, 1.0) for p in x])
    got = g.column_combinations_from(base, overrides)
    same_bits(got, want, "overrides")
    same_bits(got, g.column_combinations(x), "overrides against the dense call")
    # base with n values: zero slacks.
    short = [(c[c < lp.n], v[c < lp.n]) for c, v in overrides]
    xs = np.tile(np.concatenate([base[:lp.n], np.zeros(lp.m)]), (len(short), 1))
    for j, (cols, vals) in enumerate(short):
        xs[j, cols] = vals
    same_bits(g.column_combinations_from(base[:lp.n], short),
              np.stack([ref.row_sums(p, None, 1.0) for p in xs]), "base of n values")
    assert g.column_combinations_from(base, []).shape == (0, lp.m)


def test_round_trip_with_the_tableau_rows(solved):
    """y (A x) and (y A) x over [A | I] are one bilinear form. Each number is a
    sum of the products y_r a_rc x_c, and every such product passes through at
    most K = (n + m) + m + 2 roundings on either path (two multiplications,
    the adds of one row or column sum, the adds of the numpy dot), so either
    side is within gamma_K sum |y_r a_rc x_c| of the exact value, with
    gamma_K = K u / (1 - K u) as in tests/exact_bound.py, and the two differ
    by at most twice that."""
    g, lp, mat = solved
    N = lp.n + lp.m
    rows = np.arange(0, lp.m, 5)
    t, y = g.tableau_rows(rows, with_left_inverses=True)
    same_bits(g.row_combinations(y), t, "row combinations of the left inverses")
    x = _points(lp, g, 6, 91)
    ax = g.column_combinations(x)  # (6, m)
    a = np.zeros((lp.m, N))
    for r in range(lp.m):
        a[r, mat.t_cols[r]] = mat.t_vals[r]
    K = N + lp.m + 2
    gamma = K * U / (1.0 - K * U)
    for i in range(len(rows)):
        for j in range(len(x)):
            left = np.dot(y[i], ax[j])
            right = np.dot(t[i], x[j])
            mag = np.dot(np.abs(y[i]), np.abs(a) @ np.abs(x[j]))
            assert abs(left - right) <= 2.0 * gamma * mag * (1.0 + 1e-6), (i, j, left, right, mag)
    assert np.abs(ax).max() > 0.0 and np.abs(t).max() > 0.0


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _dense(g, h, x, k, out):
    return g._L.mi_lp_column_combinations(h, _vp(x), k, _vp(out))


def _from(g, h, base, k, starts, cols, vals, out):
    return g._L.mi_lp_column_combinations_from(h, _vp(base), k, _vp(starts), _vp(cols),
                                               _vp(vals), _vp(out))


def test_error_null(solved):
    g, lp, _ = solved
    N = lp.n + lp.m
    x, out = np.zeros(N), np.full(lp.m, -3.5)
    starts = np.array([0, 1], np.int64)
    cols, vals = np.zeros(1, np.int32), np.ones(1)
    assert _dense(g, None, x, 1, out) == ERROR_NULL
    assert _dense(g, g.h, None, 1, out) == ERROR_NULL
    assert _dense(g, g.h, x, 1, None) == ERROR_NULL
    assert _from(g, None, x, 1, starts, cols, vals, out) == ERROR_NULL
    assert _from(g, g.h, None, 1, starts, cols, vals, out) == ERROR_NULL
    assert _from(g, g.h, x, 1, None, cols, vals, out) == ERROR_NULL
    assert _from(g, g.h, x, 1, starts, cols, vals, None) == ERROR_NULL
    assert _from(g, g.h, x, 1, starts, None, vals, out) == ERROR_NULL
    assert _from(g, g.h, x, 1, starts, cols, None, out) == ERROR_NULL
    assert np.all(out == -3.5)
    # cols and vals may be NULL when there is no override.
    assert _from(g, g.h, x, 1, np.zeros(2, np.int64), None, None, out) == 0
    assert np.all(bits(out) == 0)


def test_error_state():
    lp = lp_gen.random_sparse_lp(20, 50, 0.2, 8)
    g = engine.LpHandle(abi.default_params())
    g.load(lp)
    x, out = np.zeros(lp.n + lp.m), np.full(lp.m, -3.5)
    assert _dense(g, g.h, x, 1, out) == ERROR_STATE
    assert _from(g, g.h, x, 1, np.zeros(2, np.int64), None, None, out) == ERROR_STATE
    assert np.all(out == -3.5)
    g.close()


def test_error_invalid_writes_nothing(solved):
    g, lp, _ = solved
    N = lp.n + lp.m
    x = np.ones(2 * N)
    out = np.full(2 * lp.m, -3.5)
    i64, i32 = lambda a: np.array(a, np.int64), lambda a: np.array(a, np.int32)
    assert _dense(g, g.h, x, -1, out) == ERROR_INVALID_PROBLEM
    vals = np.ones(4)
    bad = [
        (-1, i64([0, 0, 0]), i32([0, 0, 0, 0])),        # k < 0
        (2, i64([0, 2, 4]), i32([0, 1, 5, 5])),         # the same column twice in a point
        (2, i64([0, 2, 4]), i32([0, N, 1, 2])),         # a column out of range
        (2, i64([0, 2, 4]), i32([0, 1, -1, 2])),
        (2, i64([0, 3, 2]), i32([0, 1, 2, 3])),         # decreasing starts
        (2, i64([1, 2, 4]), i32([0, 1, 2, 3])),         # starts[0] != 0
    ]
    for k, starts, cols in bad:
        assert _from(g, g.h, x, k, starts, cols, vals, out) == ERROR_INVALID_PROBLEM, (k, starts)
        assert np.all(out == -3.5)
    # The same column in two different points is fine.
    assert _from(g, g.h, x, 2, i64([0, 2, 4]), i32([0, 5, 5, 0]), vals, out) == 0
    assert not np.any(out == -3.5)


def test_k_zero_is_ok_and_empty(solved):
    g, lp, _ = solved
    N = lp.n + lp.m
    x, out = np.zeros(N), np.full(lp.m, -3.5)
    assert _dense(g, g.h, x, 0, out) == 0
    assert _from(g, g.h, x, 0, np.zeros(1, np.int64), None, None, out) == 0
    assert np.all(out == -3.5)
    assert g.column_combinations(np.zeros((0, N))).shape == (0, lp.m)
    assert g.column_combinations_from(x, []).shape == (0, lp.m)


@pytest.mark.parametrize("dual", [0, 1])
def test_a_later_solve_does_not_see_the_calls(dual):
    """Two handles solve the same LP; one scores points in between; then both
    get the same tighter bounds and solve on from their bases."""
    g, lp = _solved(use_dual_simplex=dual)
    q, _ = _solved(use_dual_simplex=dual)
    try:
        x = _points(lp, g, 17, 95)
        g.column_combinations(x)
        g.column_combinations_from(x[0], [(np.array([0, 3], np.int32), np.array([1.0, 0.0]))] * 5)
        star = q.primal()
        lb, ub = np.array(lp.col_lb), np.array(lp.col_ub)
        moved = [c for c in range(lp.n) if np.isfinite(lb[c]) and star[c] > lb[c] + 1e-3][:6]
        assert moved
        for c in moved:
            ub[c] = 0.5 * (lb[c] + star[c])
        results = []
        for h in (g, q):
            h.set_variable_bounds(lb, ub)
            results.append(h.solve())
        rg, rq = results
        assert rq.iterations > 0
        assert (rg.problem_status, rg.iterations) == (rq.problem_status, rq.iterations)
        assert np.array_equal(g.basis(), q.basis())
        assert np.array_equal(g.state(), q.state())
        same_bits(g.primal(), q.primal(), "primal values")
        same_bits(g.duals(), q.duals(), "dual values")
        assert bits(np.float64(rg.objective)) == bits(np.float64(rq.objective))
    finally:
        g.close()
        q.close()
