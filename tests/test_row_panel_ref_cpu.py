"""The reference of tests/test_row_panel_ops_gpu.py (RefState.row_sums of
tests/device_ref.py, one point at a time) and its inputs
(tests/row_panel_cases.py), judged without the engine and without a GPU.

- Every reference value lies within the k-term dot-product bound of the exact
  sum of its exact live products (tests/exact_bound.py).
- Materialising an override set in numpy and summing the dense points is the
  definition the other tests use; here it is checked against the header's
  words, entry by entry.
- The inputs tell summation orders apart, against the reversed order and
  against a balanced tree (row_panel_cases.orders_not_told_apart).
- The special points do what they are there for.
"""
import numpy as np
import pytest

import row_panel_cases as rc
import solveops_cases as sc
from device_ref import bits
from exact_bound import within_gamma


def _live_terms(mat, r, x):
    return [(x[c], a) for c, a in zip(mat.t_cols[r].tolist(), mat.t_vals[r].tolist())
            if x[c] != 0.0]


def _check_bound(mat, x, out, what):
    xl = np.asarray(x, np.float64).tolist()
    for r in range(mat.m):
        t = _live_terms(mat, r, xl)
        if not all(np.isfinite(m) for m, _ in t):
            continue
        assert (len(t) == 0 and bits(out[r]) == 0) or within_gamma(float(out[r]), t), (what, r)


@pytest.mark.parametrize("name", rc.CASES)
def test_reference_within_the_dot_product_bound(name):
    mat, pts, ref = rc.matrix(name), rc.points(name), rc.reference(name)
    assert ref.shape == (rc.POOL, mat.m)
    # wide's rows hold more than a thousand entries each: a sample of its points.
    for j in (range(rc.POOL) if name != "wide" else (0, rc.WITH_NAN, 16, 32)):
        _check_bound(mat, pts[j], ref[j], f"{name} point {j}")


@pytest.mark.parametrize("name", rc.CASES)
def test_special_points(name):
    mat, pts, ref = rc.matrix(name), rc.points(name), rc.reference(name)
    assert np.all(bits(pts[rc.ALL_POS_ZERO]) == 0)
    assert np.all(bits(pts[rc.ALL_NEG_ZERO]) == bits(-0.0))
    for j in (rc.ALL_POS_ZERO, rc.ALL_NEG_ZERO):
        assert np.all(bits(ref[j]) == 0), (name, j)  # +0.0 everywhere
    for j, test in ((rc.WITH_NAN, np.isnan), (rc.WITH_INF, np.isinf)):
        col = np.nonzero(test(pts[j]))[0]
        assert len(col) == 1
        holds = np.array([col[0] in c for c in mat.t_cols])
        # It reaches every row that holds its column, and no other.
        assert holds.sum() >= 2 and np.array_equal(test(ref[j]), holds), (name, j)
    pool = pts[rc.ordinary(name)]
    zero = pool == 0.0
    assert np.isfinite(pool).all()
    assert 0.05 < np.mean(zero & ~np.signbit(pool)) < 0.15, name
    assert 0.005 < np.mean(zero & np.signbit(pool)) < 0.04, name
    assert set(rc.ALONE).isdisjoint(rc.SPECIAL + (rc.ZERO_ROW,))
    if name == "rows70":
        r = sc.ROWS70_ZERO_ROW
        x = pts[rc.ZERO_ROW]
        assert np.all(bits(x[mat.t_cols[r]]) == bits(np.array([0.0, -0.0])))
        assert bits(ref[rc.ZERO_ROW][r]) == 0
        # The point is no zero point: the longer rows all have live terms.
        assert np.all(ref[rc.ZERO_ROW][mat.row_len >= 3] != 0.0)


def test_case_shapes():
    mat = rc.matrix("rows70")
    assert mat.m == 70 and set(mat.row_len) == {1, 2, 3, 63, 64, 65, 128, 129, 130, 200}
    assert mat.m % 16 == 6 and mat.m % 64 == 6  # the last workgroup at widths 16 and 4
    assert rc.matrix("wide").N >= 33000 and rc.matrix("wide").m == 40
    assert rc.environment("dense64") == {"MILP_DENSE_BLOCK": "force"}
    steps = rc.matrix("steps")
    g = rc.GATHER
    assert {g - 1, g, g + 1, 2 * g - 1, 2 * g, 2 * g + 1} <= set(steps.row_len)
    assert steps.m > 2 * 16 and steps.m % 16 != 0
    assert [rc.width(c) for _, c in rc.panels(33)] == [16, 16, 1]
    assert [rc.width(c) for _, c in rc.panels(17)] == [16, 1]
    assert {rc.width(c) for k in rc.KS for _, c in rc.panels(k)} == {1, 4, 16}


@pytest.mark.parametrize("name", rc.CASES)
def test_points_tell_orders_apart(name):
    assert rc.orders_not_told_apart(name) == []
    mat = rc.matrix(name)
    assert (mat.row_len >= 63).any() or name == "steps"
    assert (mat.row_len >= 3).any()


@pytest.mark.parametrize("which", rc.OVERRIDE_SETS)
@pytest.mark.parametrize("name", rc.CASES)
def test_override_sets_are_what_the_header_says(name, which):
    """Point j is base with x[cols[i]] = vals[i] for i in [starts[j],
    starts[j + 1]): every position of every materialised point, on bits."""
    mat = rc.matrix(name)
    base, sets = rc.override_set(name, which)
    starts, cols, vals = rc.flatten(sets)
    x = rc.materialise(base, sets)
    assert starts[0] == 0 and len(starts) == len(sets) + 1 and np.all(np.diff(starts) >= 0)
    assert cols.dtype == np.int32 and vals.dtype == np.float64 and starts.dtype == np.int64
    assert len(cols) == len(vals) == starts[-1]
    for j in range(len(sets)):
        want = {int(c): v for c, v in zip(cols[starts[j]:starts[j + 1]],
                                          vals[starts[j]:starts[j + 1]])}
        assert len(want) == starts[j + 1] - starts[j]  # no column twice
        assert all(0 <= c < mat.N for c in want)
        for c in range(mat.N):
            assert bits(x[j, c]) == bits(want.get(c, base[c])), (name, which, j, c)
    assert rc.override_bytes(name, which) == 8 * mat.N + 12 * len(cols) + 8 * len(starts)
    ref = rc.override_reference(name, which)
    for j in range(len(sets)):
        _check_bound(mat, x[j], ref[j], f"{name} {which} point {j}")


@pytest.mark.parametrize("name", rc.CASES)
def test_override_sets_cover_their_cases(name):
    mat = rc.matrix(name)
    base, mixed = rc.override_set(name, "mixed")
    ref = rc.override_reference(name, "mixed")
    assert len(mixed) == 5 and len(mixed[0][0]) == 0
    assert sorted(mixed[1][0].tolist()) == [0, mat.N - 1]
    assert bits(mixed[2][1]).tolist() == bits(np.array([0.0, -0.0, np.nan, np.inf])).tolist()
    assert len(mixed[3][0]) >= rc.MANY
    assert np.any(np.diff(mixed[3][0]) < 0)  # unsorted
    # The overrides matter: to zero skips an entry that the base has live, and
    # the NaN and the inf arrive.
    zc = mixed[2][0][:2]
    assert np.all(base[zc] != 0.0)
    plain = rc.RefState(mat).row_sums(base, None, 1.0)
    assert np.array_equal(bits(ref[0]), bits(plain))
    for j in (1, 2, 3, 4):
        assert np.any(bits(ref[j]) != bits(plain)), (name, j)
    assert np.isnan(ref[2]).any() and np.isinf(ref[2]).any()
    _, k17 = rc.override_set(name, "k17")
    assert len(k17) == 17 and len(k17[16][0]) > 0 and all(len(c) > 0 for c, _ in k17)
    assert [len(s) for s in (rc.override_set(name, "one")[1],
                             rc.override_set(name, "four")[1])] == [1, 4]
