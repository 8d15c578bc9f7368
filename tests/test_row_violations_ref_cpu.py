"""The inputs and the reference of tests/test_row_violations_ops_gpu.py
(tests/row_violation_cases.py), judged without the engine and without a GPU:
these are conditions on the inputs, met by the reference alone.

- filter_reference follows the header's rule entry by entry (a plain Python
  restatement on a sample), every amount of a kept non-NaN activity is > 0 and
  no NaN, and the summaries are what the lists imply.
- `tall` has the geometry it is there for and its vectorised reference equals
  RefState.row_sums on a sample of rows.
- split keeps and drops entries of every point that is not all-zero; edges
  holds the four edge kinds in every panel width; NaN and +-inf activities are
  present; some point has no violated row; some panel has two rows tied for
  the worst amount.
"""
import math

import numpy as np
import pytest

import row_panel_cases as rc
import row_violation_cases as vc
from device_ref import Matrix, RefState, bits


def _plain_rule(a, lo, hi, tol):
    """The header's words for one (row, point): (violated, amount)."""
    if not (a >= lo - tol) or not (a <= hi + tol):
        return True, (math.inf if a != a else max(lo - a, a - hi))
    return False, None


@pytest.mark.parametrize("which", vc.BOUND_SETS)
@pytest.mark.parametrize("name", vc.CASES)
def test_filter_reference_is_the_rule(name, which):
    acts = vc.reference(name)
    lb, ub, tol = vc.bounds(name, which)
    k = vc.pool(name)
    starts, rows, vals, summaries = vc.expected(name, which, k)
    assert starts[0] == 0 and starts[k] == len(rows) == len(vals)
    assert rows.dtype == np.int32 and starts.dtype == np.int64
    m = acts.shape[1]
    sample = range(m) if m <= 100 else list(range(0, m, 997)) + [m - 1]
    for j in range(k):
        mine = rows[starts[j]:starts[j + 1]]
        assert np.all(np.diff(mine) > 0)
        assert np.array_equal(bits(vals[starts[j]:starts[j + 1]]), bits(acts[j, mine]))
        kept = set(mine.tolist())
        worst, worst_row = 0.0, -1
        for r in sample:
            is_violated, amount = _plain_rule(float(acts[j, r]), float(lb[r]), float(ub[r]), tol)
            assert is_violated == (r in kept), (name, which, j, r)
            if is_violated:
                assert amount > 0.0 and amount == amount
        # The summaries from the lists alone, over every kept row.
        _, _, amount = vc.amounts(acts[j, mine], lb[mine], ub[mine])
        assert not np.isnan(amount).any() and np.all(amount > 0.0)
        if len(mine):
            worst = amount.max()
            worst_row = int(mine[np.nonzero(amount == worst)[0][0]])
        s = summaries[j]
        assert (s["count"], s["worst_row"], s["reserved"]) == (len(mine), worst_row, 0)
        assert bits(s["worst"]) == bits(np.float64(worst))


def test_tall_geometry_and_reference():
    mat = vc.matrix("tall")
    assert mat.m == 66000 and mat.n == 12 and vc.pool("tall") <= 5
    assert vc.satisfies_geometry(mat.m, vc.TILE_ROWS, vc.OFFSETS_STEP_TILES)
    assert set(mat.row_len) == {1, 2, 3, 4}  # 0 to 3 structural entries and the slack
    # RefState.row_sums on the matrix of a sample of the rows (a row's sum
    # depends on its own entries and its own slack only).
    rows = np.array(list(range(0, mat.m, 211)) + [mat.m - 1])
    sample = Matrix(len(rows), mat.n, [(mat.t_cols[r][:-1], mat.t_vals[r][:-1]) for r in rows])
    ref = RefState(sample)
    acts = vc.reference("tall")
    for j, x in enumerate(vc.points("tall")):
        with np.errstate(invalid="ignore"):
            want = ref.row_sums(np.concatenate([x[:mat.n], x[mat.n + rows]]), None, 1.0)
        assert np.array_equal(bits(acts[j, rows]), bits(want)), j


@pytest.mark.parametrize("name", vc.CASES)
def test_special_activities_are_present(name):
    acts = vc.reference(name)
    nan_point, inf_point = ((vc.TALL_NAN, vc.TALL_INF) if name == "tall"
                            else (rc.WITH_NAN, rc.WITH_INF))
    assert np.isnan(acts[nan_point]).sum() >= 2 and np.isinf(acts[inf_point]).sum() >= 2
    # free: exactly the NaN activities, and they tie at +inf: the lowest row.
    k = vc.pool(name)
    starts, rows, vals, summaries = vc.expected(name, "free", k)
    assert np.isnan(vals).all() and len(vals) == np.isnan(acts).sum()
    s = summaries[nan_point]
    assert s["count"] >= 2 and s["worst"] == np.inf
    assert s["worst_row"] == np.nonzero(np.isnan(acts[nan_point]))[0][0]
    # crossed: everything.
    assert vc.expected(name, "crossed", k)[0][k] == k * acts.shape[1]
    # +-inf activities follow the comparisons: violated under split.
    srows = vc.expected(name, "split", k)
    mine = srows[1][srows[0][inf_point]:srows[0][inf_point + 1]]
    assert set(np.nonzero(np.isinf(acts[inf_point]))[0]) <= set(mine.tolist())


@pytest.mark.parametrize("name", vc.CASES)
def test_split_keeps_and_drops_for_every_point(name):
    """The bounds do not depend on k, so every panel of every k holds these
    points as they are here."""
    acts = vc.reference(name)
    m = acts.shape[1]
    counts = vc.expected(name, "split", vc.pool(name))[3]["count"]
    for j in range(vc.pool(name)):
        if np.all(vc.points(name)[j] == 0.0):
            continue
        assert 0 < counts[j] < m, (name, j, counts[j])
    total = counts.sum() / (vc.pool(name) * m)
    assert 0.3 < total < 0.7, (name, total)
    for k in vc.ks(name):
        for first, count in rc.panels(k):
            assert first + count <= vc.pool(name)


@pytest.mark.parametrize("which", ("edges0", "edges_tol"))
@pytest.mark.parametrize("name", vc.CASES)
def test_edges_hold_every_kind_in_every_width(name, which):
    acts = vc.reference(name)
    lb, ub, tol = vc.bounds(name, which)
    assert tol == (0.0 if which == "edges0" else vc.EDGE_TOLERANCE) and (tol > 0) == (
        which == "edges_tol")
    entries = vc.edge_entries(name, which)
    keep = vc.violated(acts, lb, ub, tol)
    for p, r, kind in entries:
        a = acts[p, r]
        if kind == "at_lo":
            assert bits(lb[r] - tol) == bits(a) and not keep[p, r]
        elif kind == "below_lo":
            assert bits(np.nextafter(a, np.inf)) == bits(lb[r] - tol) and keep[p, r]
        elif kind == "at_hi":
            assert bits(ub[r] + tol) == bits(a) and not keep[p, r]
        else:
            assert bits(np.nextafter(a, -np.inf)) == bits(ub[r] + tol) and keep[p, r]
    widths = set()
    for k in vc.ks(name):
        for first, count in rc.panels(k):
            inside = {kind for p, _, kind in entries if first <= p < first + count}
            if inside:
                assert inside == set(vc.EDGE_KINDS), (name, k, first)
                widths.add(rc.width(count))
    assert widths == {1, 4, 16}, (name, widths)


@pytest.mark.parametrize("name", vc.CASES)
def test_a_point_without_violations_and_a_tie(name):
    k = vc.pool(name)
    zero = vc.TALL_ZERO if name == "tall" else rc.ALL_POS_ZERO
    s = vc.expected(name, "one_sided", k)[3]
    assert s["count"][zero] == 0 and s["worst_row"][zero] == -1 and bits(s["worst"][zero]) == 0
    assert (s["count"] > 0).any()
    # Two rows with bit-equal amounts at one point: free's NaN rows tie at
    # +inf, and the summary names the lowest of them.
    acts = vc.reference(name)
    lb, ub, tol = vc.bounds(name, "free")
    nan_point = vc.TALL_NAN if name == "tall" else rc.WITH_NAN
    _, _, amount = vc.amounts(acts[nan_point], lb, ub)
    tied = np.nonzero(vc.violated(acts[nan_point], lb, ub, tol) & (amount == np.inf))[0]
    assert len(tied) >= 2
    assert vc.expected(name, "free", k)[3]["worst_row"][nan_point] == tied[0]
    # The tie is inside one panel for every k that reaches the point.
    assert any(k >= nan_point + 1 for k in vc.ks(name))
