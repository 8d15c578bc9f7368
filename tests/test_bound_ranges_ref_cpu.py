"""The reference and the inputs of the bound-set activity-range tests
(tests/bound_range_cases.py), checked without a GPU: the reference against
exact sums, that its inputs tell summation orders and a contracted
multiply-add apart, that override lists materialise to the dense pool, the
conditions on the pools and on the row-bound sets that the GPU tests rely on,
and cpsat.branch_overrides against cpsat.branch_lps.
"""
import types

import numpy as np
import pytest

import bound_range_cases as bc
import exact_bound
from device_ref import bits
from mi_glop import cpsat

SMALL = ("rows70", "steps")  # the matrices the order conditions are stated for


@pytest.mark.parametrize("name", bc.CASES)
def test_reference_against_exact_sums(name):
    """Every finite lo and hi is within the k-term bound of the exact sum of
    the terms the rule adds; the counts are the infinite bounds the rule
    reads; a row without structural entries gives (+0.0, +0.0, 0, 0)."""
    mat = bc.matrix(name)
    L, U = bc.pool(name)
    lo, hi, lo_inf, hi_inf = bc.reference(name)
    for j in range(bc.POOL):
        for r in range(mat.m):
            terms = {"lo": [], "hi": []}
            counts = {"lo": 0, "hi": 0}
            for c, a in zip(mat.t_cols[r][:-1], mat.t_vals[r][:-1]):
                assert a != 0.0 and c < mat.n
                picks = (L[j, c], U[j, c]) if a > 0.0 else (U[j, c], L[j, c])
                for side, b in zip(("lo", "hi"), picks):
                    if np.isinf(b):
                        counts[side] += 1
                    else:
                        terms[side].append((a, b))
            assert (lo_inf[j, r], hi_inf[j, r]) == (counts["lo"], counts["hi"]), (name, j, r)
            for side, value in (("lo", lo[j, r]), ("hi", hi[j, r])):
                if not terms[side]:
                    assert bits(value) == 0, (name, j, r, side)
                elif np.isfinite(value) and all(np.isfinite(b) for _, b in terms[side]):
                    assert exact_bound.within_gamma(value, terms[side]), (name, j, r, side)
    empty = mat.row_len == 1
    assert empty.any() or name != "rows70"
    for a in (lo, hi, lo_inf, hi_inf):
        assert not a[:, empty].any() and not np.signbit(a[:, empty].astype(np.float64)).any()


def test_structural_lengths():
    """What the header of bound_range_cases says of the three matrices."""
    assert bc.structural_lengths("rows70") == [0, 1, 2, 62, 63, 64, 127, 128, 129, 199]
    assert bc.structural_lengths("steps") == [0, 6, 7, 8, 14, 15, 16, 23]
    assert bc.structural_lengths("groups") == [0, 7, 8, 9, 15, 16, 17, 24]
    g = bc.GATHER
    with_slack = {x + 1 for x in bc.structural_lengths("steps")}
    assert {g - 1, g, g + 1, 2 * g - 1, 2 * g, 2 * g + 1} <= with_slack
    assert {g - 1, g, g + 1} <= set(bc.structural_lengths("groups"))
    m = bc.matrix("rows70").m
    assert all(m % rows not in (0,) for rows in (256, 64, 16))


@pytest.mark.parametrize("name", SMALL)
def test_reversed_order_changes_bits(name):
    mat = bc.matrix(name)
    L, U = bc.pool(name)
    fwd = bc.reference(name)
    rev = bc.ranges(mat, L, U, order=-1)
    assert np.array_equal(fwd[2], rev[2]) and np.array_equal(fwd[3], rev[3])
    changed = bits(fwd[0]) != bits(rev[0])
    print(name, "lo sums that change bits when summed in reverse:", int(changed.sum()),
          "of", changed.size)
    for j in bc.ordinary(name):
        assert changed[j].any() and (bits(fwd[1][j]) != bits(rev[1][j])).any(), (name, j)
    # Also within every panel of every k, so that no panel passes by chance.
    for k in bc.KS:
        for first, count in bc.rc.panels(k):
            assert changed[first:first + count].any(), (name, k, first)


@pytest.mark.parametrize("name", SMALL)
def test_contracted_multiply_add_changes_bits(name):
    mat = bc.matrix(name)
    L, U = bc.pool(name)
    pick = bc.ordinary(name)
    fwd = bc.reference(name)
    fma = bc.ranges(mat, L[pick], U[pick], product=bc.fused)
    for i, j in enumerate(pick):
        assert (bits(fwd[0][j]) != bits(fma[0][i])).any(), (name, j, "lo")
        assert (bits(fwd[1][j]) != bits(fma[1][i])).any(), (name, j, "hi")


@pytest.mark.parametrize("name", bc.CASES)
def test_pool_conditions(name):
    mat = bc.matrix(name)
    L, U = bc.pool(name)
    lo, hi, lo_inf, hi_inf = bc.reference(name)
    assert L.shape == U.shape == (bc.POOL, mat.n)
    for j in bc.ordinary(name):
        assert not np.isnan(L[j]).any() and not (L[j] > U[j]).any()
        assert int(np.isinf(L[j]).sum() + np.isinf(U[j]).sum()) == j % 4
    both = np.concatenate([L[bc.ordinary(name)].ravel(), U[bc.ordinary(name)].ravel()])
    assert ((both == 0.0) & np.signbit(both)).any() and ((both == 0.0) & ~np.signbit(both)).any()
    for j in bc.ALONE:
        assert j in bc.ordinary(name) and np.isfinite(L[j]).all() and np.isfinite(U[j]).all()
    assert set(np.unique(lo_inf)) >= {0, 1, 2, 3} and set(np.unique(hi_inf)) >= {0, 1, 2, 3}
    finite = np.mean((lo_inf == 0) & (hi_inf == 0))
    print(name, "pairs with both ranges finite:", finite)
    assert 0.5 <= finite <= 0.9
    # The special children.
    assert np.array_equal(bits(L[bc.BOX]), bits(U[bc.BOX])) and np.isfinite(L[bc.BOX]).all()
    assert not lo_inf[bc.BOX].any() and not hi_inf[bc.BOX].any()
    held = bc.most_held(mat)[0]
    rows = [r for r in range(mat.m) if held in mat.t_cols[r][:-1]]
    assert len(rows) >= 2
    assert np.isnan(L[bc.WITH_NAN, held])
    for r in rows:  # the NaN is in lo or in hi, by the entry's sign; never counted
        assert np.isnan(lo[bc.WITH_NAN, r]) != np.isnan(hi[bc.WITH_NAN, r])
    assert L[bc.WRONG_INF, held] == np.inf
    for r in rows:  # counted on the side that reads it, and no +inf in either sum
        a = mat.t_vals[r][list(mat.t_cols[r]).index(held)]
        side = lo_inf if a > 0.0 else hi_inf
        assert side[bc.WRONG_INF, r] >= 1
        assert np.isfinite(lo[bc.WRONG_INF, r]) and np.isfinite(hi[bc.WRONG_INF, r])
    huge_lo, huge_hi = lo[bc.HUGE], hi[bc.HUGE]
    assert np.isnan(huge_lo).any() and np.isinf(huge_lo).any() and np.isinf(huge_hi).any()
    for which in bc.ROW_BOUND_SETS:
        lb, ub, tol = bc.row_bounds(name, which)
        g = bc.screen(bc.reference(name), lb, ub)[bc.HUGE]
        assert not np.isnan(g).any()
        bad = np.isnan(huge_lo) & np.isnan(huge_hi)
        assert bad.any() and not (g[bad] > tol).any(), (name, which)


@pytest.mark.parametrize("name", bc.SCREEN_CASES)
def test_split_condition(name):
    """At tolerance 0 every child has a proving and a non-proving row, and
    the share of proving pairs over the first k children is between 10 % and
    90 % for every k."""
    lb, ub, tol = bc.row_bounds(name, "split")
    assert tol == 0.0
    m = bc.matrix(name).m
    for k in bc.ks(name):
        starts, rows, amounts, summaries = bc.expected(name, "split", k)
        share = starts[k] / (k * m)
        print(name, k, "share", round(float(share), 3), "proving rows per child",
              int(summaries["count"].min()), "to", int(summaries["count"].max()))
        assert 0.10 <= share <= 0.90, (name, k, share)
        assert np.all(summaries["count"] >= 1) and np.all(summaries["count"] < m), (name, k)
        assert np.all(amounts > 0.0) and not np.isnan(amounts).any()


@pytest.mark.parametrize("name", bc.SCREEN_CASES)
def test_free_and_crossed(name):
    ref = bc.reference(name)
    lo, hi, lo_inf, hi_inf = ref
    k = bc.pool_size(name)
    assert bc.expected(name, "free", k)[0][k] == 0
    starts, rows, amounts, summaries = bc.expected(name, "crossed", k)
    usable = ((lo_inf == 0) & ~np.isnan(lo) & (lo != -np.inf)) | \
             ((hi_inf == 0) & ~np.isnan(hi) & (hi != np.inf))
    assert np.array_equal(np.diff(starts), usable.sum(axis=1))
    assert np.all(amounts == np.inf)
    for j in range(k):
        if usable[j].any():
            assert summaries["worst"][j] == np.inf
            assert summaries["worst_row"][j] == np.nonzero(usable[j])[0][0]
    ordinary = [j for j in bc.ALONE if j < k]
    for j in ordinary:  # without infinite bounds every row is proven
        assert summaries["count"][j] == lo.shape[1]


@pytest.mark.parametrize("which", ("edges0", "edges_tol"))
@pytest.mark.parametrize("name", bc.SCREEN_CASES)
def test_edges(name, which):
    lb, ub, tol = bc.row_bounds(name, which)
    ref = bc.reference(name)
    g = bc.screen(ref, lb, ub)
    entries = bc.edge_entries(name, which)
    assert len({r for _, r, _ in entries}) == len(entries)
    for child, r, kind in entries:
        value = (ref[0] if kind.startswith("lo") else ref[1])[child, r]
        assert bits(g[child, r]) == bits(bc.edge_target(kind, value, tol)), (name, child, r, kind)
        bound, other = (ub[r], value) if kind.startswith("lo") else (lb[r], value)
        one = (other, bound) if kind.startswith("lo") else (bound, other)
        assert exact_bound.is_one_rounding(g[child, r], *one)
        proven = bool(g[child, r] > tol)
        assert proven == kind.endswith("_above"), (name, child, r, kind)
        starts, rows, _, _ = bc.expected(name, which, child + 1)
        assert (r in rows[starts[child]:starts[child + 1]]) == proven


def test_tall_reference_against_the_loop():
    """The vectorised reference of `tall` on a sample of rows, the first and
    the last rows included."""
    mat = bc.matrix("tall")
    L, U = bc.pool("tall")
    rng = np.random.default_rng(5)
    sample = np.unique(np.concatenate([[0, 1, mat.m - 1], rng.integers(0, mat.m, 400)]))
    sub = types.SimpleNamespace(m=len(sample), t_cols=[mat.t_cols[r] for r in sample],
                                t_vals=[mat.t_vals[r] for r in sample])
    want = bc.ranges(sub, L, U)
    got = tuple(a[:, sample] for a in bc.reference("tall"))
    bc.same_ranges(got, want, "tall")
    assert np.isnan(got[0]).any() or np.isnan(got[1]).any()
    assert got[2].any() or got[3].any()


@pytest.mark.parametrize("which", bc.OVERRIDE_SETS)
@pytest.mark.parametrize("name", bc.CASES)
def test_override_sets(name, which):
    mat = bc.matrix(name)
    base_lb, base_ub, sets = bc.override_set(name, which)
    starts, cols, lo, hi = bc.flatten(sets)
    assert starts[0] == 0 and starts[-1] == len(cols) == len(lo) == len(hi)
    assert cols.min(initial=0) >= 0 and cols.max(initial=0) < mat.n
    if which == "branch":
        L, U = bc.materialise(base_lb, base_ub, sets)
        differ = (bits(L) != bits(base_lb)) | (bits(U) != bits(base_ub))
        assert np.all(differ.sum(axis=1) <= 1) and len(sets) == 6


@pytest.mark.parametrize("name", bc.CASES)
def test_overrides_materialise_to_the_dense_pool(name):
    L, U = bc.pool(name)
    for k in (1, 5, 17, 33):
        base_lb, base_ub, sets = bc.pool_as_overrides(name, k)
        gotL, gotU = bc.materialise(base_lb, base_ub, sets)
        assert np.array_equal(bits(gotL), bits(L[:k])) and np.array_equal(bits(gotU), bits(U[:k]))
        assert bc.override_bytes(name, sets) == (16 * L.shape[1] + 20 * sum(len(c) for c, _, _ in sets)
                                                 + 8 * (k + 1))


def test_branch_overrides_equal_branch_lps():
    """cpsat.branch_overrides, materialised, is branch_lps exactly."""
    rng = np.random.default_rng(11)
    n = 12
    trail = types.SimpleNamespace(lb=np.floor(rng.uniform(-5, 0, n)),
                                  ub=np.ceil(rng.uniform(1, 6, n)))
    x = rng.uniform(trail.lb, trail.ub)
    cols = [7, 0, 11, 3]
    lbs, ubs = cpsat.branch_lps(trail, x, cols)
    base_lb, base_ub, overrides = cpsat.branch_overrides(trail, x, cols)
    assert len(overrides) == 2 * len(cols)
    assert all(len(c) == len(lo) == len(hi) == 1 for c, lo, hi in overrides)
    gotL, gotU = bc.materialise(base_lb, base_ub, overrides)
    assert gotL.dtype == lbs.dtype and gotU.dtype == ubs.dtype
    assert np.array_equal(bits(gotL), bits(lbs)) and np.array_equal(bits(gotU), bits(ubs))
    assert base_lb is not trail.lb and base_ub is not trail.ub
