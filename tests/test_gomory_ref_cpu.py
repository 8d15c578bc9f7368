"""The inputs of tests/gomory_cases.py meet the conditions the GPU test relies
on, and the reference's summaries do not depend on the order of the reduction.
No GPU and no engine: numpy only.

The last tests check the rule itself against the CPU oracle: on small mixed
integer instances every cut the rule builds from a fractional basic integer
column of the LP optimum holds at every integer witness point, and
cpsat.gomory_cuts runs on the oracle's handle.
"""
import functools
import math

import numpy as np
import pytest

import gomory_cases as gc
import panel_sparse_cases as sc
import penalty_cases as pn
from device_ref import bits


def same_summaries(got, want, what):
    assert got.dtype == want.dtype == gc.SUMMARY and got.shape == want.shape, what
    for f in ("max_abs", "min_abs"):
        assert np.array_equal(bits(got[f]), bits(want[f])), (what, f, got[f], want[f])
    for f in ("count", "bad_count", "max_col", "min_col"):
        assert np.array_equal(got[f], want[f]), (what, f, got[f], want[f])


@functools.lru_cache(maxsize=None)
def rule(name, variant):
    p = gc.inputs(name, variant)
    return gc.coefficients(gc.alpha(name), p["status"], p["unit"], p["f0"], p["row_unit"],
                           p["zero_tolerance"])


@pytest.mark.parametrize("name", gc.NAMES)
def test_the_special_vectors(name):
    mat = sc.matrix(name)
    a = gc.alpha(name)
    for variant in gc.VARIANTS:
        p = gc.inputs(name, variant)
        g, bad, c = gc.parts(name, variant)
        status, unit = p["status"], p["unit"]
        takes_part = (status == gc.AT_LOWER_BOUND) | (status == gc.AT_UPPER_BOUND)
        # The NaN: alpha is NaN on columns that take part; g is +0.0 there and
        # the columns are counted.
        nan = np.isnan(a[gc.NAN_VECTOR])
        assert (nan & takes_part).any() and not np.isnan(np.delete(a, gc.NAN_VECTOR, axis=0)).any()
        assert np.all(bits(g[gc.NAN_VECTOR][nan]) == 0)
        assert bad[gc.NAN_VECTOR] >= (nan & (status >= gc.AT_LOWER_BOUND)).sum() > 0
        # y' = 0: no slack of the unit vector has a coefficient, every s is
        # +0.0 and c is g in every bit.
        assert status[mat.n + pn._unit_row(name)[0]] == gc.BASIC
        assert np.all(bits(g[gc.UNIT_VECTOR, mat.n:]) == 0)
        assert np.array_equal(bits(c[gc.UNIT_VECTOR]), bits(g[gc.UNIT_VECTOR, :mat.n]))
        # ... and only there: the other vectors' slack parts are not zero.
        others = np.delete(np.arange(len(g)), gc.UNIT_VECTOR)
        assert all((g[v, mat.n:] != 0).any() for v in others)
        # The tie: f == f0 exactly on an integer column that takes part; the
        # first branch gives gamma = f / f0 = 1, so |g| = 1 / unit.
        col = p["tie_column"]
        f = gc.fractional_parts(a[gc.TIE_VECTOR:gc.TIE_VECTOR + 1], status, unit,
                                p["row_unit"][gc.TIE_VECTOR:gc.TIE_VECTOR + 1])[0]
        assert unit[col] > 0 and takes_part[col] and f[col] == p["f0"][gc.TIE_VECTOR]
        assert 0.0 < f[col] < 1.0 and abs(g[gc.TIE_VECTOR, col]) == 1.0 / unit[col]
        # Every f0 is strictly inside (0, 1) and every row_unit a power of two.
        assert np.all((p["f0"] > 0) & (p["f0"] < 1))
        assert np.all(np.frexp(p["row_unit"])[0] == 0.5)
        # g is never -0.0.
        assert not (np.signbit(g) & (g == 0)).any()
    # Somewhere the unit vector has a cut that is not empty.
    assert any((gc.parts(n, "a")[2][gc.UNIT_VECTOR] != 0).any() for n in gc.NAMES)


@pytest.mark.parametrize("name", gc.NAMES)
def test_the_tolerances_are_strict_hits(name):
    a = gc.alpha(name)
    for variant in gc.VARIANTS:
        p = gc.inputs(name, variant)
        g = gc.parts(name, variant)[0]
        takes_part = (p["status"] == gc.AT_LOWER_BOUND) | (p["status"] == gc.AT_UPPER_BOUND)
        at = (np.abs(a[0]) == p["zero_tolerance"]) & takes_part
        assert p["zero_tolerance"] > 0 and at.any() and np.all(bits(g[0][at]) == 0)
        below = gc.coefficients(a[:1], p["status"], p["unit"], p["f0"][:1], p["row_unit"][:1],
                                float(np.nextafter(p["zero_tolerance"], 0.0)))[0]
        assert (below[0][at] != 0).all()
        # The drop tolerances: an existing |c| is dropped by its own value and
        # kept by the next smaller one; the median splits the entries.
        drops = gc.drop_tolerances(name, variant)
        c = gc.parts(name, variant)[2]
        hit = drops["hit_column"]
        assert drops["hit"] > 0 and abs(c[0, hit]) == drops["hit"]
        starts, cols, _, summaries = gc.expected(name, variant, "hit")
        assert hit not in cols[:starts[1]]
        kept_below = gc.cut_lists(c[:1], float(np.nextafter(drops["hit"], 0.0)))
        assert hit in kept_below[1]
        total = gc.expected(name, variant, "zero")[0][-1]
        median = gc.expected(name, variant, "median")[0][-1]
        assert 0 < median < total
        # count is the list length, the columns ascend strictly.
        for drop in gc.DROPS:
            starts, cols, vals, summaries = gc.expected(name, variant, drop)
            assert np.array_equal(np.diff(starts), summaries["count"])
            for v in range(len(summaries)):
                assert np.all(np.diff(cols[starts[v]:starts[v + 1]]) > 0)


@pytest.mark.parametrize("name", gc.NAMES)
def test_bad_columns_without_a_nan_only_with_free_columns(name):
    """Variant "a" has no FREE column: only NAN_VECTOR has bad columns. In
    variant "b" every vector but UNIT_VECTOR has (that vector meets the few
    columns of one row, and none of those is FREE)."""
    bad_a, bad_b = gc.parts(name, "a")[1], gc.parts(name, "b")[1]
    others = np.delete(np.arange(len(bad_a)), [gc.NAN_VECTOR])
    assert np.all(bad_a[others] == 0) and bad_a[gc.NAN_VECTOR] > 0
    assert (gc.inputs(name, "b")["status"] == gc.FREE).any()
    assert np.all(np.delete(bad_b, gc.UNIT_VECTOR) > 0) and bad_b[gc.NAN_VECTOR] > bad_b[0]
    # No NaN coefficient in these cases: bad_count is the columns' count.
    for variant in gc.VARIANTS:
        assert not np.isnan(gc.parts(name, variant)[2]).any()


@pytest.mark.parametrize("name", gc.NAMES)
@pytest.mark.parametrize("variant", gc.VARIANTS)
def test_the_summaries_do_not_depend_on_the_order_of_the_reduction(name, variant):
    _, bad = rule(name, variant)
    c = gc.parts(name, variant)[2]
    k = min(len(c), 5)
    tiles, tiles_n = gc.tiles(name)
    N = bad.shape[1]
    bad_by_tile = np.stack([bad[:k, t * gc.TILE_COLUMNS:min(N, (t + 1) * gc.TILE_COLUMNS)]
                            .sum(axis=1) for t in range(tiles)], axis=1)
    rng = np.random.default_rng(5)
    for drop in gc.DROPS:
        tolerance = gc.drop_tolerances(name, variant)[drop]
        want = gc.expected(name, variant, drop)[3][:k]
        same_summaries(gc.summarize_by_tiles(c[:k], tolerance, bad_by_tile, range(tiles_n)), want,
                       "tiles forward")
        same_summaries(gc.summarize_by_tiles(c[:k], tolerance, bad_by_tile,
                                             rng.permutation(tiles_n)), want, "tiles shuffled")


def test_a_nan_coefficient_is_dropped_and_counted():
    # inf - inf: g = +inf and s = +inf on one column.
    c = np.array([[1.0, np.nan, -2.0, np.inf, -0.0]])
    s = gc.summarize(c, 0.0, np.array([3]))
    assert s["count"][0] == 3 and s["bad_count"][0] == 4
    assert s["max_abs"][0] == np.inf and s["max_col"][0] == 3
    assert s["min_abs"][0] == 1.0 and s["min_col"][0] == 0
    starts, cols, vals = gc.cut_lists(c, 0.0)
    assert cols.tolist() == [0, 2, 3]


# --- the rule is valid: integer witnesses against the cuts -------------------------

SEEDS = range(40)
INTEGER_COLUMNS, CONTINUOUS_COLUMNS, ROWS, WITNESSES = 6, 3, 5, 6
# Measured with the oracle on the CPU over the 40 instances below (the test
# prints both): the worst shortfall rhs - c . x_w over all cuts and witnesses,
# and the worst |rhs - (1 + g . [x*; s*])|, rhs being 1 + fsum(c x*).
# 60 cuts; no witness is tight on any of them.
MEASURED_WORST_SHORTFALL = -1.3561838575758323
MEASURED_WORST_RHS_GAP = 1.1368683772161603e-13
MARGIN_ULPS = 16


def witness_instance(seed):
    """A 5 x 9 mixed integer instance with 6 integer witness points: integer
    column j steps by unit[j], a power of two (the LP is scaled); the row
    bounds are the hull of the witnesses' activities, so every witness is
    feasible; a random objective."""
    from mi_glop.lp import LinearProgram
    rng = np.random.default_rng(12000 + seed)
    n = INTEGER_COLUMNS + CONTINUOUS_COLUMNS
    A = rng.integers(-6, 7, (ROWS, n)).astype(np.float64) / 2.0
    A[rng.random((ROWS, n)) < 0.25] = 0.0
    unit = np.concatenate([np.ldexp(1.0, rng.integers(-2, 3, INTEGER_COLUMNS)),
                           np.zeros(CONTINUOUS_COLUMNS)])
    ub = np.concatenate([6.0 * unit[:INTEGER_COLUMNS], np.full(CONTINUOUS_COLUMNS, 10.0)])
    w = np.concatenate([rng.integers(0, 7, (WITNESSES, INTEGER_COLUMNS)) * unit[:INTEGER_COLUMNS],
                        rng.uniform(0.0, 10.0, (WITNESSES, CONTINUOUS_COLUMNS))], axis=1)
    act = w @ A.T
    cols = [np.nonzero(A[:, j])[0] for j in range(n)]
    cs = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    ri = np.concatenate(cols).astype(np.int32)
    va = np.concatenate([A[c, j] for j, c in enumerate(cols)])
    lp = LinearProgram(ROWS, n, cs, ri, va, np.zeros(n), ub, act.min(axis=0), act.max(axis=0),
                       rng.uniform(-1.0, 1.0, n), 0.0, 1.0, False, f"witness_s{seed}")
    return lp, unit, w


def test_cuts_hold_at_every_integer_witness():
    """For every fractional integer basic column of the LP optimum the cut
    sum c_j x_j >= rhs, rhs = 1 + fsum(c x*), holds at every witness.

    Measured here with the oracle: see MEASURED_WORST_SHORTFALL and
    MEASURED_WORST_RHS_GAP above and DESIGN.md section 7. Cut validity in
    doubles is only ever approximate (c carries the roundings of two dot
    passes and of the rule), so the margin is a floor of MARGIN_ULPS ulp of
    1 + sum |c_j x_j| (witness and LP point together) over the measured
    shortfall where that is positive (it is not: the floor alone). The gap
    between rhs and 1 + g . [x*; s*] is two sums of the same real number: it
    is bounded by the rounding of the second pass, (ROWS + 3) eps per
    coefficient against sum_r |y'_r a_rj|, weighed with |x*_j|, plus the
    roundings of the subtraction; 16 eps of the magnitudes' sum covers ROWS =
    5. At least 30 cuts are required, so that the test cannot pass
    vacuously."""
    import oracle_lib
    from mi_glop import abi
    params = abi.default_params(use_dual_simplex=1, max_number_of_iterations=1000)
    cuts = 0
    worst, worst_gap, worst_ratio = -np.inf, 0.0, 0.0
    for seed in SEEDS:
        lp, unit, witnesses = witness_instance(seed)
        o = oracle_lib.OracleLp(params)
        o.load(lp)
        assert o.solve().problem_status == abi.OPTIMAL
        state = np.asarray(o.state())
        x = np.asarray(o.primal())
        t = x[:INTEGER_COLUMNS] / unit[:INTEGER_COLUMNS]
        frac = t - np.floor(t)
        cols = [j for j in range(INTEGER_COLUMNS)
                if state[j] == gc.BASIC and 1e-6 < frac[j] < 1 - 1e-6]
        if not cols:
            continue
        (starts, ccols, vals, summaries), g = gc.node_reference(o, lp, cols, unit)
        point = np.concatenate([x, -np.asarray(o.activities())])
        dense = np.zeros((lp.m, lp.n))
        for col in range(lp.n):
            e = slice(lp.col_starts[col], lp.col_starts[col + 1])
            dense[lp.row_idx[e], col] = lp.vals[e]
        for j in range(len(cols)):
            assert summaries["bad_count"][j] == 0 and summaries["count"][j] > 0
            idx, c = ccols[starts[j]:starts[j + 1]], vals[starts[j]:starts[j + 1]]
            rhs = 1.0 + math.fsum(c * x[idx])
            gap = abs(rhs - (1.0 + math.fsum(g[j] * point)))
            worst_gap = max(worst_gap, gap)
            magnitude = 1.0 + np.abs(g[j] * point).sum() + np.abs(c * x[idx]).sum() + \
                float(np.abs(x) @ (np.abs(dense.T) @ np.abs(g[j, lp.n:])))
            assert gap <= 16 * np.finfo(np.float64).eps * magnitude, (seed, cols[j], gap)
            worst_ratio = max(worst_ratio, gap / (np.finfo(np.float64).eps * magnitude))
            for w in witnesses:
                lhs = math.fsum(c * w[idx])
                scale = 1.0 + np.abs(c * w[idx]).sum() + np.abs(c * x[idx]).sum()
                margin = max(0.0, MEASURED_WORST_SHORTFALL) + MARGIN_ULPS * np.spacing(scale)
                worst = max(worst, rhs - lhs)
                assert rhs - lhs <= margin, (seed, cols[j], rhs, lhs)
            cuts += 1
    print("cuts", cuts, "worst shortfall", worst, "worst rhs gap", worst_gap,
          "in eps of the magnitudes", worst_ratio)
    assert cuts >= 30


def test_cpsat_gomory_cuts_on_the_oracle():
    """cpsat.gomory_cuts needs one call of its handle: here the oracle's
    handle with that call served by the reference."""
    import jobshop
    import oracle_lib
    from mi_glop import abi, cpsat

    class OracleWithCuts(oracle_lib.OracleLp):
        def gomory_cuts(self, cols, unit, zero_tolerance=0.0, drop_tolerance=0.0):
            return gc.node_reference(self, self.lp, cols, unit, zero_tolerance, drop_tolerance)[0]

    p = abi.default_params(use_dual_simplex=1, max_number_of_iterations=1000)
    lp, ycols = jobshop.relaxation(jobshop.random_instance(6, 4, 7))
    for scaling in (False, True):
        c = cpsat.LpConstraint(lp, ycols, OracleWithCuts(p), scaling=scaling)
        t = cpsat.IntegerTrail(lp.col_lb, lp.col_ub)
        assert c.solve_lp(t) and c.analyze_lp(t)
        cols = cpsat.fractional_columns(c.lp_solution, ycols, limit=20)
        cuts = cpsat.gomory_cuts(c, c.lp_solution, cols)
        assert 0 < len(cuts) <= len(cols)
        x_lp = np.asarray(c.lp_solution, np.float64) * c.factor
        for cut in cuts:
            assert cut["col"] in cols and len(cut["cols"]) == len(cut["coefs"]) > 0
            assert np.all(np.diff(cut["cols"]) > 0)
            assert cut["max_abs"] >= cut["min_abs"] > 0
            assert cut["rhs"] == 1.0 + math.fsum(cut["coefs"] * x_lp[cut["cols"]])
            # The LP point violates the cut by exactly 1 (at the LP's scale).
            lhs = math.fsum(cut["coefs"] * x_lp[cut["cols"]])
            assert abs((cut["rhs"] - lhs) - 1.0) <= 4 * np.spacing(abs(cut["rhs"]) + 1.0)
