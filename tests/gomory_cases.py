"""Inputs and numpy reference of the Gomory cut tests (DeviceLp::ColumnCutsPanel;
the rule is stated in include/mi_lp.h at mi_lp_row_gomory_cuts).

TEST INFRASTRUCTURE ONLY. The matrices and vectors are those of
tests/penalty_cases.py (quad, wave, dense13, long, edge; NAN_VECTOR and
UNIT_VECTOR included), the statuses and units those of its variants:

  "a"  BASIC, FIXED_VALUE, AT_LOWER_BOUND and AT_UPPER_BOUND columns, units
       (powers of two) on about 40 % of the columns.
  "b"  the same with FREE columns: every vector has bad columns.

with one change: the slack of UNIT_VECTOR's row is BASIC. The per-vector
inputs are f0 from [0.05, 0.95] and row_unit, a power of two. Special vectors:

  NAN_VECTOR    alpha is NaN on the columns of one row: g = +0.0 there and the
                columns count in bad_count (in variant "a" this is the only
                vector with bad_count > 0).
  UNIT_VECTOR   e_r with the slack of row r BASIC: g is +0.0 on every slack,
                y' = 0, and every s is +0.0: c = g.
  TIE_VECTOR    its f0 is the f of one integer column (TIE_COLUMN) under it:
                the `f <= f0` branch is taken with equality.

The zero tolerance is the smallest non-zero fabs(alpha) of vector 0 among the
columns that take part (a strict hit: that column gets g = +0.0). The drop
tolerances are 0, the median fabs(c) and one existing fabs(c) (a strict hit:
that entry is dropped).

The expected result is always the reference below: device_ref.
column_scalar_products of every column (alpha), the rule in element-wise numpy
operations, column_scalar_products of the structural columns again (s), one
subtraction and the filter. tests/test_gomory_ref_cpu.py asserts that each of
these conditions occurs where it is claimed.
"""
import functools

import numpy as np

import panel_sparse_cases as sc
import penalty_cases as pn
from device_ref import column_scalar_products

TILE_COLUMNS = sc.TILE_COLUMNS
BASIC, FIXED_VALUE, AT_LOWER_BOUND, AT_UPPER_BOUND, FREE = range(5)
SUMMARY = np.dtype([("max_abs", np.float64), ("min_abs", np.float64), ("count", np.int32),
                    ("bad_count", np.int32), ("max_col", np.int32), ("min_col", np.int32)])
assert SUMMARY.itemsize == 32

NAMES = pn.NAMES
VARIANTS = pn.VARIANTS
KS = pn.KS
DROPS = ("zero", "median", "hit")
NAN_VECTOR, UNIT_VECTOR = pn.NAN_VECTOR, pn.UNIT_VECTOR
TIE_VECTOR = 3

max_k = pn.max_k
environment = pn.environment
vectors = pn.vectors
alpha = pn.alpha


def tiles(name):
    """(tiles over all N columns, tiles over the n structural columns)."""
    mat = sc.matrix(name)
    return ((mat.N + TILE_COLUMNS - 1) // TILE_COLUMNS, (mat.n + TILE_COLUMNS - 1) // TILE_COLUMNS)


def fractional_parts(a, status, unit, row_unit):
    """f of step 5 for every (vector, column), whatever the column's kind."""
    with np.errstate(all="ignore"):
        abar = np.where((status == AT_LOWER_BOUND)[None], a, -a)
        t = (abar * unit[None]) / row_unit[:, None]
        return t - np.floor(t)


def coefficients(a, status, unit, f0, row_unit, zero_tolerance):
    """(g (k, N), bad (k, N) bool): steps 1-6 of the rule per (vector,
    column), every operation one numpy element-wise IEEE operation."""
    a = np.asarray(a, np.float64)
    status = np.asarray(status)
    unit = np.zeros(a.shape[1]) if unit is None else np.asarray(unit, np.float64)
    f0 = np.asarray(f0, np.float64)[:, None]
    ru = np.asarray(row_unit, np.float64)[:, None]
    lower = (status == AT_LOWER_BOUND)[None]
    bounded = lower | (status == AT_UPPER_BOUND)[None]
    free = (status == FREE)[None]
    u = unit[None]
    with np.errstate(all="ignore"):
        nan = np.isnan(a)
        above = np.abs(a) > zero_tolerance
        abar = np.where(lower, a, -a)
        # integer columns
        t = (abar * u) / ru
        f = t - np.floor(t)
        gamma_int = np.where(f <= f0, f / f0, (1.0 - f) / (1.0 - f0))
        gamma_int = gamma_int / u
        # continuous columns
        t = abar / ru
        gamma_cont = np.where(t > 0, t / f0, (-t) / (1.0 - f0))
        gamma = np.where(u > 0, gamma_int, gamma_cont)
        g = np.where(lower, gamma, 0.0 - gamma)
    g = np.where(bounded & ~nan & above, g, 0.0)
    bad = ((bounded | free) & nan) | (free & ~nan & above)
    return g, bad


def summarize(c, drop_tolerance, bad_columns, base=0):
    """SUMMARY records of the coefficients c (k, columns): the keep rule, the
    extrema with the lowest column attaining each, the counts. bad_columns
    (k,) is added to the NaN c's; columns are numbered from `base`."""
    k = c.shape[0]
    out = np.zeros(k, SUMMARY)
    with np.errstate(invalid="ignore"):
        mag = np.abs(c)
        keep = mag > drop_tolerance
    out["count"] = keep.sum(axis=1)
    out["bad_count"] = np.isnan(c).sum(axis=1) + bad_columns
    for v in range(k):
        kept = np.nonzero(keep[v])[0]
        if len(kept) == 0:
            out[v]["max_abs"], out[v]["min_abs"] = 0.0, np.inf
            out[v]["max_col"] = out[v]["min_col"] = -1
            continue
        m = mag[v][kept]
        out[v]["max_abs"], out[v]["min_abs"] = m.max(), m.min()
        out[v]["max_col"] = base + kept[np.argmax(m)]  # argmax / argmin: the first, the lowest
        out[v]["min_col"] = base + kept[np.argmin(m)]
    return out


def merge_summaries(x, y):
    """Two SUMMARY records of disjoint column sets into one: the kernels'
    merge (the larger / smaller value; among equal values the lower column;
    integer sums)."""
    out = np.zeros((), SUMMARY)
    out["count"] = x["count"] + y["count"]
    out["bad_count"] = x["bad_count"] + y["bad_count"]
    for value, col, better in (("max_abs", "max_col", lambda p, q: p > q),
                               ("min_abs", "min_col", lambda p, q: p < q)):
        xc = x[col] if x[col] >= 0 else pn.NO_COLUMN
        yc = y[col] if y[col] >= 0 else pn.NO_COLUMN
        take_y = better(y[value], x[value]) or (y[value] == x[value] and yc < xc)
        out[value], c = (y[value], yc) if take_y else (x[value], xc)
        out[col] = -1 if c == pn.NO_COLUMN else c
    return out


def summarize_by_tiles(c, drop_tolerance, bad_by_tile, tile_order):
    """The summaries when every tile of TILE_COLUMNS structural columns is
    summarized on its own and the tiles' records (and the bad-column counts
    per tile of all N columns, bad_by_tile (k, tiles)) are merged in
    `tile_order`, a permutation of the structural tiles."""
    k, n = c.shape
    out = np.zeros(k, SUMMARY)
    for v in range(k):
        acc = np.zeros((), SUMMARY)
        acc["min_abs"], acc["max_col"], acc["min_col"] = np.inf, -1, -1
        for t in tile_order:
            s = slice(t * TILE_COLUMNS, min(n, (t + 1) * TILE_COLUMNS))
            part = summarize(c[v:v + 1, s], drop_tolerance, np.zeros(1, np.int64),
                             base=t * TILE_COLUMNS)[0]
            acc = merge_summaries(acc, part)
        acc["bad_count"] += bad_by_tile[v].sum()
        out[v] = acc
    return out


def reference(mat, y, status, unit, f0, row_unit, zero_tolerance, a=None):
    """(g (k, N), bad columns (k,), c (k, n)) of the vectors y (k, m): alpha
    (given, or computed here), the rule, the second pass and the subtraction."""
    every = np.arange(mat.N)
    with np.errstate(invalid="ignore", over="ignore"):
        if a is None:
            a = np.stack([column_scalar_products(mat, every, v) for v in y]) \
                if len(y) else np.zeros((0, mat.N))
        g, bad = coefficients(a, status, unit, f0, row_unit, zero_tolerance)
        structural = np.arange(mat.n)
        s = np.stack([column_scalar_products(mat, structural, np.ascontiguousarray(v[mat.n:]))
                      for v in g]) if len(g) else np.zeros((0, mat.n))
        c = g[:, :mat.n] - s
    return g, bad.sum(axis=1), c


def cut_lists(c, drop_tolerance):
    """(row_starts, cols, vals) of the kept entries."""
    return sc.filtered(c, np.ones(c.shape[1], bool), drop_tolerance)


# --- the cases ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def inputs(name, variant):
    """dict of read-only arrays: status (int8), unit (N each), f0, row_unit
    (max_k each), the zero tolerance and TIE_COLUMN."""
    mat = sc.matrix(name)
    a = alpha(name)
    k = max_k(name)
    p = pn.inputs(name, variant)
    status = np.array(p["status"])
    unit_row = pn._unit_row(name)[0]
    status[mat.n + unit_row] = BASIC
    unit = np.array(p["unit"])
    rng = np.random.default_rng(9000 + NAMES.index(name))
    f0 = 0.05 + 0.9 * rng.random(k)
    row_unit = np.ldexp(1.0, rng.integers(-3, 4, k))
    takes_part = (status == AT_LOWER_BOUND) | (status == AT_UPPER_BOUND)
    zero_tolerance = float(np.abs(a[0][takes_part & (a[0] != 0.0)]).min())
    # The tie: the first integer column that takes part under TIE_VECTOR with
    # an f well inside (0, 1).
    f = fractional_parts(a[TIE_VECTOR:TIE_VECTOR + 1], status, unit,
                         row_unit[TIE_VECTOR:TIE_VECTOR + 1])[0]
    with np.errstate(invalid="ignore"):
        ok = takes_part & (unit > 0) & (np.abs(a[TIE_VECTOR]) > zero_tolerance) & \
            (f >= 0.05) & (f <= 0.95)
    tie_column = int(np.nonzero(ok)[0][0])
    f0[TIE_VECTOR] = f[tie_column]
    out = {"status": status, "unit": unit, "f0": f0, "row_unit": row_unit}
    for v in out.values():
        v.setflags(write=False)
    out["zero_tolerance"] = zero_tolerance
    out["tie_column"] = tie_column
    return out


@functools.lru_cache(maxsize=None)
def parts(name, variant):
    """(g, bad columns per vector, c) of all the case's vectors, computed once
    and read-only."""
    p = inputs(name, variant)
    out = reference(sc.matrix(name), vectors(name), p["status"], p["unit"], p["f0"],
                    p["row_unit"], p["zero_tolerance"], a=alpha(name))
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def drop_tolerances(name, variant):
    """dict DROPS -> value: 0, the median of fabs(c) over the case, and
    fabs(c) of the first non-zero coefficient of vector 0 (HIT_COLUMN)."""
    c = parts(name, variant)[2]
    mag = np.abs(c)
    hit = int(np.nonzero(mag[0] > 0)[0][0])
    return {"zero": 0.0, "median": float(np.median(mag[~np.isnan(mag)])),
            "hit": float(mag[0, hit]), "hit_column": hit}


@functools.lru_cache(maxsize=None)
def expected(name, variant, drop):
    """(row_starts, cols, vals, summaries) of all the case's vectors, read-only.
    The result for the first k vectors is the prefix: row_starts[:k + 1], the
    entries before row_starts[k], summaries[:k]."""
    _, bad, c = parts(name, variant)
    tolerance = drop_tolerances(name, variant)[drop]
    out = cut_lists(c, tolerance) + (summarize(c, tolerance, bad),)
    for x in out:
        x.setflags(write=False)
    return out


def prefix(result, k):
    starts, cols, vals, summaries = result
    kept = int(starts[k])
    return starts[:k + 1], cols[:kept], vals[:kept], summaries[:k]


# --- a solved node: the reference fed from the CPU oracle ----------------------------

def node_inputs(handle, lp, cols, unit):
    """What mi_lp_gomory_cuts derives from the solver, read from a solved
    handle with the oracle's surface: (left inverses (k, m), status, unit over
    n+m columns, f0, row_unit)."""
    left, _, status, values = pn.node_inputs(handle, lp, cols)
    unit = np.asarray(unit, np.float64)
    row_unit = unit[np.asarray(cols, np.int64)]
    t = values / row_unit
    return left, status, np.concatenate([unit, np.zeros(lp.m)]), t - np.floor(t), row_unit


def node_reference(handle, lp, cols, unit, zero_tolerance=0.0, drop_tolerance=0.0):
    """(row_starts, cols, vals, summaries) mi_lp_gomory_cuts must return for
    the BASIC structural columns `cols` of the node `handle` has solved, and
    g (k, n+m) for the checks of the rule."""
    left, status, steps, f0, row_unit = node_inputs(handle, lp, cols, unit)
    g, bad, c = reference(pn.lp_matrix(lp), left, status, steps, f0, row_unit, zero_tolerance)
    return cut_lists(c, drop_tolerance) + (summarize(c, drop_tolerance, bad),), g
