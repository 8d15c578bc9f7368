"""Inputs of the row-sum panel tests (DeviceLp::RowSumsPanel and
RowSumsPanelFrom, mi_lp_column_combinations): tests/test_row_panel_ops_gpu.py,
checked without a GPU by tests/test_row_panel_ref_cpu.py.

TEST INFRASTRUCTURE ONLY. Values are those of tests/panel_cases.py:
+-2^e (1 + u), e uniform in [-12, 12], u uniform in [0, 1).

Matrices (CASES), by import from tests/solveops_cases.py except the last:
  rows70   m = 70: row lengths 1, 2, 3, 63, 64, 65, 128, 129, 130 and 200; a
           6-row last workgroup at 16 and at 64 rows per workgroup
  wide     m = 40, N = 33040
  dense64  a dense block beside the full CSR (MILP_DENSE_BLOCK=force); the
           row sums read the CSR only
  steps    m = 40, n = 30, of this file. row_sums_panel_kernel does not stage
           (row_panel_geometry's chunk length is 0): what it has in place of
           a chunk is its group of GATHER = 8 entries whose multipliers are
           fetched ahead of the adds. Row lengths one below, at and one above
           one and two groups, and 1 and 24.

Points: POOL = 33 per matrix, read-only; a test with k points takes the first
k, so that k in KS covers the widths 1, 4 and 16 and the splits 16 + 1 and
16 + 16 + 1. Ordinary points are solveops_cases._family (about 10 % +0.0 and
2 % -0.0). The others sit at fixed places (SPECIAL):
  1   all +0.0            2   all -0.0          (+0.0 everywhere)
  3   a NaN               6   a -inf            (in a column two rows hold)
  7   every multiplier of ROWS70_ZERO_ROW zeroed (rows70; elsewhere ordinary)
Points 0, 16 and 32 are ordinary: each is, for some k, a panel of its own.

An inf or NaN input only ever propagates: reference() asserts that every NaN
carries the input NaN's bits.
"""
import functools

import numpy as np

import panel_cases as pc
import solveops_cases as sc
from device_ref import Matrix, RefState, bits

KS = (1, 2, 4, 5, 16, 17, 33)
POOL = 33
GATHER = 8  # kRowPanelUnroll of kernels/kernel_args.h
STEPS_M, STEPS_N = 40, 30
STEPS_LENS = (7, 8, 9, 15, 16, 17, 1, 24)  # with the slack; cycled over the rows
CASES = ("rows70", "wide", "dense64", "steps")
ALL_POS_ZERO, ALL_NEG_ZERO, WITH_NAN, WITH_INF, ZERO_ROW = 1, 2, 3, 6, 7
SPECIAL = (ALL_POS_ZERO, ALL_NEG_ZERO, WITH_NAN, WITH_INF)
ALONE = (0, 16, 32)  # points that are a whole panel for some k in KS
# One seed per point: point j of a matrix is the family drawn from
# SEEDS[name] + POINT_SEED_STEP * j + POINT_TRIES[name][j]. The tries are the
# first ones with which the reference alone tells summation orders apart as
# tests/test_row_panel_ref_cpu.py asserts (on wide every row is a length class
# of its own, and a point has to change bits in each of them).
SEEDS = {"rows70": 610000, "wide": 620000, "dense64": 630000, "steps": 640000}
POINT_SEED_STEP = 1000
POINT_TRIES = {
    "rows70": (2, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 3, 0, 0, 0, 0, 0, 1, 0,
               0, 0, 0, 1),
    "wide": (16, 0, 0, 0, 13, 1, 0, 0, 2, 17, 9, 3, 1, 8, 6, 1, 17, 5, 22, 21, 11, 16, 3, 5, 1, 33,
             4, 12, 4, 7, 9, 2, 2),
    "dense64": (0,) * 33,
    "steps": (1,) + (0,) * 32,
}
STEPS_SEED = 6001


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name != "steps":
        return sc.matrix(name)
    rng = np.random.default_rng(STEPS_SEED)
    rows = []
    for r in range(STEPS_M):
        length = STEPS_LENS[r % len(STEPS_LENS)]
        cols = np.sort(rng.choice(STEPS_N, length - 1, replace=False)).astype(np.int32)
        rows.append((cols, pc._values(rng, length - 1)))
    mat = Matrix(STEPS_M, STEPS_N, rows)
    assert set(mat.row_len) == set(STEPS_LENS)
    return mat


def environment(name):
    return sc.environment(name) if name != "steps" else {}


def shared_columns(mat):
    """Columns that at least two rows hold: those held by the fewest rows
    first, by the most rows last."""
    count = np.zeros(mat.N, np.int64)
    for c in mat.t_cols:
        count[c] += 1
    shared = np.nonzero(count >= 2)[0]
    return shared[np.argsort(count[shared], kind="stable")]


@functools.lru_cache(maxsize=None)
def points(name):
    """(POOL, N), read-only."""
    mat = matrix(name)
    x = np.stack([sc._family(np.random.default_rng(SEEDS[name] + POINT_SEED_STEP * j + t), mat.N)
                  for j, t in enumerate(POINT_TRIES[name])])
    assert x.shape == (POOL, mat.N)
    x[ALL_POS_ZERO] = 0.0
    x[ALL_NEG_ZERO] = -0.0
    shared = shared_columns(mat)
    assert len(shared) >= 2
    x[WITH_NAN, shared[0]] = np.nan
    x[WITH_INF, shared[-1]] = -np.inf
    if name == "rows70":
        cols = mat.t_cols[sc.ROWS70_ZERO_ROW]
        x[ZERO_ROW, cols[0]], x[ZERO_ROW, cols[1]] = 0.0, -0.0
    x.setflags(write=False)
    return x


def ordinary(name):
    """Indices of the points that hold the family's values only."""
    return [j for j in range(POOL) if j not in SPECIAL]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(POOL, m): RefState.row_sums(x_j, None, 1.0) of every point, computed
    once and read-only."""
    ref = RefState(matrix(name))
    out = np.stack([ref.row_sums(x, None, 1.0) for x in points(name)])
    assert sc.only_input_nans(out), name
    out.setflags(write=False)
    return out


def row_sums_pairwise(mat, x):
    """The reference's live terms added as a balanced tree: the first half
    (rounded down) of the terms, the second half, then their sum."""
    def tree(p):
        if len(p) == 1:
            return p[0]
        return tree(p[:len(p) // 2]) + tree(p[len(p) // 2:])

    out = np.zeros(mat.m)
    for r in range(mat.m):
        mult = x[mat.t_cols[r]]
        live = mult != 0.0
        p = mult[live] * mat.t_vals[r][live]
        out[r] = tree(list(p)) if len(p) else 0.0
    return out


def orders_not_told_apart(name, pts=None):
    """Where the points fail to tell the reference's order from the reversed
    order (solveops_cases.row_sums_reversed) or from the balanced tree, as
    (order, what, row length) triples; empty when
      - every ordinary point changes bits in at least one row of every length
        class >= 63, and
      - over every panel of every k in KS, every length class >= 3 changes
        bits in at least one (row, point) pair."""
    mat = matrix(name)
    pts = points(name) if pts is None else pts
    ref = RefState(mat)
    fwd = np.stack([ref.row_sums(x, None, 1.0) for x in pts])
    missed = []
    for order, other in (("reversed", lambda x: sc.row_sums_reversed(mat, x, None, 1.0)),
                         ("pairwise", lambda x: row_sums_pairwise(mat, x))):
        changed = bits(fwd) != bits(np.stack([other(x) for x in pts]))  # (POOL, m)
        for L in np.unique(mat.row_len):
            rows = mat.row_len == L
            if L >= 63:
                missed += [(order, f"point {j}", int(L)) for j in ordinary(name)
                           if not changed[j][rows].any()]
            if L >= 3:
                for k in KS:
                    missed += [(order, f"k {k} panel at {first}", int(L))
                               for first, count in panels(k)
                               if not changed[first:first + count][:, rows].any()]
    return missed


def panels(k):
    """The (first, count) panels of a call with k points."""
    return [(first, min(16, k - first)) for first in range(0, k, 16)]


def width(count):
    return 1 if count == 1 else (4 if count <= 4 else 16)


# --- overrides ------------------------------------------------------------------------------------

OVERRIDE_SETS = ("one", "four", "mixed", "k17")
MANY = 65  # the point of "mixed" that overrides at least this many columns


@functools.lru_cache(maxsize=None)
def override_set(name, which):
    """(base, [(cols int32, vals float64), ...]). "mixed" (k = 5): no
    overrides; column 0 and column N - 1; 0.0, -0.0, NaN and inf; at least
    MANY columns; a few. "four" is its first four points, "one" its last.
    "k17": 17 points of a few overrides each, over one base and across a panel
    boundary. Columns are unsorted and distinct within a point."""
    mat = matrix(name)
    rng = np.random.default_rng(SEEDS[name] + 50)
    base = sc._family(rng, mat.N)
    base.setflags(write=False)

    def some(count):
        cols = rng.permutation(mat.N)[:count].astype(np.int32)
        return cols, pc._values(rng, count)

    if which == "k17":
        sets = [some(int(rng.integers(1, 6))) for _ in range(17)]
    else:
        shared = [c for c in shared_columns(mat) if base[c] != 0.0]
        special = np.array([shared[1], shared[2], shared[0], shared[-1]], np.int32)
        assert len(set(special.tolist())) == 4
        many = min(mat.N, MANY + 5)
        mixed = [(np.zeros(0, np.int32), np.zeros(0)),
                 (np.array([mat.N - 1, 0], np.int32), pc._values(rng, 2)),
                 (special, np.array([0.0, -0.0, np.nan, np.inf])),
                 some(many), some(3)]
        assert many >= MANY
        sets = {"mixed": mixed, "four": mixed[:4], "one": mixed[4:]}[which]
    for cols, vals in sets:
        assert len(set(cols.tolist())) == len(cols) == len(vals)
    return base, sets


def materialise(base, sets):
    """The dense points of an override set: the header's definition."""
    x = np.tile(np.asarray(base, np.float64), (len(sets), 1))
    for j, (cols, vals) in enumerate(sets):
        x[j, cols] = vals
    return x


def flatten(sets):
    """starts (k + 1, int64), cols (int32), vals (float64) of the C call."""
    starts = np.zeros(len(sets) + 1, np.int64)
    np.cumsum([len(c) for c, _ in sets], out=starts[1:])
    cols = np.concatenate([np.zeros(0, np.int32)] + [c for c, _ in sets]).astype(np.int32)
    vals = np.concatenate([np.zeros(0)] + [v for _, v in sets]).astype(np.float64)
    return starts, cols, vals


@functools.lru_cache(maxsize=None)
def override_reference(name, which):
    """(k, m): the reference on the materialised points."""
    base, sets = override_set(name, which)
    ref = RefState(matrix(name))
    out = np.stack([ref.row_sums(x, None, 1.0) for x in materialise(base, sets)])
    assert sc.only_input_nans(out), (name, which)
    out.setflags(write=False)
    return out


def override_bytes(name, which):
    """What the override call sends up: base, (column, value) pairs, starts."""
    _, sets = override_set(name, which)
    return 8 * matrix(name).N + 12 * sum(len(c) for c, _ in sets) + 8 * (len(sets) + 1)
