"""Inputs and numpy reference of the branching penalty tests
(DeviceLp::ColumnPenaltiesPanel; the rule is stated in include/mi_lp.h at
mi_lp_row_penalties).

TEST INFRASTRUCTURE ONLY. The matrices are those of tests/panel_sparse_cases.py
(quad: short columns, wave: long columns, dense13: forced dense block, long:
several tiles and offset steps, edge: N smaller than one tile). The vectors are
that module's with three of them replaced:

  NAN_VECTOR    one entry is NaN: alpha is NaN on every column of that row.
  UNIT_VECTOR   e_r for a row r: alpha is the row's entry on the columns that
                touch r and +0.0 elsewhere. In variant "a" the statuses of
                those columns are set so that none of them can move x_B up:
                the up direction of this vector has no eligible column.
  ZERO_DIST_VECTOR  is an ordinary vector whose down distance is 0.

The expected record is always the reference below over
device_ref.column_scalar_products of every column: no other arithmetic.

Every case has two variants of the per-column inputs, because a column with a
NaN reduced cost or a FREE status offers the candidate +0.0 to (nearly) every
vector, and with such a column every minimum is 0:

  "a"  a dual feasible node: statuses BASIC, FIXED_VALUE, AT_LOWER_BOUND and
       AT_UPPER_BOUND, reduced costs of the right sign, units on 40 % of the
       columns. Two columns, PAIR, one in the first and one in the last tile,
       are AT_LOWER_BOUND with d = 2^-80 and unit = 2^10: where both are
       eligible they tie at cost * unit = 2^-70, below every other candidate
       (the unit decides the max, and the tie spans two tiles where N has
       two). The pivot tolerance is fabs(alpha) of one eligible column of
       vector 0, the smallest non-zero one.
  "b"  the same with FREE columns, and reduced costs of the wrong sign, +0.0,
       -0.0 and NaN sprinkled over it: minima of 0 with ties inside a tile.

tests/test_penalties_ref_cpu.py asserts that each of these conditions occurs
where it is claimed.
"""
import functools

import numpy as np

import panel_cases as pc
import panel_sparse_cases as sc
from device_ref import column_scalar_products

TILE_COLUMNS = sc.TILE_COLUMNS
BASIC, FIXED_VALUE, AT_LOWER_BOUND, AT_UPPER_BOUND, FREE = range(5)
RECORD = np.dtype([("down", np.float64), ("up", np.float64), ("down_col", np.int32),
                   ("up_col", np.int32), ("down_count", np.int32), ("up_count", np.int32)])
assert RECORD.itemsize == 32

NAMES = ("quad", "wave", "dense13", "long", "edge")
VARIANTS = ("a", "b")
KS = (1, 3, 4, 5, 16, 17, 33)
NAN_VECTOR, UNIT_VECTOR, ZERO_DIST_VECTOR = 1, 2, 3
TWO_TILES = ("wave", "long")  # N spans more than one tile, the last one partial


def max_k(name):
    return sc.CASES[name][3]


def environment(name):
    return sc.CASES[name][2]


def tiles(name):
    return (sc.matrix(name).N + TILE_COLUMNS - 1) // TILE_COLUMNS


@functools.lru_cache(maxsize=None)
def _unit_row(name):
    """The row of UNIT_VECTOR and of NAN_VECTOR's NaN: the two rows with the
    fewest entries among those with at least two structural ones."""
    mat = sc.matrix(name)
    order = [r for r in np.argsort(mat.row_len, kind="stable") if mat.row_len[r] >= 3]
    return int(order[0]), int(order[1])


@functools.lru_cache(maxsize=None)
def vectors(name):
    """(max_k, m), read-only."""
    mat = sc.matrix(name)
    y = np.array(sc.vectors(name))
    unit_row, nan_row = _unit_row(name)
    y[NAN_VECTOR, nan_row] = np.nan
    y[UNIT_VECTOR] = 0.0
    y[UNIT_VECTOR, unit_row] = 1.0
    assert y.shape == (max_k(name), mat.m)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def alpha(name):
    """(max_k, N): the dense reference of the case's vectors, read-only."""
    mat = sc.matrix(name)
    cols = np.arange(mat.N)
    with np.errstate(invalid="ignore"):
        out = np.stack([column_scalar_products(mat, cols, y) for y in vectors(name)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pair(name):
    """(p1, p2): the two columns of variant "a" that tie at 2^-70. p1 is the
    first column of the first tile and p2 the first other column of the last
    tile that UNIT_VECTOR and NAN_VECTOR do not reach and whose alpha under
    vector 0 is positive."""
    a = alpha(name)
    N = a.shape[1]
    ok = (a[0] > 0.0) & (a[UNIT_VECTOR] == 0.0) & ~np.isnan(a[NAN_VECTOR])
    first = np.nonzero(ok[:TILE_COLUMNS])[0]
    last0 = (tiles(name) - 1) * TILE_COLUMNS
    last = [c for c in np.nonzero(ok[last0:])[0] + last0 if c != first[0]]
    return int(first[0]), int(last[0])


@functools.lru_cache(maxsize=None)
def inputs(name, variant):
    """dict of read-only arrays: d, status (int8), unit (N each), down, up
    (max_k each), and the float tolerance."""
    mat = sc.matrix(name)
    a = alpha(name)
    N, k = mat.N, max_k(name)
    rng = np.random.default_rng(7000 + NAMES.index(name))
    status = rng.choice([BASIC, FIXED_VALUE, AT_LOWER_BOUND, AT_UPPER_BOUND], N,
                        p=[0.3, 0.1, 0.3, 0.3]).astype(np.int8)
    for c in range(4):  # every status of this variant on structural and slack columns
        status[10 + c] = status[mat.n + 5 + c] = c
    p1, p2 = pair(name)
    status[p1] = status[p2] = AT_LOWER_BOUND
    # UNIT_VECTOR: a column of its row can only move x_B down.
    touched = a[UNIT_VECTOR] != 0.0
    free_able = status >= AT_LOWER_BOUND
    status[touched & free_able & (a[UNIT_VECTOR] > 0)] = AT_LOWER_BOUND
    status[touched & free_able & (a[UNIT_VECTOR] < 0)] = AT_UPPER_BOUND
    mag = pc._values(rng, N)
    d = np.where(status == AT_UPPER_BOUND, -np.abs(mag), np.abs(mag))
    unit = np.where(rng.random(N) < 0.4, np.ldexp(1.0, rng.integers(-6, 7, N)), 0.0)
    d[[p1, p2]] = np.ldexp(1.0, -80)
    unit[[p1, p2]] = np.ldexp(1.0, 10)
    down = 0.05 + 0.9 * rng.random(k)
    up = 1.0 - down
    down[ZERO_DIST_VECTOR] = 0.0
    # The tolerance: the smallest non-zero |alpha| of vector 0 over the columns
    # that would take part.
    part = (status >= AT_LOWER_BOUND) & (a[0] != 0.0)
    tolerance = float(np.abs(a[0][part]).min())
    kind = rng.random(N)  # drawn for both variants, so that "a" and "b" share the rest
    free = rng.random(N) < 0.05
    if variant == "b":
        status[free & ~touched] = FREE
        status[4] = status[mat.n + 4] = FREE
        d[kind < 0.10] = -d[kind < 0.10]
        d[(kind >= 0.10) & (kind < 0.15)] = 0.0
        d[(kind >= 0.15) & (kind < 0.20)] = -0.0
        d[(kind >= 0.20) & (kind < 0.22)] = np.nan
        # Every kind at both bounds whatever the draw: the last four columns
        # at each bound take the wrong sign, +0.0, -0.0 and NaN.
        for bound in (AT_LOWER_BOUND, AT_UPPER_BOUND):
            at = np.nonzero(status == bound)[0][-4:]
            wrong = -1.0 if bound == AT_LOWER_BOUND else 1.0
            d[at] = [wrong, 0.0, -0.0, np.nan]
    else:
        assert variant == "a"
    out = {"d": d, "status": status, "unit": unit, "down": down, "up": up}
    for v in out.values():
        v.setflags(write=False)
    out["tolerance"] = tolerance
    return out


def candidates(a, d, status, unit, down, up, tolerance):
    """(eligible, candidate), each (k, 2, N) with direction 0 = down: the rule
    per (vector, direction, column), every operation one numpy element-wise
    IEEE operation."""
    a = np.asarray(a, np.float64)
    if unit is None:
        unit = np.zeros(len(d))
    lower, upper, free = status == AT_LOWER_BOUND, status == AT_UPPER_BOUND, status == FREE
    takes_part = lower | upper | free
    with np.errstate(all="ignore"):
        cost = np.where(lower, np.where(d > 0, d, 0.0),
                        np.where(upper, np.where(d < 0, -d, 0.0), 0.0))
        nan = np.isnan(a) | np.isnan(d)[None, :]
        abs_a = np.abs(a)
        above = abs_a > tolerance
        pos, neg = a > 0, a < 0
        by_sign = (free[None] | (lower[None] & pos) | (upper[None] & neg),
                   free[None] | (lower[None] & neg) | (upper[None] & pos))
        r = cost[None] / abs_a
        step = cost * unit
        eligible, candidate = [], []
        for dist, el in zip((down, up), by_sign):
            c = np.asarray(dist, np.float64)[:, None] * r
            c = np.where((unit > 0)[None] & (c < step[None]), step[None], c)
            c = np.where(np.isnan(c) | nan, 0.0, c)
            eligible.append(takes_part[None] & (nan | (above & el)))
            candidate.append(c)
    return np.stack(eligible, axis=1), np.stack(candidate, axis=1)


def reduce_forward(eligible, candidate):
    """The records of (eligible, candidate): minimum, lowest column attaining
    it, count."""
    k = eligible.shape[0]
    out = np.zeros(k, RECORD)
    masked = np.where(eligible, candidate, np.inf)
    for which, name in enumerate(("down", "up")):
        best = masked[:, which].min(axis=1) if masked.shape[2] else np.full(k, np.inf)
        hit = eligible[:, which] & (candidate[:, which] == best[:, None])
        count = eligible[:, which].sum(axis=1)
        out[name] = best
        out[name + "_col"] = np.where(count > 0, hit.argmax(axis=1), -1)
        out[name + "_count"] = count
    return out


def reference(a, d, status, unit, down, up, tolerance):
    return reduce_forward(*candidates(a, d, status, unit, down, up, tolerance))


@functools.lru_cache(maxsize=None)
def expected(name, variant):
    """The records of all the case's vectors, computed once and read-only."""
    p = inputs(name, variant)
    out = reference(alpha(name), p["d"], p["status"], p["unit"], p["down"], p["up"],
                    p["tolerance"])
    out.setflags(write=False)
    return out


def merge(x, y):
    """Two (value, column, count) partials into one: the kernels' merge. A
    partial without a column is (inf, NO_COLUMN, 0)."""
    if y[0] < x[0] or (y[0] == x[0] and y[1] < x[1]):
        return (y[0], y[1], x[2] + y[2])
    return (x[0], x[1], x[2] + y[2])


NO_COLUMN = 0x7fffffff
EMPTY = (np.inf, NO_COLUMN, 0)


def reduce_in_order(eligible, candidate, order):
    """The records when the columns are merged one by one in `order`."""
    k = eligible.shape[0]
    out = np.zeros(k, RECORD)
    for v in range(k):
        for which, name in enumerate(("down", "up")):
            acc = EMPTY
            e, c = eligible[v, which], candidate[v, which]
            for col in order:
                if e[col]:
                    acc = merge(acc, (c[col], int(col), 1))
            _store(out, v, name, acc)
    return out


def reduce_by_tiles(eligible, candidate, tile_order):
    """The records when every tile of TILE_COLUMNS columns is reduced on its
    own (forward) and the tiles' partials are merged in `tile_order`."""
    k, _, N = eligible.shape
    out = np.zeros(k, RECORD)
    per_tile = []
    for t in tile_order:
        s = slice(t * TILE_COLUMNS, min(N, (t + 1) * TILE_COLUMNS))
        per_tile.append((t * TILE_COLUMNS, reduce_forward(eligible[:, :, s], candidate[:, :, s])))
    for v in range(k):
        for name in ("down", "up"):
            acc = EMPTY
            for base, rec in per_tile:
                count = int(rec[name + "_count"][v])
                col = int(rec[name + "_col"][v]) + base if count else NO_COLUMN
                acc = merge(acc, (rec[name][v], col, count))
            _store(out, v, name, acc)
    return out


def _store(out, v, name, acc):
    out[name][v] = acc[0]
    out[name + "_col"][v] = -1 if acc[1] == NO_COLUMN else acc[1]
    out[name + "_count"][v] = acc[2]


# --- a solved node: the reference fed from the CPU oracle ----------------------

def lp_matrix(lp):
    """device_ref.Matrix of an LP's A."""
    from device_ref import Matrix
    rows = [([], []) for _ in range(lp.m)]
    for c in range(lp.n):
        for e in range(lp.col_starts[c], lp.col_starts[c + 1]):
            rows[lp.row_idx[e]][0].append(c)
            rows[lp.row_idx[e]][1].append(lp.vals[e])
    return Matrix(lp.m, lp.n, [(np.array(c, np.int32), np.array(v, np.float64))
                               for c, v in rows])


def node_inputs(handle, lp, cols):
    """What mi_lp_branching_penalties derives from the solver, read from a
    solved handle with the oracle's surface: (left inverses (k, m), d, status,
    values of cols). d is in the simplex's internal minimisation sense."""
    basis = np.asarray(handle.basis())
    row_of = {int(c): r for r, c in enumerate(basis)}
    left = np.stack([handle.unit_row_left_inverse(row_of[int(c)])[0] for c in cols]) \
        if len(cols) else np.zeros((0, lp.m))
    rc, duals = np.asarray(handle.reduced_costs()), np.asarray(handle.duals())
    d = np.concatenate([-rc, duals]) if lp.maximize else np.concatenate([rc, -duals])
    x = np.concatenate([np.asarray(handle.primal()), -np.asarray(handle.activities())])
    return left, d, np.asarray(handle.state(), np.int8), x[np.asarray(cols, np.int64)]


def node_reference(handle, lp, cols, down=None, up=None, unit=None, tolerance=0.0):
    """The records mi_lp_branching_penalties must return for the BASIC columns
    `cols` of the node `handle` has solved. unit: n entries, or None."""
    left, d, status, values = node_inputs(handle, lp, cols)
    mat = lp_matrix(lp)
    every = np.arange(mat.N)
    a = np.stack([column_scalar_products(mat, every, y) for y in left]) \
        if len(cols) else np.zeros((0, mat.N))
    if down is None:
        down = values - np.floor(values)
    if up is None:
        up = np.ceil(values) - values
    if unit is not None:
        unit = np.concatenate([np.asarray(unit, np.float64), np.zeros(lp.m)])
    return reference(a, d, status, unit, np.asarray(down, np.float64),
                     np.asarray(up, np.float64), tolerance)
