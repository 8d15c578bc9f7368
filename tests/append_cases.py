"""Cases and the numpy reference of DeviceLp::AppendRows (rows appended to the
resident [A | I]).

A case is a matrix A (m x n, CSC) and one or more appends, each k rows given as
lists (row_starts, cols, vals; columns ascending per row). Two independent
routes give the extended matrix:

  merge()    the device's scheme on the arrays of [A | I]: per new entry its
             rank among the earlier new rows of its column, per column the
             count, an exclusive scan of the counts, every old entry moved by
             its column's shift, the new entries scattered to
             new_starts[c + 1] - add[c] + rank, the slack columns behind.
  scratch()  [A | I] in CSC and CSR built from the triplets of the extended A
             by one sort each.

tests/test_append_rows_ref_cpu.py holds them equal, array for array, on every
case; tests/test_append_rows_ops_gpu.py holds the device to them.

The cases are the smallest that reach each limit of the kernels
(kernels/matrix_kernels.hip): 256 columns per scan tile and 256 tiles per step
of the offsets scan, columns of more than 32 entries moved by a workgroup of
256 threads, the dense block packed in steps of 4 rows.
"""
from dataclasses import dataclass, field

import numpy as np

TILE = 256          # kAppendTileColumns
SHORT_COLUMN = 32   # kAppendShortColumn
THREADS = 256       # kAppendThreads


@dataclass
class Case:
    name: str
    m: int
    n: int
    col_starts: np.ndarray
    row_idx: np.ndarray
    vals: np.ndarray
    appends: list          # of (row_starts, cols, vals)
    env: dict = field(default_factory=dict)
    long_columns: bool = False  # a column of more than SHORT_COLUMN entries moves


def _value(rng, size):
    """Non-zero doubles with full mantissas, so that a misplaced entry shows."""
    return rng.uniform(0.5, 2.0, size) * rng.choice([-1.0, 1.0], size)


def _csc(m, n, col_rows, rng):
    """CSC of A from the ascending row list of every column."""
    starts = np.zeros(n + 1, np.int64)
    np.cumsum([len(r) for r in col_rows], out=starts[1:])
    rows = np.concatenate([np.asarray(r, np.int32) for r in col_rows] + [np.zeros(0, np.int32)])
    return starts, rows.astype(np.int32), _value(rng, len(rows))


def _random_columns(m, n, density, rng):
    return [np.flatnonzero(rng.random(m) < density) for _ in range(n)]


def _rows(row_cols, rng):
    """An append from the ascending column list of every new row."""
    starts = np.zeros(len(row_cols) + 1, np.int64)
    np.cumsum([len(c) for c in row_cols], out=starts[1:])
    cols = np.concatenate([np.asarray(c, np.int32) for c in row_cols] + [np.zeros(0, np.int32)])
    return starts, cols.astype(np.int32), _value(rng, len(cols))


def _random_rows(k, n, density, rng, every=(), never=(), first_last=()):
    """k rows; the columns of `every` in all of them, those of `never` in none,
    those of `first_last` in the first and the last row only."""
    out = []
    for j in range(k):
        hit = rng.random(n) < density
        hit[list(every)] = True
        hit[list(never)] = False
        hit[list(first_last)] = j in (0, k - 1)
        out.append(np.flatnonzero(hit))
    return out


def _case(name, m, n, col_rows, appends, seed, **kw):
    rng = np.random.default_rng(seed)
    starts, rows, vals = _csc(m, n, col_rows, rng)
    return Case(name, m, n, starts, rows, vals, [_rows(a, rng) for a in appends], **kw)


def _build():
    cases = []
    rng = np.random.default_rng(7)

    # k = 1, n no multiple of 64.
    cases.append(_case("k1", 5, 7, _random_columns(5, 7, 0.5, rng), [[[1, 4, 6]]], 1))

    # k = 2: column 0 in both rows, 1 in none, 2 in the first only, 3 in the
    # last only.
    cases.append(_case("k2", 6, 9, _random_columns(6, 9, 0.5, rng),
                       [[[0, 2, 5], [0, 3, 8]]], 2))

    # k = 17: an empty new row (5, slack only) and a new row over every column
    # (9: its full-row flag); column 0 in every other row too, 1 in none of
    # them, 2 in the first and the last; an old empty column that gains
    # entries (3).
    cols17 = _random_columns(40, 70, 0.3, rng)
    cols17[3] = np.zeros(0, np.int64)
    rows17 = _random_rows(17, 70, 0.3, rng, every=(0, 3), never=(1,), first_last=(2,))
    rows17[5] = np.zeros(0, np.int64)
    rows17[9] = np.arange(70)
    cases.append(_case("k17", 40, 70, cols17, [rows17], 3))

    # k = 65, more rows than a wave: column 99 in all k rows, 0 in none, 50 in
    # the first and the last only.
    cases.append(_case("k65", 10, 100, _random_columns(10, 100, 0.4, rng),
                       [_random_rows(65, 100, 0.2, rng, every=(99,), never=(0,),
                                     first_last=(50,))], 4))

    # Old columns of 31, 32 and 33 entries around the switch of the move
    # kernels, one of 600 (more than two rounds of a workgroup's 256 threads),
    # an empty one and short ones.
    m = 700
    lengths = [31, 32, 33, 600, 0, 1, 5, 33, 32, 31, 2]
    cols_len = [np.sort(rng.choice(m, size=length, replace=False)) for length in lengths]
    cases.append(_case("column_lengths", m, len(lengths), cols_len,
                       [_random_rows(3, len(lengths), 0.6, rng, every=(3, 4), never=(1,))], 5,
                       long_columns=True))

    # n over three scan tiles (and no multiple of 64), hits in the first and
    # the last column of each tile.
    n = 2 * TILE + 45
    edge = [0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, n - 1]
    cases.append(_case("three_tiles", 6, n, _random_columns(6, n, 0.3, rng),
                       [[edge, edge[::2], edge[1::2], sorted(set(edge + [7, 300, 400]))]], 6))

    # More tiles than one step of the offsets scan (256 tiles).
    n = TILE * (THREADS + 1) + 3
    far = [0, TILE * THREADS - 1, TILE * THREADS, n - 1]
    cases.append(_case("many_tiles", 3, n, _random_columns(3, n, 0.4, rng),
                       [[far, far[1:], [5, n - 2]]], 7))

    # m = 0 before the append.
    cases.append(_case("m0", 0, 9, [np.zeros(0, np.int64)] * 9,
                       [[[0, 4, 8], [], [4, 5]]], 8))

    # Two appends in a row.
    cases.append(_case("two_appends", 12, 37, _random_columns(12, 37, 0.3, rng),
                       [_random_rows(2, 37, 0.4, rng, every=(36,)),
                        _random_rows(3, 37, 0.4, rng, every=(0, 36))], 9))

    # The dense block: columns 0..5 full; 0..2 stay full (every new row hits
    # them), 3 is hit by the first row only, 4 and 5 by none: broken. Before,
    # m = 8 packs in two steps of 4 rows and no tail; after, m = 10 has a tail
    # of 2 rows.
    dense_cols = [np.arange(8)] * 6 + _random_columns(8, 6, 0.5, rng)
    cases.append(_case("dense_block", 8, 12, dense_cols,
                       [[[0, 1, 2, 3, 7], [0, 1, 2, 9]]], 10,
                       env={"MILP_DENSE_BLOCK": "force"}))
    return cases


CASES = _build()
NAMES = [c.name for c in CASES]


def case(name):
    return CASES[NAMES.index(name)]


# ---------------------------------------------------------------------------
# [A | I] from scratch.

def scratch(m, n, triplet_rows, triplet_cols, triplet_vals):
    """CSC and CSR of [A | I] from A's triplets (any order, no duplicates)."""
    r = np.concatenate([np.asarray(triplet_rows, np.int64), np.arange(m, dtype=np.int64)])
    c = np.concatenate([np.asarray(triplet_cols, np.int64), n + np.arange(m, dtype=np.int64)])
    v = np.concatenate([np.asarray(triplet_vals, np.float64), np.ones(m)])
    by_col = np.lexsort((r, c))
    by_row = np.lexsort((c, r))
    starts = np.zeros(n + m + 1, np.int64)
    np.cumsum(np.bincount(c, minlength=n + m), out=starts[1:])
    t_starts = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=m), out=t_starts[1:])
    return {"starts": starts, "rows": r[by_col].astype(np.int32), "vals": v[by_col],
            "t_starts": t_starts, "t_cols": c[by_row].astype(np.int32), "t_vals": v[by_row]}


def triplets(c, appends=None):
    """Triplets of the case's A extended by its first `appends` appends (all
    of them by default): (m, rows, cols, vals)."""
    appends = len(c.appends) if appends is None else appends
    rows = [c.row_idx.astype(np.int64)]
    cols = [np.repeat(np.arange(c.n, dtype=np.int64), np.diff(c.col_starts))]
    vals = [c.vals]
    m = c.m
    for rs, cl, vl in c.appends[:appends]:
        k = len(rs) - 1
        rows.append(m + np.repeat(np.arange(k, dtype=np.int64), np.diff(rs)))
        cols.append(cl.astype(np.int64))
        vals.append(vl)
        m += k
    return m, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)


def extended_csc(c, appends=None):
    """A itself, extended, in CSC: (m, col_starts, row_idx, vals), what a fresh
    handle is created from."""
    m, r, cl, v = triplets(c, appends)
    order = np.lexsort((r, cl))
    starts = np.zeros(c.n + 1, np.int64)
    np.cumsum(np.bincount(cl, minlength=c.n), out=starts[1:])
    return m, starts, r[order].astype(np.int32), v[order]


# ---------------------------------------------------------------------------
# The device's scheme.

def merge(old, m, n, row_starts, cols, vals):
    """old: the dict of [A | I] (m rows, n structural columns). Returns the
    dict of the matrix with the k rows appended."""
    k = len(row_starts) - 1
    e = int(row_starts[-1])
    nnz = int(old["starts"][-1])
    row_of = np.repeat(np.arange(k, dtype=np.int64), np.diff(row_starts))
    add = np.zeros(n, np.int64)
    rank = np.zeros(e, np.int64)
    for p in range(e):  # a thread per entry: the earlier rows that hold its column
        j, col = row_of[p], cols[p]
        for jj in range(j):
            lst = cols[row_starts[jj]:row_starts[jj + 1]]
            i = np.searchsorted(lst, col)
            rank[p] += int(i < len(lst) and lst[i] == col)
        add[col] += 1
    shift = np.zeros(n + 1, np.int64)
    np.cumsum(add, out=shift[1:])  # exclusive scan; shift[n] == e
    starts = np.zeros(n + m + k + 1, np.int64)
    starts[:n + 1] = old["starts"][:n + 1] + shift
    starts[n:n + m] = old["starts"][n:n + m] + e
    starts[n + m:] = nnz + e + np.arange(k + 1)
    rows = np.full(nnz + e + k, -1, np.int32)
    out_vals = np.full(nnz + e + k, np.nan)
    for col in range(n + m):  # move
        b, end = old["starts"][col], old["starts"][col + 1]
        to = starts[col]
        rows[to:to + end - b] = old["rows"][b:end]
        out_vals[to:to + end - b] = old["vals"][b:end]
    for p in range(e):  # scatter
        to = starts[cols[p] + 1] - add[cols[p]] + rank[p]
        rows[to] = m + row_of[p]
        out_vals[to] = vals[p]
    rows[nnz + e:] = m + np.arange(k)
    out_vals[nnz + e:] = 1.0
    # CSR: the old arrays, then per new row its entries and its slack.
    t_cols = [old["t_cols"]]
    t_vals = [old["t_vals"]]
    for j in range(k):
        t_cols += [cols[row_starts[j]:row_starts[j + 1]], [n + m + j]]
        t_vals += [vals[row_starts[j]:row_starts[j + 1]], [1.0]]
    t_starts = np.concatenate([old["t_starts"],
                               nnz + row_starts[1:] + np.arange(1, k + 1)]).astype(np.int64)
    return {"starts": starts, "rows": rows, "vals": out_vals, "t_starts": t_starts,
            "t_cols": np.concatenate(t_cols).astype(np.int32),
            "t_vals": np.concatenate(t_vals).astype(np.float64)}


def merged(c):
    """The case's [A | I] after all of its appends, by merge()."""
    m, r, cl, v = triplets(c, 0)
    mat = scratch(m, c.n, r, cl, v)
    for rs, cols, vals in c.appends:
        mat = merge(mat, m, c.n, rs, cols, vals)
        m += len(rs) - 1
    return m, mat

