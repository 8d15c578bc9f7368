"""Cases and the numpy reference of DeviceLp::DeleteRows (rows deleted from the
resident [A | I]).

A case is a matrix A (m x n, CSC) and a sequence of steps on one handle, each
("delete", mask) or ("append", (row_starts, cols, vals)). Two independent
routes give the matrix after a delete:

  compact()  the device's scheme on the arrays of [A | I]: new_row as the
             exclusive scan of the keep flags, the CSR starts as the scan of
             the kept rows' lengths, each kept row moved with its slack
             renumbered, per column the count of kept entries and its scan,
             each column compacted in order, the kept slack columns behind.
  scratch()  [A | I] in CSC and CSR built from the triplets of the reduced A
             by one sort each (append_cases.scratch).

tests/test_delete_rows_ref_cpu.py holds them equal, array for array, on every
case; tests/test_delete_rows_native_cpu.py holds the host's lp_data.h routines
to them, tests/test_delete_rows_ops_gpu.py the device.

The cases are the smallest that reach each limit of the kernels
(kernels/matrix_kernels.hip): 256 rows or columns per scan tile and 256 tiles
per step of the offsets scans, columns and rows of more than 32 entries moved
by a workgroup of 256 threads in chunks of 256, the dense block packed in
steps of 4 rows.
"""
from dataclasses import dataclass, field

import numpy as np

import append_cases as ac

TILE = 256     # kDeleteTile
SHORT = 32     # kDeleteShort
THREADS = 256  # kDeleteThreads


@dataclass
class Case:
    name: str
    m: int
    n: int
    col_starts: np.ndarray
    row_idx: np.ndarray
    vals: np.ndarray
    steps: list            # of ("delete", mask) / ("append", (row_starts, cols, vals))
    env: dict = field(default_factory=dict)


def _mask(m, rows):
    mask = np.zeros(m, bool)
    mask[list(rows)] = True
    return mask


def _case(name, m, n, col_rows, deletes, seed, **kw):
    """One delete per entry of `deletes` (row index lists, each in the
    numbering the delete meets)."""
    rng = np.random.default_rng(seed)
    starts, rows, vals = ac._csc(m, n, col_rows, rng)
    steps = []
    rows_now = m
    for d in deletes:
        steps.append(("delete", _mask(rows_now, d)))
        rows_now -= len(set(d))
    return Case(name, m, n, starts, rows, vals, steps, **kw)


def _columns_from_rows(m, n, row_cols):
    """The ascending row list of every column from the column list of every row."""
    cols = [[] for _ in range(n)]
    for r, cl in enumerate(row_cols):
        for c in cl:
            cols[c].append(r)
    return [np.asarray(c, np.int64) for c in cols]


def _build():
    cases = []
    rng = np.random.default_rng(17)

    # 5 x 7: the first row, the last, both, alternating, all but one.
    small = ac._random_columns(5, 7, 0.6, rng)
    cases.append(_case("first_row", 5, 7, small, [[0]], 1))
    cases.append(_case("last_row", 5, 7, small, [[4]], 2))
    cases.append(_case("first_and_last", 5, 7, small, [[0, 4]], 3))
    cases.append(_case("alternating", 5, 7, small, [[0, 2, 4]], 4))
    cases.append(_case("all_but_one", 5, 7, small, [[0, 1, 3, 4]], 5))

    # Columns and rows that change shape. Deleted rows: 3 (holds only its
    # slack), 8 and 11. Column 0 loses every entry (rows 8 and 11), column 1
    # none, column 2 is empty before.
    m, n = 14, 9
    cols = [np.setdiff1d(c, [3]) for c in ac._random_columns(m, n, 0.4, rng)]
    cols[0] = np.array([8, 11])
    cols[1] = np.array([0, 6, 12])
    cols[2] = np.zeros(0, np.int64)
    cases.append(_case("shapes", m, n, cols, [[3, 8, 11]], 6))

    # Full rows (every structural column): row 5 is deleted, row 6 kept.
    cols = [np.union1d(c, [5, 6]) for c in ac._random_columns(m, n, 0.3, rng)]
    cases.append(_case("full_rows", m, n, cols, [[2, 5]], 6))

    # Old columns of 31, 32, 33 and 600 entries around the switch of the
    # kernels. Column 3 holds rows 0..599: the deleted rows 255, 256 and 511,
    # 512 sit at those positions, on both sides of its chunks' borders, so
    # that a chunk's running base is used. Column 4 holds rows 600..899 (one
    # chunk and a rest): rows 600..855, its first chunk, all go.
    m = 900
    lengths = [31, 32, 33]
    cols = [np.sort(rng.choice(m, size=length, replace=False)) for length in lengths]
    cols += [np.arange(600), np.arange(600, 900), np.zeros(0, np.int64), np.array([255, 512])]
    cases.append(_case("column_lengths", m, len(cols), cols,
                       [[255, 256, 511, 512] + list(range(600, 856))], 7))

    # The same lengths for the CSR move: rows of 30, 31, 32 and 599 structural
    # entries (31, 32, 33 and 600 with the slack), a deleted long row and a
    # deleted short one between them.
    n = 640
    row_cols = [np.sort(rng.choice(n, size=length, replace=False))
                for length in (30, 5, 31, 32, 599, 400, 0, 599, 2)]
    cases.append(_case("row_lengths", len(row_cols), n, _columns_from_rows(len(row_cols), n, row_cols),
                       [[1, 5]], 8))

    # m = 257 and m = 513: deletes in the first tile only, so that the later
    # tiles must pick up its offset.
    for m in (TILE + 1, 2 * TILE + 1):
        cases.append(_case(f"rows_{m}", m, 11, ac._random_columns(m, 11, 0.1, rng),
                           [[0, 7, 200]], 9))

    # m and n just above 256 x 256 with at most two entries per column: the
    # offsets scans over the row tiles and over the column tiles take a second
    # step. Deletes in the first tile, at the step's border and at the end.
    m = n = TILE * THREADS + 3
    first = rng.integers(0, m, n)
    second = rng.integers(0, m, n)
    cols = [np.unique([a, b]) if c % 3 else np.array([a]) for c, (a, b) in
            enumerate(zip(first.tolist(), second.tolist()))]
    cases.append(_case("many_tiles", m, n, cols,
                       [[1, TILE * THREADS - 1, TILE * THREADS, m - 1]], 10))

    # The dense block: columns 0..2 are full before. Column 3 misses row 2
    # only and becomes full when row 2 goes; 0..2 stay full. m' = 8 (a
    # multiple of 4) after the first delete, 7 (a tail of 3) after the second.
    m = 9
    cols = [np.arange(m)] * 3 + [np.delete(np.arange(m), 2)] + ac._random_columns(m, 5, 0.5, rng)
    cases.append(_case("dense_block_4", m, len(cols), cols, [[2]], 11,
                       env={"MILP_DENSE_BLOCK": "force"}))
    cases.append(_case("dense_block_tail", m, len(cols), cols, [[2, 6]], 12,
                       env={"MILP_DENSE_BLOCK": "force"}))

    # Sequences on one handle: two deletes; append then delete (one old row,
    # one of the new ones); delete then append of as many rows.
    cols = ac._random_columns(12, 37, 0.3, rng)
    cases.append(_case("two_deletes", 12, 37, cols, [[1, 4, 11], [0, 8]], 13))
    seq_rng = np.random.default_rng(14)
    starts, rows, vals = ac._csc(12, 37, cols, seq_rng)
    app = ac._rows(ac._random_rows(3, 37, 0.4, seq_rng, every=(0, 36)), seq_rng)
    cases.append(Case("append_then_delete", 12, 37, starts, rows, vals,
                      [("append", app), ("delete", _mask(15, [2, 13]))]))
    cases.append(Case("delete_then_append", 12, 37, starts, rows, vals,
                      [("delete", _mask(12, [0, 5, 11])), ("append", app)]))
    return cases


CASES = _build()
NAMES = [c.name for c in CASES]


def case(name):
    return CASES[NAMES.index(name)]


# ---------------------------------------------------------------------------
# The reduced A from its triplets.

def triplets(c, steps=None):
    """Triplets of the case's A after its first `steps` steps (all of them by
    default): (m, rows, cols, vals)."""
    steps = len(c.steps) if steps is None else steps
    rows = c.row_idx.astype(np.int64)
    cols = np.repeat(np.arange(c.n, dtype=np.int64), np.diff(c.col_starts))
    vals = c.vals
    m = c.m
    for kind, arg in c.steps[:steps]:
        if kind == "append":
            rs, cl, vl = arg
            k = len(rs) - 1
            rows = np.concatenate([rows, m + np.repeat(np.arange(k, dtype=np.int64), np.diff(rs))])
            cols = np.concatenate([cols, cl.astype(np.int64)])
            vals = np.concatenate([vals, vl])
            m += k
        else:
            assert len(arg) == m
            keep = ~arg[rows]
            new_row = np.cumsum(~arg) - 1
            rows, cols, vals = new_row[rows[keep]], cols[keep], vals[keep]
            m = int((~arg).sum())
    return m, rows, cols, vals


def move_shapes(c, step):
    """(columns, rows) of the delete at index `step`: bit 0 for the kernels
    with a thread per column / row, which always run, bit 1 for those with a
    workgroup each, which run if an old structural column / a kept row (its
    slack counts) has more than SHORT entries."""
    m, r, cl, _ = triplets(c, step)
    mask = c.steps[step][1]
    col_len = np.bincount(cl, minlength=c.n)
    row_len = np.bincount(r, minlength=m)[~mask] + 1
    return (1 | (2 if col_len.max(initial=0) > SHORT else 0),
            1 | (2 if row_len.max(initial=0) > SHORT else 0))


def scratch(c, steps=None):
    """(m, the dict of [A | I]) after the steps, from the triplets."""
    m, r, cl, v = triplets(c, steps)
    return m, ac.scratch(m, c.n, r, cl, v)


def reduced_csc(c, steps=None):
    """A itself after the steps, in CSC: (m, col_starts, row_idx, vals), what
    a fresh handle is created from."""
    m, r, cl, v = triplets(c, steps)
    order = np.lexsort((r, cl))
    starts = np.zeros(c.n + 1, np.int64)
    np.cumsum(np.bincount(cl, minlength=c.n), out=starts[1:])
    return m, starts, r[order].astype(np.int32), v[order]


# ---------------------------------------------------------------------------
# The device's scheme.

def _exclusive_scan_by_tiles(x, tile):
    """Count per tile, exclusive scan of the tile counts, starts per tile."""
    x = np.asarray(x, np.int64)
    tiles = (len(x) + tile - 1) // tile
    counts = np.array([x[t * tile:(t + 1) * tile].sum() for t in range(tiles)], np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64) if tiles else counts
    out = np.zeros(len(x), np.int64)
    for t in range(tiles):
        part = x[t * tile:(t + 1) * tile]
        out[t * tile:t * tile + len(part)] = offsets[t] + np.cumsum(part) - part
    return out


def compact(old, m, n, mask):
    """old: the dict of [A | I] (m rows, n structural columns). Returns the
    dict of the matrix without the rows of the boolean mask."""
    keep = ~np.asarray(mask, bool)
    kept = int(keep.sum())
    new_row = _exclusive_scan_by_tiles(keep, TILE)
    lengths = np.where(keep, np.diff(old["t_starts"]), 0)
    row_start = _exclusive_scan_by_tiles(lengths, TILE)
    total = int(lengths.sum())
    t_starts = np.zeros(kept + 1, np.int64)
    t_cols = np.full(total, -1, np.int32)
    t_vals = np.full(total, np.nan)
    for r in np.flatnonzero(keep):  # a thread or a workgroup per kept row
        b, end = old["t_starts"][r], old["t_starts"][r + 1]
        to = row_start[r]
        t_starts[new_row[r]] = to
        t_cols[to:to + end - b] = old["t_cols"][b:end]
        t_vals[to:to + end - b] = old["t_vals"][b:end]
        t_cols[to + end - b - 1] = n + new_row[r]  # the slack
    t_starts[kept] = total
    count = np.zeros(n, np.int64)
    for c in range(n):
        count[c] = keep[old["rows"][old["starts"][c]:old["starts"][c + 1]]].sum()
    structural = int(count.sum())
    starts = np.zeros(n + kept + 1, np.int64)
    starts[:n] = _exclusive_scan_by_tiles(count, TILE)
    rows = np.full(structural + kept, -1, np.int32)
    vals = np.full(structural + kept, np.nan)
    for c in range(n):  # in chunks of THREADS entries with a running base
        base = starts[c]
        b, end = old["starts"][c], old["starts"][c + 1]
        for chunk in range(b, end, THREADS):
            r = old["rows"][chunk:min(chunk + THREADS, end)]
            flags = keep[r]
            at = base + np.cumsum(flags) - flags
            rows[at[flags]] = new_row[r[flags]]
            vals[at[flags]] = old["vals"][chunk:chunk + len(r)][flags]
            base += int(flags.sum())
    for r in np.flatnonzero(keep):  # the slack columns
        to = structural + new_row[r]
        starts[n + new_row[r]] = to
        rows[to] = new_row[r]
        vals[to] = old["vals"][old["starts"][n + r]]
    starts[n + kept] = structural + kept
    return {"starts": starts, "rows": rows, "vals": vals, "t_starts": t_starts,
            "t_cols": t_cols, "t_vals": t_vals}


def compacted(c):
    """The case's [A | I] after all of its steps, the deletes by compact() and
    the appends by append_cases.merge()."""
    m, r, cl, v = triplets(c, 0)
    mat = ac.scratch(m, c.n, r, cl, v)
    for kind, arg in c.steps:
        if kind == "append":
            mat = ac.merge(mat, m, c.n, *arg)
            m += len(arg[0]) - 1
        else:
            mat = compact(mat, m, c.n, arg)
            m = int((~arg).sum())
    return m, mat
