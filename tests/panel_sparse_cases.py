"""Inputs of the sparse panel tests (DeviceLp::ColumnDotsPanelSparse): the
matrices, vectors and references of tests/panel_cases.py for quad, wave,
dense13 and dense23, two more matrices, and per case the column masks and drop
tolerances the tests run.

TEST INFRASTRUCTURE ONLY. The expected result is always the dense reference
(tests/device_ref.py column_scalar_products) filtered in numpy:
keep = mask & (|ref| > tolerance), columns ascending per row.

  edge   m = 37, n = 100: N = 137 is no multiple of 64 and is less than one
         tile of the sparse-row kernels. Column lengths cycle through
         panel_cases.QUAD_LENS capped at m.
  long   m = 24, column lengths cycle through LONG_LENS, n = 70 000: N =
         70 024 needs 274 tiles of TILE_COLUMNS columns, more than one step of
         OFFSETS_STEP_TILES tiles of the offsets kernel; N mod TILE_COLUMNS =
         136 and N mod 64 = 8. At most LONG_MAX_K vectors, so that the
         reference stays quick.

dense13 and dense23 use a subset of panel_cases.vectors, DENSE_VECTORS,
repeated in turn up to 33 vectors: nearly every column of those matrices is
full, so the size of a whole row follows the few largest entries of its
vector, and only some of the 33 vectors have rows that one tolerance per call
splits near the middle; with m = 13 or 23, a quarter of them also have no
zero entry, hence no +-0.0 slack dot to drop at tolerance 0.
tests/test_panel_sparse_ref_cpu.py states the conditions every vector that
is used has to meet; DENSE_VECTORS lists the vectors that meet them.

TILE_COLUMNS and OFFSETS_STEP_TILES are the kernels' constants this module
ASSUMES (kernels/kernel_args.h kPanelTileColumns, kPanelOffsetsStep); the GPU
test compares them with the probe's panel_sparse_geometry.
"""
import functools

import numpy as np

import panel_cases as pc
from device_ref import Matrix, column_scalar_products

TILE_COLUMNS = 256
OFFSETS_STEP_TILES = 256

LONG_LENS = (0, 1, 2, 3, 5)
LONG_MAX_K = 5

# name -> (m, n, environment, vectors)
CASES = {name: pc.CASES[name] + (pc.MAX_K,) for name in ("quad", "wave", "dense13", "dense23")}
CASES["edge"] = (37, 100, {}, pc.MAX_K)
CASES["long"] = (24, 70000, {}, LONG_MAX_K)
OWN = ("edge", "long")
# Rows of panel_cases.vectors that the dense cases use, repeated in turn.
DENSE_VECTORS = {"dense13": (15, 23, 24, 27, 29),
                 "dense23": (0, 1, 2, 5, 6, 7, 9, 11, 12, 13, 14, 16, 17, 21, 22, 23, 25, 26, 27,
                             28, 29, 32)}

MASKS = ("all", "structural", "random", "none", "last", "first")
TOLERANCES = ("zero", "median", "tstar", "below_tstar", "inf")


def satisfies_geometry(N, tile_columns, offsets_step_tiles):
    """What `long` is for: more than one step of the offsets loop, a partial
    last tile of more than one column, a partial last mask word."""
    return (N > tile_columns * offsets_step_tiles and N % tile_columns not in (0, 1)
            and N % 64 != 0)


assert satisfies_geometry(CASES["long"][0] + CASES["long"][1], TILE_COLUMNS, OFFSETS_STEP_TILES)


def column_lengths(name):
    m, n = CASES[name][:2]
    if name == "edge":
        return [min(m, pc.QUAD_LENS[c % len(pc.QUAD_LENS)]) for c in range(n)]
    if name == "long":
        return [LONG_LENS[c % len(LONG_LENS)] for c in range(n)]
    return pc.column_lengths(name)


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name not in OWN:
        return pc.matrix(name)
    m, n = CASES[name][:2]
    rng = np.random.default_rng(3000 + OWN.index(name))
    lens = np.array(column_lengths(name))
    # Column c takes the rows of the lens[c] smallest of m random keys.
    order = np.argsort(rng.random((n, m)), axis=1)
    taken = np.arange(m)[None, :] < lens[:, None]
    col = np.repeat(np.arange(n), lens)
    row = order[taken]
    val = pc._values(rng, len(row))
    by_row = np.lexsort((col, row))
    col, row, val = col[by_row], row[by_row], val[by_row]
    cut = np.searchsorted(row, np.arange(m + 1))
    mat = Matrix(m, n, [(col[cut[r]:cut[r + 1]].astype(np.int32), val[cut[r]:cut[r + 1]])
                        for r in range(m)])
    assert np.array_equal(np.diff(mat.col_starts), lens)
    return mat


def _dense_rows(name):
    rows = DENSE_VECTORS[name]
    return np.array([rows[i % len(rows)] for i in range(CASES[name][3])])


@functools.lru_cache(maxsize=None)
def vectors(name):
    """(CASES[name][3], m), read-only; panel_cases' recipe."""
    if name in DENSE_VECTORS:
        y = pc.vectors(name)[_dense_rows(name)]
        y.setflags(write=False)
        return y
    if name not in OWN:
        return pc.vectors(name)
    m, k = CASES[name][0], CASES[name][3]
    rng = np.random.default_rng(4000 + OWN.index(name))
    y = pc._values(rng, k * m)
    kind = rng.random(k * m)
    y[kind < 0.10] = 0.0
    y[(kind >= 0.10) & (kind < 0.12)] = -0.0
    y = y.reshape(k, m)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def reference(name):
    """(CASES[name][3], N) dense reference, computed once and read-only."""
    if name in DENSE_VECTORS:
        out = pc.reference(name)[_dense_rows(name)]
        out.setflags(write=False)
        return out
    if name not in OWN:
        return pc.reference(name)
    mat = matrix(name)
    cols = np.arange(mat.N)
    out = np.stack([column_scalar_products(mat, cols, y) for y in vectors(name)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mask(name, which):
    """bool[N], read-only."""
    mat = matrix(name)
    b = np.zeros(mat.N, bool)
    if which == "all":
        b[:] = True
    elif which == "structural":
        b[:mat.n] = True
    elif which == "random":
        rng = np.random.default_rng(5000 + sorted(CASES).index(name))
        b[:] = rng.random(mat.N) < 0.5
    elif which == "last":
        b[mat.N - 1] = True
    elif which == "first":
        b[0] = True
    else:
        assert which == "none"
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def anchor(name, which):
    """(j0, c0): the fixed masked non-zero entry behind the tstar tolerances,
    the first one of vector 0 (None when the mask keeps no such entry)."""
    hit = np.nonzero(mask(name, which) & (reference(name)[0] != 0.0))[0]
    return (0, int(hit[0])) if len(hit) else None


@functools.lru_cache(maxsize=None)
def tolerances(name, which):
    """dict tolerance name -> value under mask `which`, derived from the
    reference of all the case's vectors and used for every k: 0, the median
    of |ref| over the masked entries, t* = |ref[j0, c0]| (drops that entry),
    nextafter(t*, 0) (keeps it) and +inf. Masks without entries or without a
    non-zero entry of vector 0 leave median / tstar out."""
    ref = np.abs(reference(name))
    b = mask(name, which)
    tol = {"zero": 0.0, "inf": float("inf")}
    if b.any():
        tol["median"] = float(np.median(ref[:, b]))
    a = anchor(name, which)
    if a is not None:
        tol["tstar"] = float(ref[a])
        tol["below_tstar"] = float(np.nextafter(ref[a], 0.0))
    return tol


def filtered(ref, keep_columns, tolerance):
    """(row_starts int64[k+1], cols int32, vals float64) of the numpy filter."""
    with np.errstate(invalid="ignore"):
        keep = np.asarray(keep_columns, bool)[None, :] & (np.abs(ref) > tolerance)
    starts = np.zeros(len(ref) + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=starts[1:])
    rows = [np.nonzero(keep[j])[0] for j in range(len(ref))]
    cols = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
    vals = (np.concatenate([ref[j][rows[j]] for j in range(len(ref))])
            if rows else np.zeros(0))
    return starts, cols, vals
