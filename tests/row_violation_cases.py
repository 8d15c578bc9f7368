"""Inputs and the numpy reference of the row-violation tests
(DeviceLp::RowViolationsPanel and RowViolationsPanelFrom,
mi_lp_column_combinations_violations): tests/test_row_violations_ops_gpu.py,
checked without a GPU by tests/test_row_violations_ref_cpu.py.

TEST INFRASTRUCTURE ONLY. The activities are the dense references of
tests/row_panel_cases.py; the expected result is that reference filtered in
numpy with the header's rule (filter_reference).

Matrices (CASES):
  rows70, steps  of row_panel_cases, with its points, reference and override
                 sets (m = 70 and 40: less than one tile)
  tall           m = 66 000, n = 12: rows of 0 to 3 structural entries and the
                 slack. 258 tiles of 256 rows, more than one step of the
                 offsets kernel's scan, and a last tile of 208 rows
                 (satisfies_geometry). TALL_POOL = 5 points: 0 and 2 ordinary,
                 1 all +0.0, 3 with a NaN and 4 with a -inf in a structural
                 column. Its reference is vectorised here (at most 4 entries
                 per row) and compared with RefState.row_sums on a sample of
                 rows by the CPU test.

Bound sets (bounds(name, which) -> row_lb, row_ub, tolerance), built from the
reference activities of the whole pool, so the same for every k:
  split      per row the pool's quartiles: about half of the pairs violated
  free       (-inf, +inf): only NaN activities are violated
  crossed    row_lb > row_ub: every row is violated at every point
  one_sided  even rows (-inf, hi], odd rows [lo, +inf), with 0.0 inside: the
             all-zero points have no violated row
  edges0, edges_tol
             split, with the rows of edge_entries(name, which) rebuilt so that
             the activity of one point is exactly on a widened bound or one
             ulp outside it, at tolerance 0 and EDGE_TOLERANCE.
"""
import functools

import numpy as np

import panel_cases as pc
import row_panel_cases as rc
import solveops_cases as sc
from device_ref import Matrix, bits

CASES = ("rows70", "steps", "tall")
BOUND_SETS = ("split", "free", "crossed", "one_sided", "edges0", "edges_tol")
EDGE_KINDS = ("at_lo", "below_lo", "at_hi", "above_hi")
EDGE_TOLERANCE = 0.375
EDGE_POINTS = rc.ALONE  # 0 is in the first panel of every k; 16 and 32 end k = 17 and 33
TILE_ROWS = 256          # kPanelTileColumns of kernels/kernel_args.h
OFFSETS_STEP_TILES = 256  # kPanelOffsetsStep
TALL_M, TALL_N, TALL_POOL = 66000, 12, 5
TALL_SEED = 810000
TALL_KS = (1, 4, 5)
TALL_ZERO, TALL_NAN, TALL_INF = 1, 3, 4
TALL_NAN_COL, TALL_INF_COL = 0, TALL_N - 1
INF = np.inf

SUMMARY = np.dtype([("count", np.int64), ("worst", np.float64), ("worst_row", np.int32),
                    ("reserved", np.int32)])  # mi_lp_point_violations


def satisfies_geometry(m, tile_rows, offsets_step_tiles):
    """What `tall` is for: more than one step of the offsets kernel's scan
    and a partial last tile of more than one row."""
    return m > tile_rows * offsets_step_tiles and m % tile_rows not in (0, 1)


assert satisfies_geometry(TALL_M, TILE_ROWS, OFFSETS_STEP_TILES)
assert -(-TALL_M // TILE_ROWS) == 258 and TALL_M % TILE_ROWS == 208


def ks(name):
    return TALL_KS if name == "tall" else rc.KS


def pool(name):
    return TALL_POOL if name == "tall" else rc.POOL


@functools.lru_cache(maxsize=None)
def _tall_rows():
    """(cols (m, 3) ascending with TALL_N as padding, vals (m, 3), lengths)."""
    rng = np.random.default_rng(TALL_SEED)
    lens = rng.integers(0, 4, TALL_M)
    order = np.argsort(rng.random((TALL_M, TALL_N)), axis=1)[:, :3]
    used = np.arange(3)[None, :] < lens[:, None]
    cols = np.sort(np.where(used, order, TALL_N), axis=1).astype(np.int32)
    vals = pc._values(rng, TALL_M * 3).reshape(TALL_M, 3)
    return cols, vals, lens


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name != "tall":
        return rc.matrix(name)
    cols, vals, lens = _tall_rows()
    mat = Matrix(TALL_M, TALL_N, [(cols[r, :lens[r]], vals[r, :lens[r]]) for r in range(TALL_M)])
    assert set(mat.row_len) == {1, 2, 3, 4}
    return mat


@functools.lru_cache(maxsize=None)
def points(name):
    """(pool, N), read-only."""
    if name != "tall":
        return rc.points(name)
    N = TALL_M + TALL_N
    x = np.stack([sc._family(np.random.default_rng(TALL_SEED + 1000 * (j + 1)), N)
                  for j in range(TALL_POOL)])
    x[TALL_ZERO] = 0.0
    x[TALL_NAN, TALL_NAN_COL] = np.nan
    x[TALL_INF, TALL_INF_COL] = -np.inf
    x.setflags(write=False)
    return x


def tall_row_sums(x):
    """RefState.row_sums(x, None, 1.0) of `tall` for all rows at once: from
    +0.0, the structural entries in increasing column order, then the slack.
    A skipped or padding term is added as -0.0, which leaves every sum's bits
    as they are."""
    cols, vals, _ = _tall_rows()
    x = np.asarray(x, np.float64)
    xs = np.concatenate([x[:TALL_N], [0.0]])  # the padding column multiplies by 0.0
    acc = np.zeros(TALL_M)
    with np.errstate(invalid="ignore"):
        for e in range(3):
            mult = xs[cols[:, e]]
            acc = acc + np.where(mult != 0.0, mult * vals[:, e], -0.0)
        slack = x[TALL_N:]
        acc = acc + np.where(slack != 0.0, slack * 1.0, -0.0)
    return acc


@functools.lru_cache(maxsize=None)
def reference(name):
    """(pool, m), read-only: the dense activities."""
    if name != "tall":
        return rc.reference(name)
    out = np.stack([tall_row_sums(x) for x in points(name)])
    assert sc.only_input_nans(out)
    out.setflags(write=False)
    return out


# --- the rule -----------------------------------------------------------------------------------

def violated(acts, lb, ub, tol):
    """The header's keep rule, elementwise over (k, m)."""
    return ~(acts >= lb - tol) | ~(acts <= ub + tol)


def amounts(acts, lb, ub):
    """+inf for a NaN activity, else the larger of lb - a and a - ub (either
    may be NaN where the row is not violated; see filter_reference)."""
    with np.errstate(invalid="ignore"):
        below, above = lb - acts, acts - ub
        return below, above, np.where(np.isnan(acts), INF, np.maximum(below, above))


def filter_reference(acts, lb, ub, tol):
    """row_starts (k + 1, int64), rows (int32), activities and the summaries
    (SUMMARY) of the dense activities acts (k, m) under the header's rule."""
    acts = np.asarray(acts, np.float64)
    k, m = acts.shape
    lb, ub = np.asarray(lb, np.float64), np.asarray(ub, np.float64)
    assert lb.shape == ub.shape == (m,) and tol >= 0.0 and np.isfinite(tol)
    assert not np.isnan(lb).any() and not np.isnan(ub).any()
    assert not (lb == INF).any() and not (ub == -INF).any()
    keep = violated(acts, lb, ub, tol)
    below, above, amount = amounts(acts, lb, ub)
    real = keep & ~np.isnan(acts)
    assert not np.isnan(below[real]).any() and not np.isnan(above[real]).any()
    assert np.all(amount[keep] > 0.0)
    row_starts = np.zeros(k + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=row_starts[1:])
    point, row = np.nonzero(keep)  # point-major, rows ascending
    summaries = np.zeros(k, SUMMARY)
    summaries["count"] = keep.sum(axis=1)
    summaries["worst_row"] = -1
    for j in np.nonzero(summaries["count"])[0]:
        masked = np.where(keep[j], amount[j], -1.0)
        summaries["worst_row"][j] = np.argmax(masked)  # the first, so the lowest row
        summaries["worst"][j] = masked.max()
    return row_starts, row.astype(np.int32), acts[point, row], summaries


# --- bound sets ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sorted_finite(name):
    """Per row the pool's finite activities ascending (NaN behind them), and
    how many there are."""
    acts = reference(name)
    finite = np.isfinite(acts)
    assert finite.sum(axis=0).min() >= 2
    return np.sort(np.where(finite, acts, np.nan), axis=0), finite.sum(axis=0)


def _quantiles(name, q):
    """Per row the q-quantile (linear between neighbours) of the pool's finite
    activities; a fresh array."""
    s, n = _sorted_finite(name)
    pos = q * (n - 1)
    below = np.floor(pos).astype(np.int64)
    above = np.minimum(below + 1, n - 1)
    row = np.arange(s.shape[1])
    out = s[below, row] + (s[above, row] - s[below, row]) * (pos - below)
    assert np.isfinite(out).all()
    return out


def _exact(kind, a, tol):
    """(lb, ub) that put the activity a on the widened bound (at_*) or one ulp
    outside it (below_lo, above_hi), or None when rounding does not let
    lb - tol or ub + tol land there."""
    if kind in ("at_lo", "below_lo"):
        target = a if kind == "at_lo" else np.nextafter(a, INF)
        lb = target + tol
        return (lb, INF) if lb - tol == target and np.isfinite(lb) else None
    target = a if kind == "at_hi" else np.nextafter(a, -INF)
    ub = target - tol
    return (-INF, ub) if ub + tol == target and np.isfinite(ub) else None


@functools.lru_cache(maxsize=None)
def _edges(name, tol):
    acts = reference(name)
    lb, ub = _quantiles(name, 0.25), _quantiles(name, 0.75)
    used = set()
    entries = []
    for p in (p for p in EDGE_POINTS if p < pool(name)):
        for kind in EDGE_KINDS:
            for r in range(acts.shape[1]):
                a = acts[p, r]
                pair = _exact(kind, a, tol) if np.isfinite(a) and a != 0.0 else None
                if r not in used and pair is not None:
                    lb[r], ub[r] = pair
                    used.add(r)
                    entries.append((p, r, kind))
                    break
            else:
                raise AssertionError((name, tol, p, kind))
    return lb, ub, tuple(entries)


def edge_entries(name, which):
    """((point, row, kind), ...) of edges0 / edges_tol."""
    return _edges(name, {"edges0": 0.0, "edges_tol": EDGE_TOLERANCE}[which])[2]


@functools.lru_cache(maxsize=None)
def bounds(name, which):
    """(row_lb, row_ub, tolerance), read-only."""
    m = matrix(name).m
    tol = 0.0
    if which == "split":
        lb, ub = _quantiles(name, 0.25), _quantiles(name, 0.75)
    elif which == "free":
        lb, ub = np.full(m, -INF), np.full(m, INF)
    elif which == "crossed":
        med = _quantiles(name, 0.5)
        lb, ub = med + (np.abs(med) + 1.0), med - (np.abs(med) + 1.0)
        assert np.all(lb > ub)
    elif which == "one_sided":
        even = np.arange(m) % 2 == 0
        lb = np.where(even, -INF, np.minimum(_quantiles(name, 0.4), 0.0))
        ub = np.where(even, np.maximum(_quantiles(name, 0.6), 0.0), INF)
    else:
        tol = {"edges0": 0.0, "edges_tol": EDGE_TOLERANCE}[which]
        lb, ub, _ = _edges(name, tol)
        lb, ub = lb.copy(), ub.copy()
    lb.setflags(write=False)
    ub.setflags(write=False)
    return lb, ub, tol


@functools.lru_cache(maxsize=None)
def expected(name, which, k):
    """filter_reference of the first k points under a bound set."""
    out = filter_reference(reference(name)[:k], *bounds(name, which))
    for a in out:
        a.setflags(write=False)
    return out


def same_summaries(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == SUMMARY and got.shape == want.shape, (what, got.shape)
    for field in SUMMARY.names:
        g, w = got[field], want[field]
        same = bits(g) == bits(w) if field == "worst" else g == w
        assert np.all(same), (what, field, got[~same][:3], want[~same][:3])


def same_result(got, want, what):
    """row_starts, rows, activities and summaries, every one on all its bits."""
    for g, w, part in zip(got[:3], want[:3], ("row_starts", "rows", "activities")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.dtype, g.shape, w.shape)
        if part == "activities":
            bad = np.nonzero(bits(g) != bits(w))[0]
            assert len(bad) == 0, (what, part, len(bad), int(bad[0]))
        else:
            assert np.array_equal(g, w), (what, part, g[:8], w[:8])
    same_summaries(got[3], want[3], what)
