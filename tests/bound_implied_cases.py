"""Inputs and the numpy reference of the implied-column-bound tests
(DeviceLp::BoundImpliedPanel(From) and BoundTightenedPanel(From),
mi_lp_bound_implied_bounds, mi_lp_bound_tightened_columns):
tests/test_bound_implied_ops_gpu.py and tests/test_bound_implied_gpu.py,
checked without a GPU by tests/test_bound_implied_ref_cpu.py.

TEST INFRASTRUCTURE ONLY. implied() restates the rule of include/mi_lp.h in
numpy, one rounded operation at a time (a product, a difference, a
difference, a quotient, + 0.0; numpy does not fuse), for all children of a
column at once, and folds the candidates one entry after the other in the
order asked for. implied_scalar() is the same rule in plain Python floats, a
literal copy of the header's loop, for the CPU test. keep_reference() restates
the keep rule and the summaries.

Matrices (CASES): rows70, steps and groups of bound_range_cases (column
lengths 6 to 21, 11 to 19 and 11 to 24: around one and two unroll groups of 8;
n = 230, 30, 30: a partial last workgroup at 256, 64 and 16 columns per
workgroup) and
  wide    of this file: m = 320, n = 700 (two full filter tiles of 256 columns
          and a partial one). The first 300 columns cycle through WIDE_LENS:
          0, 1, 7, 8, 9 (the unroll group), 15, 16, 17, 63, 64, 65, 255, 256,
          257 (one below, at and one above a slice round of the long shape at
          K = 16, 4 and 1) and 320 (the full column); the others hold 2 to 9
          entries. Structural entries per column are above 32, so `wide` takes
          the long shape by itself and the other three the short one.
Its pool is built as bound_range_cases builds the small matrices' pools.

Row-bound sets (row_bounds(name, which) -> row_lb, row_ub): `mid`, built from
the pool's reference ranges (so the same for every k), and bound_range_cases'
`free` and `crossed`, which have no finite bound and yield no candidate:
children 3, 6 and 7 still exercise a NaN own bound, l = +inf > u kept as
crossing with worst = +inf, and +-2^1023.
  mid   for row r, ok = the ordinary children with both counts 0 and finite lo
        and hi. Rows with r % 4 == 3 or an empty ok stay free. Otherwise w =
        median(hi - lo over ok); r % 4 in {0, 2}: ub = median(lo[ok]) + 0.5 w;
        r % 4 in {1, 2}: lb = median(hi[ok]) - 0.5 w.
Tolerances: 0.0, 0.375, and per matrix an edge pair (edge(name)): one actual
movement nl - l of child 0, at which that column is not kept, and the double
below it, at which it is.
"""
import functools

import numpy as np

import bound_range_cases as bc
import panel_cases as pc
from device_ref import Matrix, bits

CASES = bc.CASES + ("wide",)
KS = bc.KS
POOL = bc.POOL
WIDE_M, WIDE_N = 320, 700
WIDE_LENS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 320)
WIDE_CYCLED = 300  # columns that cycle through WIDE_LENS
WIDE_SEED = 8001
WIDE_POOL_SEED = 950000
ROW_BOUND_SETS = ("mid", "free", "crossed")
TOLERANCES = (0.0, 0.375)
LONG_COLUMNS_FROM = 32.0  # structural entries per column: the engine's rule
INF = np.inf
SUMMARY = bc.SUMMARY


def wide_lengths():
    rng = np.random.default_rng(WIDE_SEED + 1)
    return [WIDE_LENS[c % len(WIDE_LENS)] if c < WIDE_CYCLED else int(rng.integers(2, 10))
            for c in range(WIDE_N)]


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name != "wide":
        return bc.matrix(name)
    rng = np.random.default_rng(WIDE_SEED)
    per_row = [([], []) for _ in range(WIDE_M)]
    for c, length in enumerate(wide_lengths()):
        rows = np.sort(rng.choice(WIDE_M, length, replace=False))
        for r, x in zip(rows, pc._values(rng, length)):
            per_row[r][0].append(c)
            per_row[r][1].append(x)
    mat = Matrix(WIDE_M, WIDE_N, per_row)
    assert np.array_equal(np.diff(mat.col_starts), wide_lengths())
    return mat


def column_lengths(name):
    return np.diff(matrix(name).col_starts)


def long_by_itself(name):
    """Whether the engine's rule takes the long shape for this matrix."""
    mat = matrix(name)
    return int(mat.col_starts[-1]) / mat.n >= LONG_COLUMNS_FROM


@functools.lru_cache(maxsize=None)
def pool(name):
    """(L, U), each (POOL, n), read-only: bound_range_cases.pool, and for
    `wide` the same construction."""
    if name != "wide":
        return bc.pool(name)
    mat = matrix(name)
    pairs = [bc._ordinary(WIDE_POOL_SEED + 1000 * (j + 1), mat.n) for j in range(POOL)]
    L = np.stack([p[0] for p in pairs])
    U = np.stack([p[1] for p in pairs])
    held = bc.most_held(mat)
    rng = np.random.default_rng(WIDE_POOL_SEED + 77)
    for j in range(POOL):
        for c in rng.permutation(held)[:j % 4]:
            if rng.random() < 0.5:
                L[j, c] = -INF
            else:
                U[j, c] = INF
    L[bc.BOX], U[bc.BOX] = bc._ordinary(WIDE_POOL_SEED + 1000 * (bc.BOX + 1), mat.n)
    U[bc.BOX] = L[bc.BOX]
    L[bc.WITH_NAN, held[0]] = np.nan
    L[bc.WRONG_INF, held[0]] = INF
    for i, c in enumerate(held):
        L[bc.HUGE, c], U[bc.HUGE, c] = ((-bc.HUGE_BOUND, bc.HUGE_BOUND) if i % 2 == 0 else
                                        (bc.HUGE_BOUND, bc.HUGE_BOUND))
    L.setflags(write=False)
    U.setflags(write=False)
    return L, U


@functools.lru_cache(maxsize=None)
def ranges_reference(name):
    """bound_range_cases.ranges of the whole pool, computed once, read-only."""
    if name != "wide":
        return bc.reference(name)
    out = bc.ranges(matrix(name), *pool(name))
    for a in out:
        a.setflags(write=False)
    return out


# --- row bounds -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def row_bounds(name, which):
    """(row_lb, row_ub), read-only."""
    m = matrix(name).m
    if which == "free":
        lb, ub = np.full(m, -INF), np.full(m, INF)
    elif which == "crossed":
        lb, ub = np.full(m, INF), np.full(m, -INF)
    else:
        assert which == "mid"
        lo, hi, lo_inf, hi_inf = ranges_reference(name)
        pick = np.array(bc.ordinary(name))
        lb, ub = np.full(m, -INF), np.full(m, INF)
        for r in range(m):
            ok = pick[(lo_inf[pick, r] == 0) & (hi_inf[pick, r] == 0) &
                      np.isfinite(lo[pick, r]) & np.isfinite(hi[pick, r])]
            if r % 4 == 3 or len(ok) == 0:
                continue
            w = np.median(hi[ok, r] - lo[ok, r])
            if r % 4 in (0, 2):
                ub[r] = np.median(lo[ok, r]) + 0.5 * w
            if r % 4 in (1, 2):
                lb[r] = np.median(hi[ok, r]) - 0.5 * w
    lb.setflags(write=False)
    ub.setflags(write=False)
    return lb, ub


# --- the rule -------------------------------------------------------------------------------------

def _column_order(order, c, length):
    if order is None:
        return np.arange(length)
    if order == "reversed":
        return np.arange(length)[::-1]
    return np.random.default_rng((int(order), c)).permutation(length)


def implied(mat, L, U, ref, rlb, rub, order=None, normalise=True, stats=None):
    """(new_lbs, new_ubs), each (k, n), of the bound sets L, U (k, n) whose
    activity ranges are ref = (lo, hi, lo_inf, hi_inf), each (k, m). order:
    None walks a column's entries as stored, "reversed" backwards, an integer
    seed in a random permutation of its own per column. normalise=False leaves
    the q + 0.0 step out (for the CPU test). stats: a Counter that receives
    how often each branch of the rule was taken."""
    L, U = np.asarray(L, np.float64), np.asarray(U, np.float64)
    lo, hi, lo_inf, hi_inf = ref
    rlb, rub = np.asarray(rlb, np.float64), np.asarray(rub, np.float64)
    NL, NU = L.copy(), U.copy()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        for c in range(mat.n):
            s, e = int(mat.col_starts[c]), int(mat.col_starts[c + 1])
            walk = s + _column_order(order, c, e - s)
            rows, a = mat.row_idx[walk], mat.vals[walk][:, None]
            live = (a != 0.0) & ~np.isnan(a)
            up = a > 0.0
            l, u = L[:, c][None, :], U[:, c][None, :]
            bl, bh = np.where(up, l, u), np.where(up, u, l)  # what c fed into lo / hi

            def side(rb, total, count, b):
                rb = rb[:, None]
                none = count == 0
                own = (count == 1) & np.isinf(b)  # c itself is the one infinite term
                product = a * b
                res = np.where(none, total - product, total)
                q = (rb - res) / a
                open_side = live & np.isfinite(rb)
                ok = open_side & (none | own) & np.isfinite(q)
                if stats is not None:
                    stats["own_infinite"] += int((ok & own).sum())
                    stats["non_finite_q"] += int((open_side & (none | own) & ~np.isfinite(q)).sum())
                    stats["other_infinite"] += int((open_side & ~(none | own)).sum())
                if normalise:
                    q = q + 0.0  # -0.0 becomes +0.0
                return q, ok

            q_lo, ok_lo = side(rub[rows], lo[:, rows].T, lo_inf[:, rows].T, bl)
            q_hi, ok_hi = side(rlb[rows], hi[:, rows].T, hi_inf[:, rows].T, bh)
            for_upper, upper_ok = np.where(up, q_lo, q_hi), np.where(up, ok_lo, ok_hi)
            for_lower, lower_ok = np.where(up, q_hi, q_lo), np.where(up, ok_hi, ok_lo)
            nl, nu = L[:, c].copy(), U[:, c].copy()
            for i in range(e - s):  # the fold, one entry after the other
                nu = np.where(upper_ok[i] & (for_upper[i] < nu), for_upper[i], nu)
                nl = np.where(lower_ok[i] & (for_lower[i] > nl), for_lower[i], nl)
            NL[:, c], NU[:, c] = nl, nu
    if stats is not None:
        stats["lower_from_infinite"] += int((np.isinf(L) & np.isfinite(NL)).sum())
        stats["upper_from_infinite"] += int((np.isinf(U) & np.isfinite(NU)).sum())
    return NL, NU


def implied_scalar(mat, l, u, ref_j, rlb, rub, c, normalise=True, candidates=None):
    """(nl, nu) of column c under one bound set (l, u: n values) with ranges
    ref_j = (lo, hi, lo_inf, hi_inf), m values each: the header's loop in
    Python floats. candidates: a list that receives, per candidate, (row, a,
    rb, s, cnt, b, q, tightens_upper)."""
    nl, nu = float(l[c]), float(u[c])
    lo, hi, lo_inf, hi_inf = ref_j
    for i in range(int(mat.col_starts[c]), int(mat.col_starts[c + 1])):
        r, a = int(mat.row_idx[i]), float(mat.vals[i])
        if a == 0.0 or a != a:
            continue
        up = a > 0.0
        bl, bh = (float(l[c]), float(u[c])) if up else (float(u[c]), float(l[c]))
        for rb, s, cnt, b, tightens_upper in ((float(rub[r]), float(lo[r]), int(lo_inf[r]), bl, up),
                                              (float(rlb[r]), float(hi[r]), int(hi_inf[r]), bh,
                                               not up)):
            if not np.isfinite(rb):
                continue
            if cnt == 0:
                res = s - a * b
            elif cnt == 1 and np.isinf(b):
                res = s
            else:
                continue
            q = (rb - res) / a
            if not np.isfinite(q):
                continue
            if normalise:
                q = q + 0.0
            if candidates is not None:
                candidates.append((r, a, rb, s, cnt, b, q, tightens_upper))
            if tightens_upper:
                if q < nu:
                    nu = q
            elif q > nl:
                nl = q
    return nl, nu


def keep_reference(L, U, NL, NU, tol, base=None):
    """(col_starts (k + 1, int64), cols (int32), new_lbs, new_ubs, summaries
    (SUMMARY)) of the header's keep rule. base = (base_lb, base_ub): the
    override form, which also keeps the columns whose own bounds differ in
    bits from the base."""
    assert tol >= 0.0 and np.isfinite(tol)
    with np.errstate(invalid="ignore", over="ignore"):
        moved = (NL - L > tol) | (U - NU > tol)  # inf - inf is NaN and does not count
        cross = NL - NU
        crossing = cross > tol
    keep = moved | crossing
    if base is not None:
        keep = keep | (bits(L) != bits(base[0])[None, :]) | (bits(U) != bits(base[1])[None, :])
    k = L.shape[0]
    col_starts = np.zeros(k + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=col_starts[1:])
    child, col = np.nonzero(keep)  # child-major, columns ascending
    summaries = np.zeros(k, SUMMARY)
    summaries["count"] = keep.sum(axis=1)
    summaries["worst_row"] = -1
    for j in np.nonzero(crossing.any(axis=1))[0]:
        masked = np.where(crossing[j], cross[j], -INF)
        summaries["worst_row"][j] = np.argmax(masked)  # the first, so the lowest column
        summaries["worst"][j] = masked.max()
    return col_starts, col.astype(np.int32), NL[child, col], NU[child, col], summaries


@functools.lru_cache(maxsize=None)
def reference(name, which):
    """implied() of the whole pool under a row-bound set, computed once,
    read-only."""
    out = implied(matrix(name), *pool(name), ranges_reference(name), *row_bounds(name, which))
    for a in out:
        a.setflags(write=False)
    return out


def first(pair, k):
    return tuple(a[:k] for a in pair)


@functools.lru_cache(maxsize=None)
def expected(name, which, k, tol):
    """keep_reference of the first k children, dense form."""
    L, U = pool(name)
    out = keep_reference(L[:k], U[:k], *first(reference(name, which), k), tol)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def edge(name):
    """(tol, col): a movement nl - l of child 0 under `mid` that is the only
    reason to keep that column: at tolerance tol the column is not kept, at
    nextafter(tol, 0) it is."""
    L, U = pool(name)
    NL, NU = reference(name, "mid")
    with np.errstate(invalid="ignore"):
        d = NL[0] - L[0]
        other = U[0] - NU[0]
        cross = NL[0] - NU[0]
    for c in np.argsort(-np.where(np.isfinite(d), d, -INF), kind="stable"):
        if np.isfinite(d[c]) and d[c] > 0.0 and not other[c] > np.nextafter(d[c], 0.0) and \
                not cross[c] > np.nextafter(d[c], 0.0):
            return float(d[c]), int(c)
    raise AssertionError(f"{name}: no column of child 0 moves its lower bound alone")


def tolerances(name):
    tol, _ = edge(name)
    return TOLERANCES + (tol, float(np.nextafter(tol, 0.0)))


# --- overrides ------------------------------------------------------------------------------------

def pool_as_overrides(name, k):
    """bound_range_cases.pool_as_overrides, for `wide` too."""
    L, U = pool(name)
    sets = []
    for j in range(k):
        cols = np.nonzero((bits(L[j]) != bits(L[0])) | (bits(U[j]) != bits(U[0])))[0]
        cols = cols.astype(np.int32)
        sets.append((cols, L[j, cols], U[j, cols]))
    return L[0], U[0], sets


def override_bytes(name, sets):
    return 16 * matrix(name).n + 20 * sum(len(c) for c, _, _ in sets) + 8 * (len(sets) + 1)


@functools.lru_cache(maxsize=None)
def override_reference(name, which, bounds="mid"):
    """(L, U, NL, NU) of bound_range_cases.override_set(name, which),
    materialised, under a row-bound set."""
    base_lb, base_ub, sets = bc.override_set(name, which)
    L, U = bc.materialise(base_lb, base_ub, sets)
    NL, NU = implied(matrix(name), L, U, bc.override_reference(name, which),
                     *row_bounds(name, bounds))
    for a in (L, U, NL, NU):
        a.setflags(write=False)
    return L, U, NL, NU


# --- comparisons ----------------------------------------------------------------------------------

def same_bounds(got, want, what):
    """new_lbs and new_ubs on all 64 bits, NaNs included."""
    for g, w, part in zip(got, want, ("new_lbs", "new_ubs")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, part, g.shape, w.shape)
        bad = np.argwhere(bits(g) != bits(w))
        assert len(bad) == 0, (what, part, len(bad), bad[:3].tolist())


def same_lists(got, want, what):
    """(col_starts, cols, new_lbs, new_ubs, summaries) of a filtered call."""
    for g, w, part in zip(got[:4], want[:4], ("col_starts", "cols", "new_lbs", "new_ubs")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, part, g.shape, w.shape)
        if part.startswith("new"):
            assert np.array_equal(bits(g), bits(w)), (what, part)
        else:
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, part)
    bc.same_summaries(got[4], want[4], what)
