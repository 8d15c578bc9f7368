"""Inputs and the numpy reference of the bound-set activity-range tests
(DeviceLp::BoundRangesPanel(From) and BoundInfeasiblePanel(From),
mi_lp_bound_activity_ranges, mi_lp_bound_infeasible_rows):
tests/test_bound_ranges_ops_gpu.py and tests/test_bound_ranges_gpu.py, checked
without a GPU by tests/test_bound_ranges_ref_cpu.py.

TEST INFRASTRUCTURE ONLY. ranges() restates the rule of include/mi_lp.h in
numpy, one rounded product and one rounded sum at a time (numpy does not
fuse); screen() and filter_reference() restate the screening.

Matrices (CASES); bound sets are over the n structural columns, and the slack
entry that closes every CSR row is no part of a range:
  rows70  of solveops_cases: m = 70, structural lengths 0, 1, 2, 62, 63, 64,
          127, 128, 129 and 199; a partial last workgroup at 256, 64 and 16
          rows per workgroup; 34 rows that are only a slack (empty ranges).
  steps   of row_panel_cases: m = 40, structural lengths 6, 7, 8, 14, 15, 16,
          0 and 23. The kernel walks the whole row (the slack is skipped by a
          compare), so its groups of GATHER = 8 entries are met one below, at
          and one above one and two groups, as by the row sums; but 9
          structural entries are not among them, hence
  groups  of this file: m = 40, n = 30, structural lengths 7, 8, 9, 15, 16,
          17, 0 and 24 (with the slack: 8, 9, 10, 16, 17, 18, 1, 25).
  tall    of row_violation_cases: m = 66 000, 258 tiles of 256 rows, for the
          screening only, k in TALL_KS; its reference is vectorised
          (tall_ranges) and compared with ranges() on a sample of rows.

Bound pools: POOL = 33 children per small matrix, read-only; k in KS takes
the first k. An ordinary child is l = min(a, b), u = max(a, b) of two
solveops_cases._family draws (+-0.0 bounds included). Child j also gets j mod
4 of the 8 most-held structural columns set to l = -inf or u = +inf: a few
columns that many rows hold, so that the counts run from 0 to 3 on both sides
and most long rows keep a finite side. The others sit at fixed places:
  1  BOX        finite, l == u everywhere
  3  WITH_NAN   a NaN lower bound in the most-held column
  6  WRONG_INF  l = +inf in the most-held column: counted, never added
  7  HUGE       +-2^1023 in the 8 most-held columns, l = u = +2^1023 in every
                other one of them: products overflow to +inf and -inf and
                their sums to NaN. (The matrices' entries are below 2^13, so a
                bound of 2^1000 cannot overflow a sum of theirs.) Its g is
                never NaN.
Children 0, 16 and 32 are ordinary and free of infinities (j mod 4 == 0):
each is, for some k, a panel of its own.

Row-bound sets (row_bounds(name, which) -> row_lb, row_ub, tolerance), built
from the pool's reference ranges, so the same for every k:
  split      even rows: ub = the median of lo over the children with lo_inf
             == 0 (and a finite lo), lb = -inf; odd rows: lb = the median of
             hi likewise, ub = +inf; rows without such a child stay free
  free       (-inf, +inf): nothing is proven
  crossed    lb = +inf, ub = -inf: every pair with a zero count and a sum that
             is not NaN or -inf / +inf on that side is proven, worst = +inf
  edges0, edges_tol
             split, with the rows of edge_entries(name, which) rebuilt so that
             one child's g is exactly the tolerance (not proven) or the next
             double above it that a difference can give (proven), at
             tolerance 0 and EDGE_TOLERANCE.
"""
import functools
from fractions import Fraction

import numpy as np

import panel_cases as pc
import row_panel_cases as rc
import row_violation_cases as vc
import solveops_cases as sc
from device_ref import Matrix, bits

CASES = ("rows70", "steps", "groups")
SCREEN_CASES = CASES + ("tall",)
KS = rc.KS
POOL = rc.POOL
GATHER = rc.GATHER
GROUPS_M, GROUPS_N = 40, 30
GROUPS_LENS = (7, 8, 9, 15, 16, 17, 0, 24)  # structural; cycled over the rows
GROUPS_SEED = 7001
SEEDS = {"rows70": 910000, "steps": 920000, "groups": 930000, "tall": 940000}
BOX, WITH_NAN, WRONG_INF, HUGE = 1, 3, 6, 7
SPECIAL = (BOX, WITH_NAN, WRONG_INF, HUGE)
ALONE = rc.ALONE
MOST_HELD = 8
HUGE_BOUND = 2.0 ** 1023
TALL_KS = vc.TALL_KS
TALL_POOL = vc.TALL_POOL
TALL_BOX, TALL_NAN, TALL_INF = 1, 3, 4
ROW_BOUND_SETS = ("split", "free", "crossed", "edges0", "edges_tol")
EDGE_KINDS = ("lo_at", "lo_above", "hi_at", "hi_above")
EDGE_TOLERANCE = 0.375
EDGE_CHILDREN = ALONE
INF = np.inf
SUMMARY = vc.SUMMARY


def ks(name):
    return TALL_KS if name == "tall" else KS


def pool_size(name):
    return TALL_POOL if name == "tall" else POOL


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name in ("rows70", "steps"):
        return rc.matrix(name)
    if name == "tall":
        return vc.matrix(name)
    rng = np.random.default_rng(GROUPS_SEED)
    rows = []
    for r in range(GROUPS_M):
        length = GROUPS_LENS[r % len(GROUPS_LENS)]
        cols = np.sort(rng.choice(GROUPS_N, length, replace=False)).astype(np.int32)
        rows.append((cols, pc._values(rng, length)))
    mat = Matrix(GROUPS_M, GROUPS_N, rows)
    assert set(mat.row_len - 1) == set(GROUPS_LENS)
    return mat


def structural_lengths(name):
    return sorted(set(int(x) - 1 for x in matrix(name).row_len))


def most_held(mat):
    """The MOST_HELD structural columns that the most rows hold, the most-held
    first."""
    count = np.zeros(mat.n, np.int64)
    for c in mat.t_cols:
        count[c[:-1]] += 1
    return np.argsort(-count, kind="stable")[:MOST_HELD]


def _ordinary(seed, n):
    a = sc._family(np.random.default_rng(seed), n)
    b = sc._family(np.random.default_rng(seed + 500), n)
    return np.minimum(a, b), np.maximum(a, b)


@functools.lru_cache(maxsize=None)
def pool(name):
    """(L, U), each (pool_size, n), read-only."""
    mat = matrix(name)
    size = pool_size(name)
    pairs = [_ordinary(SEEDS[name] + 1000 * (j + 1), mat.n) for j in range(size)]
    L = np.stack([p[0] for p in pairs])
    U = np.stack([p[1] for p in pairs])
    if name == "tall":
        U[TALL_BOX] = L[TALL_BOX]
        L[TALL_NAN, 0] = np.nan
        L[TALL_INF, mat.n - 1] = -INF
    else:
        held = most_held(mat)
        rng = np.random.default_rng(SEEDS[name] + 77)
        for j in range(size):
            for c in rng.permutation(held)[:j % 4]:
                if rng.random() < 0.5:
                    L[j, c] = -INF
                else:
                    U[j, c] = INF
        L[BOX], U[BOX] = _ordinary(SEEDS[name] + 1000 * (BOX + 1), mat.n)
        U[BOX] = L[BOX]
        assert np.isfinite(L[BOX]).all()
        L[WITH_NAN, held[0]] = np.nan
        L[WRONG_INF, held[0]] = INF
        for i, c in enumerate(held):
            L[HUGE, c], U[HUGE, c] = (-HUGE_BOUND, HUGE_BOUND) if i % 2 == 0 else (HUGE_BOUND,
                                                                                   HUGE_BOUND)
    L.setflags(write=False)
    U.setflags(write=False)
    return L, U


def ordinary(name):
    return [j for j in range(POOL) if j not in SPECIAL]


# --- the rule -----------------------------------------------------------------------------------

def ranges(mat, L, U, order=1, product=None):
    """(lo, hi, lo_inf, hi_inf), each (k, m), of the bound sets L, U (k, n):
    the header's loop, all children of a row at once. order = -1 walks the
    entries backwards; product(a, b, acc) replaces acc + a * b (for the CPU
    test's contracted multiply-add)."""
    L, U = np.asarray(L, np.float64), np.asarray(U, np.float64)
    k = L.shape[0]
    lo, hi = np.zeros((k, mat.m)), np.zeros((k, mat.m))
    lo_inf, hi_inf = np.zeros((k, mat.m), np.int32), np.zeros((k, mat.m), np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(mat.m):
            acc_lo, acc_hi = np.zeros(k), np.zeros(k)
            for c, a in list(zip(mat.t_cols[r][:-1], mat.t_vals[r][:-1]))[::order]:
                if a == 0.0:
                    continue
                bl, bh = (L[:, c], U[:, c]) if a > 0.0 else (U[:, c], L[:, c])
                for b, acc, count in ((bl, acc_lo, lo_inf), (bh, acc_hi, hi_inf)):
                    infinite = np.isinf(b)
                    count[:, r] += infinite
                    if product is None:
                        acc[~infinite] = acc[~infinite] + a * b[~infinite]
                    else:
                        acc[~infinite] = [product(a, x, s) for x, s in
                                          zip(b[~infinite], acc[~infinite])]
            lo[:, r], hi[:, r] = acc_lo, acc_hi
    return lo, hi, lo_inf, hi_inf


def fused(a, b, acc):
    """fl(a * b + acc) with one rounding, for finite arguments."""
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(acc)):
        return acc + a * b
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(acc))
    try:
        return float(exact)
    except OverflowError:
        return INF if exact > 0 else -INF


def tall_ranges(L, U):
    """ranges() of `tall` for all rows at once: at most 3 structural entries
    per row, ascending; a skipped term is added as -0.0, which leaves every
    sum's bits as they are."""
    cols, vals, lens = vc._tall_rows()
    L, U = np.asarray(L, np.float64), np.asarray(U, np.float64)
    k, n = L.shape
    lo, hi = np.zeros((k, vc.TALL_M)), np.zeros((k, vc.TALL_M))
    lo_inf = np.zeros((k, vc.TALL_M), np.int32)
    hi_inf = np.zeros((k, vc.TALL_M), np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for e in range(3):
            a = vals[:, e]
            live = (np.arange(3)[e] < lens) & (a != 0.0)
            c = np.where(live, cols[:, e], 0)
            up = a > 0.0
            bl = np.where(up, L[:, c], U[:, c])
            bh = np.where(up, U[:, c], L[:, c])
            for b, acc, count in ((bl, lo, lo_inf), (bh, hi, hi_inf)):
                infinite = np.isinf(b)
                count += live & infinite
                acc += np.where(live & ~infinite, a * b, -0.0)
    return lo, hi, lo_inf, hi_inf


@functools.lru_cache(maxsize=None)
def reference(name):
    """(lo, hi, lo_inf, hi_inf) of the whole pool, computed once, read-only."""
    L, U = pool(name)
    out = tall_ranges(L, U) if name == "tall" else ranges(matrix(name), L, U)
    for a in out:
        a.setflags(write=False)
    return out


def screen(ref, lb, ub):
    """g (k, m) of the header's screening; never NaN."""
    lo, hi, lo_inf, hi_inf = ref
    g = np.full(lo.shape, -INF)
    with np.errstate(invalid="ignore"):
        d = lo - ub
        g = np.where((lo_inf == 0) & (d > g), d, g)
        d = lb - hi
        g = np.where((hi_inf == 0) & (d > g), d, g)
    assert not np.isnan(g).any()
    return g


def filter_reference(ref, lb, ub, tol):
    """row_starts (k + 1, int64), rows (int32), amounts and the summaries
    (SUMMARY) of the ranges ref under the header's screening."""
    lb, ub = np.asarray(lb, np.float64), np.asarray(ub, np.float64)
    assert tol >= 0.0 and np.isfinite(tol)
    assert not np.isnan(lb).any() and not np.isnan(ub).any()
    g = screen(ref, lb, ub)
    k = g.shape[0]
    keep = g > tol
    row_starts = np.zeros(k + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=row_starts[1:])
    child, row = np.nonzero(keep)  # child-major, rows ascending
    summaries = np.zeros(k, SUMMARY)
    summaries["count"] = keep.sum(axis=1)
    summaries["worst_row"] = -1
    for j in np.nonzero(summaries["count"])[0]:
        masked = np.where(keep[j], g[j], -INF)
        summaries["worst_row"][j] = np.argmax(masked)  # the first, so the lowest row
        summaries["worst"][j] = masked.max()
    return row_starts, row.astype(np.int32), g[child, row], summaries


def first(ref, k):
    return tuple(a[:k] for a in ref)


# --- row-bound sets -------------------------------------------------------------------------------

def _split(name):
    lo, hi, lo_inf, hi_inf = reference(name)
    m = lo.shape[1]
    lb, ub = np.full(m, -INF), np.full(m, INF)
    for r in range(m):
        if r % 2 == 0:
            ok = (lo_inf[:, r] == 0) & np.isfinite(lo[:, r])
            if ok.any():
                ub[r] = np.median(lo[ok, r])
        else:
            ok = (hi_inf[:, r] == 0) & np.isfinite(hi[:, r])
            if ok.any():
                lb[r] = np.median(hi[ok, r])
    return lb, ub


def _around(x):
    out = [x]
    for _ in range(3):
        out = [np.nextafter(out[0], -INF)] + out + [np.nextafter(out[-1], INF)]
    return out


def edge_target(kind, value, tol):
    """The g an edge row is built for: tol itself (*_at); the next double
    above tol (*_above, tol > 0); at tol 0 the least positive difference the
    sum `value` can show, its distance to the neighbouring double."""
    lo_kind = kind.startswith("lo")
    if kind.endswith("_at"):
        return tol
    if tol > 0.0:
        return np.nextafter(tol, INF)
    return value - np.nextafter(value, -INF) if lo_kind else np.nextafter(value, INF) - value


def _edge_bound(kind, value, tol):
    """(lb, ub) that give a row whose sum is `value` exactly edge_target's g
    (g = lo - ub for the lo kinds, lb - hi for the hi kinds, one rounded
    difference), or None when rounding does not let it land there."""
    lo_kind = kind.startswith("lo")
    want = edge_target(kind, value, tol)
    for bound in _around(value - want if lo_kind else value + want):
        if np.isfinite(bound) and (value - bound if lo_kind else bound - value) == want:
            return (-INF, bound) if lo_kind else (bound, INF)
    return None


@functools.lru_cache(maxsize=None)
def _edges(name, tol):
    lo, hi, lo_inf, hi_inf = reference(name)
    lb, ub = _split(name)
    used, entries = set(), []
    for child in (c for c in EDGE_CHILDREN if c < pool_size(name)):
        for kind in EDGE_KINDS:
            sums, counts = (lo, lo_inf) if kind.startswith("lo") else (hi, hi_inf)
            rows = sorted(range(lo.shape[1]), key=lambda r: sums[child, r] == 0.0)  # sums first
            for r in rows:
                value = sums[child, r]
                if r in used or counts[child, r] != 0 or not np.isfinite(value):
                    continue
                pair = _edge_bound(kind, value, tol)
                if pair is not None:
                    lb[r], ub[r] = pair
                    used.add(r)
                    entries.append((child, r, kind))
                    break
    # A (child, kind) without a row that rounding lets land there is left out
    # (EDGE_TOLERANCE needs a sum below 1/2 in magnitude); what has to remain
    # is asserted here and by the CPU test.
    assert {kind for _, _, kind in entries} == set(EDGE_KINDS), (name, tol, entries)
    for child in (c for c in EDGE_CHILDREN if c < pool_size(name)):
        mine = {kind[3:] for c, _, kind in entries if c == child}
        assert mine == {"at", "above"}, (name, tol, child, entries)
    return lb, ub, tuple(entries)


def edge_entries(name, which):
    """((child, row, kind), ...) of edges0 / edges_tol."""
    return _edges(name, {"edges0": 0.0, "edges_tol": EDGE_TOLERANCE}[which])[2]


@functools.lru_cache(maxsize=None)
def row_bounds(name, which):
    """(row_lb, row_ub, tolerance), read-only."""
    m = matrix(name).m
    tol = 0.0
    if which == "split":
        lb, ub = _split(name)
    elif which == "free":
        lb, ub = np.full(m, -INF), np.full(m, INF)
    elif which == "crossed":
        lb, ub = np.full(m, INF), np.full(m, -INF)
    else:
        tol = {"edges0": 0.0, "edges_tol": EDGE_TOLERANCE}[which]
        lb, ub, _ = _edges(name, tol)
        lb, ub = lb.copy(), ub.copy()
    lb.setflags(write=False)
    ub.setflags(write=False)
    return lb, ub, tol


@functools.lru_cache(maxsize=None)
def expected(name, which, k):
    """filter_reference of the first k children under a row-bound set."""
    out = filter_reference(first(reference(name), k), *row_bounds(name, which))
    for a in out:
        a.setflags(write=False)
    return out


# --- overrides ------------------------------------------------------------------------------------

OVERRIDE_SETS = ("branch", "mixed", "k17")


@functools.lru_cache(maxsize=None)
def override_set(name, which):
    """(base_lb, base_ub, [(cols int32, new_lbs, new_ubs), ...]).
    "branch": the pool's child 0 as the node and 6 children that differ from
    it in one bound of one column (a branching node: down and up branches of
    three columns). "mixed" (k = 5): no overrides; column 0 and column n - 1;
    +-0.0, NaN, +inf and -inf bounds in shared columns; 20 columns; a few.
    "k17": 17 children of a few overrides each, across a panel boundary.
    Columns are unsorted and distinct within a child."""
    mat = matrix(name)
    L, U = pool(name)
    rng = np.random.default_rng(SEEDS[name] + 50)
    base_lb, base_ub = L[0].copy(), U[0].copy()
    base_lb.setflags(write=False)
    base_ub.setflags(write=False)

    def some(count):
        cols = rng.permutation(mat.n)[:count].astype(np.int32)
        a, b = pc._values(rng, count), pc._values(rng, count)
        return cols, np.minimum(a, b), np.maximum(a, b)

    if which == "branch":
        sets = []
        for c in most_held(mat)[:3]:
            mid = pc._values(rng, 1)
            col = np.array([c], np.int32)
            sets.append((col, base_lb[[c]], np.floor(mid)))
            sets.append((col, np.ceil(mid), base_ub[[c]]))
    elif which == "k17":
        sets = [some(int(rng.integers(1, 6))) for _ in range(17)]
    else:
        held = most_held(mat)[:4].astype(np.int32)
        sets = [(np.zeros(0, np.int32), np.zeros(0), np.zeros(0)),
                (np.array([mat.n - 1, 0], np.int32), *some(2)[1:]),
                (held, np.array([0.0, np.nan, -INF, INF]), np.array([-0.0, 1.0, INF, INF])),
                some(20), some(3)]
    for cols, lo, hi in sets:
        assert len(set(cols.tolist())) == len(cols) == len(lo) == len(hi)
    return base_lb, base_ub, sets


def materialise(base_lb, base_ub, sets):
    """The dense bound sets of an override set: the header's definition."""
    L = np.tile(np.asarray(base_lb, np.float64), (len(sets), 1))
    U = np.tile(np.asarray(base_ub, np.float64), (len(sets), 1))
    for j, (cols, lo, hi) in enumerate(sets):
        L[j, cols] = lo
        U[j, cols] = hi
    return L, U


def flatten(sets):
    """starts (k + 1, int64), cols (int32), new_lbs, new_ubs of the C call."""
    starts = np.zeros(len(sets) + 1, np.int64)
    np.cumsum([len(c) for c, _, _ in sets], out=starts[1:])
    cols = np.concatenate([np.zeros(0, np.int32)] + [c for c, _, _ in sets]).astype(np.int32)
    lo = np.concatenate([np.zeros(0)] + [x for _, x, _ in sets]).astype(np.float64)
    hi = np.concatenate([np.zeros(0)] + [x for _, _, x in sets]).astype(np.float64)
    return starts, cols, lo, hi


def pool_as_overrides(name, k):
    """The first k children of the pool as overrides of child 0: per child the
    columns in which it differs from child 0 in a bit of either bound."""
    L, U = pool(name)
    sets = []
    for j in range(k):
        cols = np.nonzero((bits(L[j]) != bits(L[0])) | (bits(U[j]) != bits(U[0])))[0]
        cols = cols.astype(np.int32)
        sets.append((cols, L[j, cols], U[j, cols]))
    return L[0], U[0], sets


@functools.lru_cache(maxsize=None)
def override_reference(name, which):
    base_lb, base_ub, sets = override_set(name, which)
    out = ranges(matrix(name), *materialise(base_lb, base_ub, sets))
    for a in out:
        a.setflags(write=False)
    return out


def override_bytes(name, sets):
    """What an override call sends up: two bases, (column, lower, upper)
    triples, starts."""
    return 16 * matrix(name).n + 20 * sum(len(c) for c, _, _ in sets) + 8 * (len(sets) + 1)


# --- comparisons ----------------------------------------------------------------------------------

def same_ranges(got, want, what):
    """lo and hi on all 64 bits (NaNs included), the counts as integers."""
    for g, w, part in zip(got, want, ("lo", "hi", "lo_inf", "hi_inf")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, part, g.shape, w.shape)
        if part in ("lo", "hi"):
            bad = np.argwhere(bits(g) != bits(w))
            assert len(bad) == 0, (what, part, len(bad), bad[:3].tolist())
        else:
            assert g.dtype == np.int32 and np.array_equal(g, w), (what, part)


same_result = vc.same_result
same_summaries = vc.same_summaries
