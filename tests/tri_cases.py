"""Triangles, right-hand sides and expected launch plans for the operation-
level tests of the device triangular solves (tests/test_tri_ref_cpu.py,
tests/test_tri_ops_gpu.py, tests/test_dense_tail_ops_gpu.py).

TEST INFRASTRUCTURE ONLY. A triangle is made from a level sequence in the
loop's own order (make_dag): output i of the loop reads outputs j < i only, at
least one of them on the level below its own, so the schedule the engine
builds has exactly the level widths asked for (asserted here from the
triangle, and again on the device from last_tri). The levels are interleaved
along the loop order: the first output of every level comes first, in level
order, the rest follow shuffled, so the engine's position map is a real
permutation. An output's entries are evaluated by ascending loop index of what
they read (the scatter loops leave no choice); where its deepest entry sits in
that order -- first, middle, last -- is chosen through which outputs it reads.

Values: mantissas in [1, 2) with random signs; off-diagonal exponents in
[-12, 0], each output's entries then scaled by a power of two so that their
absolute sum lies in (0.5, 1]; diagonal magnitudes in [1, 2); right-hand sides
with exponents in [-20, 20].

The six kinds map the same loop-order triangle onto the matrix their host
loop expects (to_tri). An identity prefix of p columns lies outside the
schedule for the kinds whose loops stop at the first non-identity column; for
kUpperTUp its rows are read (the first p outputs of the loop), for kUpper they
receive (the last p outputs, read by nobody).
"""
import functools

import numpy as np

import tri_ref
from tri_ref import LOWER, LOWER_T, UNIT_ROW, UPPER, UPPER_T, UPPER_T_UP, Tri

LDS_VALS = 16384        # kTriLdsVals
CHAIN_VALS = 12288      # kTriChainVals
SYNCFREE_MAX = 131072   # kTriSyncFreeMaxWork
PREFETCHED = 2048       # kTriPrefetch * kTriThreads
GRID_CAP = 1024 * 256   # threads of the capped grids

FIRST, MIDDLE, LAST = "first", "middle", "last"
ENTRY_COUNTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 15, 16, 17, 24, 25, 72)
# Every count with its deepest entry first, middle and last.
ENTRY_CYCLE = tuple((k, w) for w in (FIRST, MIDDLE, LAST) for k in ENTRY_COUNTS)
FEW = tuple((k, w) for k in (1, 2, 3) for w in (FIRST, LAST))


class Dag:
    """A triangle in loop order: output i reads src[starts[i]:starts[i + 1]]
    (ascending, the evaluation order) with the coefficients val."""

    def __init__(self, level, starts, src, val, diag, head, tail):
        self.level, self.starts, self.src, self.val, self.diag = level, starts, src, val, diag
        self.head, self.tail = head, tail
        self.n = len(level)


def _pick(rng, population, k):
    """k distinct integers of range(population), k <= population."""
    if k == 0:
        return np.zeros(0, np.int64)
    if population <= 4 * k:
        return rng.permutation(population)[:k]
    got = np.unique(rng.integers(0, population, 2 * k))
    while len(got) < k:
        got = np.unique(np.concatenate([got, rng.integers(0, population, 2 * k)]))
    return rng.permutation(got)[:k]


def make_dag(widths, counts, seed, unit, head=0, tail=0):
    """widths[l] outputs on level l (every level at least one), entry counts
    and deepest-entry places cycling through `counts` over the outputs of the
    levels above 0. head: that many extra level-0 outputs first (diagonal 1,
    no entries); tail: the last that many outputs are read by nobody and have
    diagonal 1."""
    rng = np.random.default_rng(seed)
    widths = np.asarray(widths, np.int64)
    depth = len(widths)
    assert (widths >= 1).all()
    rest = np.repeat(np.arange(depth), widths - 1)
    rng.shuffle(rest)
    level = np.concatenate([np.zeros(head, np.int64), np.arange(depth), rest]).astype(np.int32)
    n = len(level)
    readable = np.ones(n, bool)
    if tail:
        readable[n - tail:] = False
    lt, eq = {}, {}
    lists = {}
    cyc = 0
    for i in np.nonzero(level > 0)[0].tolist():
        l = int(level[i])
        if l not in lt:
            lt[l] = np.nonzero((level < l) & readable)[0]
            eq[l] = np.searchsorted(lt[l], np.nonzero((level == l - 1) & readable)[0])
        cand = lt[l]                          # what output i may read, ascending
        nl = int(np.searchsorted(cand, i))    # ... of them before i
        deep = eq[l][:int(np.searchsorted(cand[eq[l]], i))]  # places in cand of level l - 1
        k, where = counts[cyc % len(counts)]
        cyc += 1
        k = min(k, nl)
        below_want = {FIRST: 0, LAST: k - 1, MIDDLE: (k - 1) // 2}[where]
        ok = deep[(deep >= below_want) & (nl - deep - 1 >= k - 1 - below_want)]
        if len(ok) > 0:
            d = int(ok[rng.integers(len(ok))])
        else:  # not enough on the wanted side: the count comes first
            d = int(deep[rng.integers(len(deep))])
            below_want = min(below_want, d)
            if nl - d - 1 < k - 1 - below_want:
                below_want = k - 1 - (nl - d - 1)
        lo = _pick(rng, d, below_want)
        hi = d + 1 + _pick(rng, nl - d - 1, k - 1 - below_want)
        lists[i] = np.sort(cand[np.concatenate([lo, [d], hi]).astype(np.int64)])
    counts_of = np.zeros(n, np.int64)
    for i, s in lists.items():
        counts_of[i] = len(s)
    starts = np.zeros(n + 1, np.int64)
    np.cumsum(counts_of, out=starts[1:])
    src = (np.concatenate([lists[i] for i in sorted(lists)]) if lists
           else np.zeros(0, np.int64)).astype(np.int64)
    e = len(src)
    val = np.ldexp((1.0 + rng.random(e)) * rng.choice([-1.0, 1.0], e),
                   rng.integers(-12, 1, e).astype(np.int32))
    if e > 0:
        has = np.nonzero(counts_of > 0)[0]
        sums = np.add.reduceat(np.abs(val), starts[has])
        m, ex = np.frexp(sums)               # sums = m * 2^ex, m in [0.5, 1)
        shift = np.where(m > 0.5, -ex, -ex + 1)
        val = np.ldexp(val, np.repeat(shift, counts_of[has]).astype(np.int32))
        check = np.add.reduceat(np.abs(val), starts[has])
        assert ((check > 0.5) & (check <= 1.0)).all()
    diag = np.ones(n) if unit else (1.0 + rng.random(n)) * rng.choice([-1.0, 1.0], n)
    diag[:head] = 1.0
    if tail:
        diag[n - tail:] = 1.0
    dag = Dag(level, starts, src, val, diag, head, tail)
    # The levels are what was asked for.
    lv = np.zeros(n, np.int64)
    out_of = np.repeat(np.arange(n), counts_of)
    if e > 0:
        assert (src < out_of).all()
        for i in np.nonzero(counts_of > 0)[0].tolist():
            lv[i] = 1 + lv[src[starts[i]:starts[i + 1]]].max()
    assert (lv == level).all()
    return dag


def to_tri(kind, dag, prefix=0):
    """The matrix of `kind` whose host loop evaluates dag in its order. The
    kinds with rows below the diagonal get `prefix` identity columns in
    front; the other two carry theirs inside the dag (head / tail)."""
    n_out = dag.n
    counts = np.diff(dag.starts)
    out_of = np.repeat(np.arange(n_out), counts)
    place = np.arange(len(dag.src)) - np.repeat(dag.starts[:-1], counts)
    if kind in (UPPER_T, LOWER_T):
        n = prefix + n_out
        col, row = n - 1 - out_of, n - 1 - dag.src
        order = np.lexsort((-place, col))    # evaluated from the column's end
        diag = np.concatenate([np.ones(prefix), dag.diag[::-1]])
    elif kind == UPPER_T_UP:
        assert prefix == 0
        n = n_out
        col, row = out_of, dag.src
        order = np.arange(len(col))
        diag = dag.diag.copy()
    elif kind in (LOWER, UNIT_ROW):
        n = prefix + n_out
        col, row = prefix + dag.src, prefix + out_of
        order = np.lexsort((row, col))
        diag = np.concatenate([np.ones(prefix), dag.diag])
    else:
        assert kind == UPPER and prefix == 0
        n = n_out
        col, row = n - 1 - dag.src, n - 1 - out_of
        order = np.lexsort((row, col))
        diag = dag.diag[::-1].copy()
    col, row, val = col[order], row[order], dag.val[order]
    starts = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(col, minlength=n), out=starts[1:])
    return Tri(n, starts, row, val, diag)


def row_of_output(kind, n, prefix, i):
    """The matrix row of loop output i (numpy arrays welcome)."""
    if kind in (UPPER_T, LOWER_T, UPPER):
        return n - 1 - i
    return i + (prefix if kind in (LOWER, UNIT_ROW) else 0)


# --- the cases --------------------------------------------------------------------------------

def _spec(widths, counts=FEW, unit=False, seed=1):
    return {"widths": list(widths), "counts": counts, "unit": unit, "seed": seed}


SPECS = {
    # Every entry count at the group-of-four and window-of-8 boundaries, each
    # with its deepest entry first, middle and last; ~150 levels deep.
    "entries": _spec([90] + [3, 4] * 74 + [3], ENTRY_CYCLE, seed=11),
    "entries_unit": _spec([90] + [3, 4] * 74 + [3], ENTRY_CYCLE, unit=True, seed=12),
    "widths": _spec([1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025], seed=13),
    "widths_unit": _spec([40, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025], unit=True, seed=14),
    "wide_prefetch": _spec([556, 2047, 2048, 2049, 3500], seed=15),
    "lds_cut_448": _spec([448] * 40, seed=16),
    "lds_cut_256": _spec([256] * 65, seed=17),
    "chain_cut_500": _spec([500] * 30, seed=18),
    "chain_cut_256": _spec([256] * 49, seed=19),
    "chain_cut_wide": _spec([300] * 5 + [CHAIN_VALS + 1] + [300] * 5, seed=20),
    "syncfree_limit": _spec([SYNCFREE_MAX + 1, 200, 200, 200], seed=21),
    "syncfree_at_limit": _spec([SYNCFREE_MAX - 600, 200, 200, 200], seed=22),
    "grid_stride": _spec([GRID_CAP + 100] + [100] * 5, seed=23),
    "grid_stride_unit": _spec([GRID_CAP + 600 - 2000] + [200] * 10, unit=True, seed=24),
    "small": _spec([40, 30, 30, 25, 25, 20, 20, 20], ENTRY_CYCLE, seed=25),
    "small_unit": _spec([40, 30, 30, 25, 25, 20, 20, 20], ENTRY_CYCLE, unit=True, seed=26),
}
PREFIXES = (0, 1, 63, 64, 65)
for _p in PREFIXES:
    SPECS[f"identity_prefix_{_p}"] = dict(SPECS["small"], prefix=_p, seed=30 + _p)
    SPECS[f"identity_prefix_{_p}_unit"] = dict(SPECS["small_unit"], prefix=_p, seed=40 + _p)
BIG = ("syncfree_limit", "syncfree_at_limit", "grid_stride", "grid_stride_unit", "lds_cut_448",
       "lds_cut_256", "chain_cut_500", "chain_cut_256", "chain_cut_wide")
ALL_KINDS = (UPPER_T, LOWER, UPPER_T_UP, LOWER_T, UNIT_ROW, UPPER)


@functools.lru_cache(maxsize=None)
def dag_of(name, kind):
    s = SPECS[name]
    p = s.get("prefix", 0)
    head = p if kind == UPPER_T_UP else 0
    tail = p if kind == UPPER else 0
    # One dag for the kinds that keep the prefix outside it.
    if head == 0 and tail == 0 and kind != UPPER_T:
        return dag_of(name, UPPER_T)
    return make_dag(s["widths"], s["counts"], s["seed"], s["unit"], head, tail)


@functools.lru_cache(maxsize=None)
def tri_of(name, kind):
    p = SPECS[name].get("prefix", 0)
    return to_tri(kind, dag_of(name, kind), 0 if kind in (UPPER_T_UP, UPPER) else p)


def listed_widths(name, kind):
    """Level widths of the schedule the engine builds: listed outputs only
    (with a unit diagonal an output without entries is not listed); the two
    kinds scheduled from row 0 list their identity rows."""
    s = SPECS[name]
    w = list(s["widths"])
    if kind == UPPER_T_UP:
        w[0] += s.get("prefix", 0)
    if s["unit"]:
        w[0] = 0
    return w


def first_output(name, kind):
    """TriSchedule::first_col."""
    return 0 if kind in (UPPER_T_UP, UPPER) else tri_of(name, kind).first_non_identity


# --- the launch plan the engine is expected to choose --------------------------------------------

def _i(env, key, default):
    return int(env.get(key, default))


def expected_plan(widths, unit, env):
    """last_tri of a non-trivial solve on a schedule of these listed level
    widths under env (the MILP_TRI_* switches), from the rules of
    DESIGN.md's section on device solves: which plan, how many launches of
    each kind, where the runs are cut."""
    syncfree = _i(env, "MILP_TRI_SYNCFREE", 1) != 0
    persist = _i(env, "MILP_TRI_PERSIST", 0)
    chain = _i(env, "MILP_TRI_CHAIN", 0) != 0 and syncfree and persist == 0
    chain_width = _i(env, "MILP_TRI_CHAIN_WIDTH", 512)
    chain_min = max(1, _i(env, "MILP_TRI_CHAIN_MIN_LEVELS", 4))
    pad_on = _i(env, "MILP_TRI_PAD", 0) != 0 or not syncfree
    fuse0 = _i(env, "MILP_TRI_FUSE0", 1) != 0
    wide = min(_i(env, "MILP_TRI_WIDE", 600), LDS_VALS - 64)
    depth = len(widths)
    pad64 = lambda w: (w + 63) // 64 * 64
    # Single-workgroup segments of the sync-free plan.
    segs = []
    if chain:
        wide_from = l = 0
        while l < depth:
            if widths[l] > chain_width:
                l += 1
                continue
            e, held = l, 0
            while e < depth and widths[e] <= chain_width and held + widths[e] <= CHAIN_VALS:
                held += widths[e]
                e += 1
            if e - l >= chain_min:
                if l > wide_from:
                    segs.append((wide_from, l, 0))
                segs.append((l, e, 1))
                wide_from = e
            l = max(e, l + 1)
        if wide_from < depth:
            segs.append((wide_from, depth, 0))
    else:
        segs = [(0, depth, 0)]
    narrow = [False] * depth
    for b, e, nar in segs:
        if nar:
            narrow[b:e] = [True] * (e - b)
    start = [0]
    for l in range(depth):
        start.append(start[-1] + (pad64(widths[l]) if pad_on and not narrow[l] else widths[l]))
    runs = [(start[b], start[e], nar) for b, e, nar in segs if start[e] > start[b]]
    max_wide = max([e - b for b, e, nar in runs if not nar], default=0)
    level0_end = 0 if narrow[0] else start[1]
    out = {"work": start[-1], "levels": depth, "chain_levels": sum(narrow),
           "level0_end": level0_end, "max_wide_run": max_wide,
           "wide_runs": 0, "chain_runs": 0, "chip_launches": 0, "cu_runs": 0}
    if persist > 0 and syncfree:
        out["plan"] = "persistent"
        out["fused0"] = fuse0 and level0_end > 0
    elif syncfree and max_wide <= SYNCFREE_MAX:
        out["plan"] = "sync_free"
        l0 = level0_end if fuse0 else 0
        out["fused0"] = l0 > 0
        for b, e, nar in runs:
            if e > max(b, l0):
                out["chain_runs" if nar else "wide_runs"] += 1
    else:
        out["plan"] = "levels"
        launches = []
        l = 0
        while l < depth:
            if widths[l] == 0:
                l += 1
            elif widths[l] > wide:
                launches.append(("chip", l, l + 1))
                l += 1
            else:
                e, run = l, 0
                while e < depth and widths[e] <= wide:
                    if e > l and run + pad64(widths[e]) > LDS_VALS:
                        break
                    run += pad64(widths[e])
                    e += 1
                launches.append(("cu", l, e))
                l = e
        out["fused0"] = fuse0 and not unit and bool(launches) and launches[0][:2] == ("chip", 0)
        rest = launches[1:] if out["fused0"] else launches
        out["chip_launches"] = sum(1 for x in rest if x[0] == "chip")
        out["cu_runs"] = sum(1 for x in rest if x[0] == "cu")
        out["cu_run_levels"] = [x[1:] for x in launches if x[0] == "cu"]
    return out


# --- right-hand sides -----------------------------------------------------------------------------

def dense_rhs(rng, n):
    return np.ldexp((1.0 + rng.random(n)) * rng.choice([-1.0, 1.0], n),
                    rng.integers(-20, 21, n).astype(np.int32))


def rhs_list(name, kind, full=True):
    """[(label, x, start)] for the triangle of (name, kind). full=False: the
    dense vector and the trailing zeros only (the large cases)."""
    t = tri_of(name, kind)
    n, fni = t.n, t.first_non_identity
    rng = np.random.default_rng(SPECS[name]["seed"] * 100 + kind)
    out = [("dense", dense_rhs(rng, n), 0)]
    # Trailing zeros, the last one -0.0 on a negative diagonal where there is
    # one: rows the trimming kinds neither compute nor divide.
    x = dense_rhs(rng, n)
    cut = n - max(2, n // 7)
    x[cut:] = 0.0
    neg = cut + np.nonzero(t.diag[cut:] < 0)[0]
    x[neg[-1] if len(neg) else n - 1] = -0.0
    out.append(("trailing_zeros", x, 0))
    if not full:
        return out
    # A second dense vector (same key: the pending marks are set again).
    out.append(("dense2", dense_rhs(rng, n), 0))
    x = dense_rhs(rng, n)
    x[fni + (n - fni) // 2:] = 0.0
    out.append(("top_inside_a_level", x, 0))
    x = dense_rhs(rng, n)
    x[fni + 1:] = 0.0
    out.append(("top_at_first_non_identity", x, 0))
    x = dense_rhs(rng, n)
    x[fni:] = 0.0
    out.append(("only_below_first_non_identity", x, 0))
    out.append(("all_zero", np.zeros(n), 0))
    for label, v in (("nan", np.nan), ("plus_inf", np.inf), ("minus_inf", -np.inf)):
        x = dense_rhs(rng, n)
        x[fni + (n - fni) // 3] = v
        out.append((label, x, 0))
    if kind in tri_ref.SEQUENTIAL and kind != UPPER:
        # LowerSolveStartingAt(start) above the first non-identity column: the
        # engine's precondition is that everything below start is zero.
        x = dense_rhs(rng, n)
        start = fni + (n - fni) // 4
        x[:start] = 0.0
        out.append(("start_above_first_non_identity", x, start))
    return out


def special_tri(kind, which, unit=False):
    """Small triangles with one planted event, and their right-hand side:
    (Tri, x, rows) where `rows` are the rows the event decides.
      inf_meets_zero: an infinite coefficient whose input value is zero: NaN
        in the grouped kinds, skipped in the sequential ones.
      cancellation (sequential kinds): outputs whose single subtraction
        cancels exactly; the zero is not divided (its diagonal is negative)
        and its column is skipped, though that column holds infinite
        coefficients: every output reading it would become NaN without the
        skip."""
    s = _spec([30, 30, 30, 30, 30], ((5, FIRST), (6, LAST), (9, MIDDLE), (2, FIRST)), unit,
              seed=70 + kind)
    dag = make_dag(s["widths"], s["counts"], s["seed"], unit)
    rng = np.random.default_rng(700 + kind)
    x_out = dense_rhs(rng, dag.n)            # by loop output
    level, starts, src = dag.level, dag.starts, dag.src
    val, diag = dag.val.copy(), dag.diag.copy()
    if which == "inf_meets_zero":
        zero = np.nonzero(level == 0)[0][:10]  # level 0: the input is the value
        x_out[zero] = 0.0
        hit = np.nonzero(np.isin(src, zero))[0]
        val[hit] = np.inf
    else:
        assert which == "cancellation" and kind in tri_ref.SEQUENTIAL
        # Level-1 outputs cut down to their one level-0 entry; x there is the
        # product the loop subtracts, so the difference is exactly 0.0.
        ones_ = np.nonzero(level == 1)[0][:12]
        keep = np.ones(len(src), bool)
        for i in ones_.tolist():
            b, e = starts[i], starts[i + 1]
            first0 = b + int(np.argmax(level[src[b:e]] == 0))
            keep[b:e] = False
            keep[first0] = True
            j = src[first0]
            coeff = x_out[j] if unit else x_out[j] / diag[j]
            x_out[i] = coeff * val[first0]
            if not unit:
                diag[i] = -abs(diag[i])
        hit = np.isin(src, ones_) & keep
        val[hit] = np.inf
        counts = np.add.reduceat(keep.astype(np.int64), starts[:-1][np.diff(starts) > 0])
        new_counts = np.zeros(dag.n, np.int64)
        new_counts[np.diff(starts) > 0] = counts
        starts = np.zeros(dag.n + 1, np.int64)
        np.cumsum(new_counts, out=starts[1:])
        src, val = src[keep], val[keep]
        zero = ones_
    d2 = Dag(level, starts, src, val, diag, 0, 0)
    t = to_tri(kind, d2)
    x = np.zeros(t.n)
    x[row_of_output(kind, t.n, 0, np.arange(dag.n))] = x_out
    return t, x, row_of_output(kind, t.n, 0, zero)


# --- dense tail -----------------------------------------------------------------------------------

TAIL_N = 400
TAIL_COLS = (1, 63, 64, 65, 129)
TAIL_DENSE = max(16, TAIL_N // 8)  # entries of a dense column
TAIL_VARIANTS = ("prefix64", "prefix68", "prefix128", "prefix132", "tail_row_first",
                 "out_of_order", "exactly_dense")


def tail_tri(T, unit, identity=False, offset=0, n=TAIL_N, seed=0):
    """An upper triangle (rows < column) for TransposeUpperSolve whose last T
    columns are dense (at least n / 8 entries) and column t - 1 is one short
    of dense. Tail column q = c - t is built by variant (q + offset) mod 7:
      prefix64 / 68 / 128 / 132: that many rows below t first (ascending),
        then rows of the tail;
      tail_row_first: the previous column's row inside the first group of
        four, then more than 72 rows below t (the advance takes nothing, the
        finish reads past its staged entries);
      out_of_order: 64 rows below t, a tail row, then more rows below t;
      exactly_dense: n / 8 rows below t and nothing else.
    identity: the columns before t are identity columns (t stops at the first
    non-identity column); else they are sparse, column t - 1 holding one entry
    less than a dense one. Returns (Tri, t, variants used by column)."""
    rng = np.random.default_rng(1000 * T + 10 * offset + (1 if unit else 0) + seed)
    t = n - T
    dense = max(16, n // 8)
    assert t > 140 and dense <= 64
    cols, used = [], []
    for c in range(n):
        if c < t:
            if identity or c < 4:
                rows = np.zeros(0, np.int64)
            elif c == t - 1:
                rows = np.sort(rng.permutation(c)[:dense - 1])
            else:
                rows = np.sort(rng.permutation(c)[:rng.integers(0, 4)])
            cols.append(rows)
            continue
        q = c - t
        variant = TAIL_VARIANTS[(q + offset) % len(TAIL_VARIANTS)]
        own = t + q - 1 if q % 64 >= 1 else None  # a row of the column's own block
        below = rng.permutation(t)
        in_tail = t + rng.permutation(q)[:rng.integers(0, q + 1)] if q else np.zeros(0, np.int64)
        if variant.startswith("prefix"):
            p = int(variant[6:])
            rows = np.concatenate([np.sort(below[:p]), np.sort(in_tail)])
        elif variant == "tail_row_first" and own is not None:
            rows = np.concatenate([below[:2], [own], below[2:2 + 80 + q % 4]])
        elif variant == "out_of_order" and own is not None:
            rows = np.concatenate([np.sort(below[:64]), [own], below[64:64 + 20 + q % 4]])
        else:
            variant = "exactly_dense"
            rows = np.sort(below[:dense])
        assert len(rows) >= dense and len(np.unique(rows)) == len(rows) and rows.max() < c
        used.append((variant, len(rows)))
        cols.append(rows.astype(np.int64))
    counts = np.array([len(r) for r in cols], np.int64)
    starts = np.zeros(n + 1, np.int64)
    np.cumsum(counts, out=starts[1:])
    rows = np.concatenate(cols).astype(np.int64)
    e = len(rows)
    val = np.ldexp((1.0 + rng.random(e)) * rng.choice([-1.0, 1.0], e),
                   rng.integers(-12, 1, e).astype(np.int32))
    has = np.nonzero(counts > 0)[0]
    m, ex = np.frexp(np.add.reduceat(np.abs(val), starts[has]))
    val = np.ldexp(val, np.repeat(np.where(m > 0.5, -ex, -ex + 1), counts[has]).astype(np.int32))
    diag = np.ones(n) if unit else (1.0 + rng.random(n)) * rng.choice([-1.0, 1.0], n)
    if identity:
        diag[:t] = 1.0
    tri = Tri(n, starts, rows, val, diag)
    assert not identity or tri.first_non_identity == t
    return tri, t, used
