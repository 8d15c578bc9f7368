"""Inputs and the numpy reference of the bound-propagation tests
(DeviceLp::BoundPropagatePanel(From) and BoundPropagatedColumnsFrom,
mi_lp_bound_propagate(_from), mi_lp_bound_propagated_columns_from):
tests/test_bound_propagate_ops_gpu.py and tests/test_bound_propagate_gpu.py,
checked without a GPU by tests/test_bound_propagate_ref_cpu.py.

TEST INFRASTRUCTURE ONLY. propagate() restates the rule of include/mi_lp.h
(mi_lp_bound_propagate) in numpy, one rounded operation at a time, on top of
bound_range_cases.ranges and bound_implied_cases.implied. propagate_scalar() is
a literal Python-float copy of the header's loop for the CPU test.
changed_reference() restates the keep rule of the lists.

Hand cases (hand(name)): chain, halving, knapsack and negzero (an integer
column whose implied lower bound -0.5 must end at +0.0): small matrices whose
results the tests assert literally.

Node cases (node(name, f)) on rows70, steps, groups and wide of
bound_implied_cases (both column shapes, partial workgroups and filter tiles):
  base      the pool's child 0, the bounds of the integer columns (c % 3 == 0)
            rounded outward to integers.
  witness   x0 = the midpoint of the base's box, rounded on integer columns.
  rows      ub = A x0 + f w on rows with r % 4 in {0, 2}, lb = A x0 - f w on
            rows with r % 4 in {1, 2}; w = hi - lo of the base's activity range;
            f in FS.
  children  child 0 is the base; child j overrides 1 + j % 3 random columns:
            even j with a box of a tenth of the column's width around x0, odd j
            with a lower bound 60 % of the way from x0 to u; integer columns
            rounded inward. On `wide` the columns are drawn at random among
            those of at least 63 entries: drawn among all 700, no child of
            that matrix is infeasible at any entry of the grid (only a long
            column's bound is felt by enough rows), and INFEASIBLE beside
            FIXPOINT in one call of several tiles would go untested.
Parameters: k in KS (16 plus a second panel of one is the case that matters),
max_rounds in ROUNDS, tolerance in TOLERANCES, with and without integers:
grid(name) lists the (f, tolerance, integers) that run, the same eight on every
matrix.
A set's result does not depend on the other sets of its call, and a run of R
rounds is the run of R' > R rounds stopped early, so trace() computes each
(matrix, f, tolerance, integers) once for the CHILDREN sets at the largest
max_rounds and snapshots the others. The traces fold a round's candidates with
implied_columns(), which the CPU test holds to bound_implied_cases.implied bit
for bit; propagate() itself, the hand cases and the special children use
implied().
"""
import functools

import numpy as np

import bound_implied_cases as ic
import bound_range_cases as bc
from device_ref import Matrix, bits

CASES = ic.CASES
KS = (1, 3, 4, 16, 17)
CHILDREN = 17
ROUNDS = (1, 3, 30)
TOLERANCES = (0.0, 1e-9, 0.375)
FS = (0.05, 0.15)
ITOL = 1e-6
INF = np.inf
ROUND_LIMIT, FIXPOINT, INFEASIBLE = 0, 1, 2
NODE_SEED = 990000
SUMMARY = np.dtype([("status", np.int32), ("rounds", np.int32), ("moves", np.int64),
                    ("worst", np.float64), ("worst_col", np.int32), ("kept", np.int32)])
assert SUMMARY.itemsize == 32


# --- the rule -------------------------------------------------------------------------------------

def new_summaries(k):
    s = np.zeros(k, SUMMARY)
    s["worst_col"] = -1
    return s


def round_integers(NL, NU, is_integer, itol):
    """One rounded difference / sum, an exact ceil / floor, + 0.0."""
    if is_integer is None:
        return NL, NU
    ints = np.asarray(is_integer) != 0
    NL, NU = NL.copy(), NU.copy()
    with np.errstate(invalid="ignore"):
        NL[:, ints] = np.ceil(NL[:, ints] - itol) + 0.0
        NU[:, ints] = np.floor(NU[:, ints] + itol) + 0.0
    return NL, NU


def apply_round(L, U, NL, NU, tol):
    """(L', U', moved, cross, crossing) of the move rule."""
    with np.errstate(invalid="ignore", over="ignore"):
        moved = (NL - L > tol) | (U - NU > tol)  # NaN: no
        L2, U2 = np.where(moved, NL, L), np.where(moved, NU, U)
        cross = L2 - U2
        crossing = cross > tol
    return L2, U2, moved, cross, crossing


def implied_columns(mat, L, U, ref, rlb, rub):
    """bound_implied_cases.implied(mat, L, U, ref, rlb, rub) with the candidates
    of all entries of a set formed at once and folded per column by
    minimum / maximum.reduceat: the same independently rounded candidates, and a
    max and a min of them have the same bits in any order.
    tests/test_bound_propagate_ref_cpu.py holds it to implied() bit for bit on
    every matrix; the traces use it because implied() walks the entries of a
    column one after the other in Python (29 000 a round on `wide`)."""
    L, U = np.asarray(L, np.float64), np.asarray(U, np.float64)
    lo, hi, lo_inf, hi_inf = ref
    rlb, rub = np.asarray(rlb, np.float64), np.asarray(rub, np.float64)
    starts = np.asarray(mat.col_starts[:mat.n + 1], np.int64)
    entries = int(starts[-1])
    NL, NU = L.copy(), U.copy()
    if entries == 0:
        return NL, NU
    rows = np.asarray(mat.row_idx[:entries], np.int64)
    a = np.asarray(mat.vals[:entries], np.float64)
    lens = np.diff(starts)
    col_of = np.repeat(np.arange(mat.n), lens)
    filled = lens > 0
    first = starts[:-1][filled]
    live = (a != 0.0) & ~np.isnan(a)
    up = a > 0.0
    rub_e, rlb_e = rub[rows], rlb[rows]

    def side(rb, total, count, b):
        none = count == 0
        own = (count == 1) & np.isinf(b)
        res = np.where(none, total - a * b, total)
        q = (rb - res) / a
        return q + 0.0, live & np.isfinite(rb) & (none | own) & np.isfinite(q)

    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        for j in range(L.shape[0]):
            l_e, u_e = L[j, col_of], U[j, col_of]
            q_lo, ok_lo = side(rub_e, lo[j, rows], lo_inf[j, rows], np.where(up, l_e, u_e))
            q_hi, ok_hi = side(rlb_e, hi[j, rows], hi_inf[j, rows], np.where(up, u_e, l_e))
            upper = np.where(np.where(up, ok_lo, ok_hi), np.where(up, q_lo, q_hi), INF)
            lower = np.where(np.where(up, ok_hi, ok_lo), np.where(up, q_hi, q_lo), -INF)
            least = np.minimum.reduceat(upper, first)
            most = np.maximum.reduceat(lower, first)
            own_u, own_l = NU[j, filled], NL[j, filled]
            NU[j, filled] = np.where(least < own_u, least, own_u)
            NL[j, filled] = np.where(most > own_l, most, own_l)
    return NL, NU


def trace_rounds(mat, L, U, rlb, rub, is_integer, tol, itol, rounds, stats=None,
                 implied=None):
    """{R: (new_lbs, new_ubs, summaries)} for every R of `rounds`: the rule run
    to max(rounds) and looked at after each R. kept counts the columns that
    differ in bits from the input. stats: a dict that receives
    "rounded_alone", the bounds that the integer rounding alone changed.
    implied: the one-round rule, bound_implied_cases.implied unless given."""
    implied = implied or ic.implied
    assert tol >= 0.0 and np.isfinite(tol) and 0.0 <= itol < 0.5
    L0, U0 = np.asarray(L, np.float64), np.asarray(U, np.float64)
    L, U = L0.copy(), U0.copy()
    k = L.shape[0]
    s = new_summaries(k)
    active = np.ones(k, bool)
    out = {}
    for rnd in range(1, max(rounds) + 1):
        idx = np.nonzero(active)[0]
        if len(idx) > 0:
            l, u = L[idx], U[idx]
            raw = implied(mat, l, u, bc.ranges(mat, l, u), rlb, rub)
            NL, NU = round_integers(*raw, is_integer, itol)
            if stats is not None:
                stats["rounded_alone"] = stats.get("rounded_alone", 0) + \
                    int((bits(NL) != bits(raw[0])).sum() + (bits(NU) != bits(raw[1])).sum())
            l2, u2, moved, cross, crossing = apply_round(l, u, NL, NU, tol)
            L[idx], U[idx] = l2, u2
            s["rounds"][idx] = rnd
            s["moves"][idx] += moved.sum(axis=1)
            for i, j in enumerate(idx):
                if crossing[i].any():
                    masked = np.where(crossing[i], cross[i], -INF)
                    s["status"][j] = INFEASIBLE
                    s["worst"][j] = masked.max()
                    s["worst_col"][j] = np.argmax(masked)  # the first: the lowest column
                    active[j] = False
                elif not moved[i].any():
                    s["status"][j] = FIXPOINT
                    active[j] = False
        if rnd in rounds:
            snap = s.copy()
            snap["kept"] = ((bits(L) != bits(L0)) | (bits(U) != bits(U0))).sum(axis=1)
            out[rnd] = (L.copy(), U.copy(), snap)
    return out


def propagate(mat, L, U, rlb, rub, is_integer, tol, itol, max_rounds):
    """(new_lbs, new_ubs, summaries) of the header's rule for the bound sets
    L, U (k, n)."""
    return trace_rounds(mat, L, U, rlb, rub, is_integer, tol, itol, (max_rounds,))[max_rounds]


def _ranges_scalar(mat, l, u):
    """mi_lp_bound_activity_ranges of one set in Python floats."""
    lo, hi = [0.0] * mat.m, [0.0] * mat.m
    lo_inf, hi_inf = [0] * mat.m, [0] * mat.m
    for c in range(mat.n):  # columns ascending: each row's entries in column order
        for i in range(int(mat.col_starts[c]), int(mat.col_starts[c + 1])):
            r, a = int(mat.row_idx[i]), float(mat.vals[i])
            if a == 0.0:
                continue
            bl, bh = (float(l[c]), float(u[c])) if a > 0.0 else (float(u[c]), float(l[c]))
            if np.isinf(bl):
                lo_inf[r] += 1
            else:
                lo[r] += a * bl
            if np.isinf(bh):
                hi_inf[r] += 1
            else:
                hi[r] += a * bh
    return lo, hi, lo_inf, hi_inf


def propagate_scalar(mat, l, u, rlb, rub, is_integer, tol, itol, max_rounds):
    """The header's loop for one bound set in plain Python floats:
    (l, u, status, rounds, moves, worst, worst_col)."""
    l, u = [float(x) for x in l], [float(x) for x in u]
    status, rounds, moves, worst, worst_col = ROUND_LIMIT, 0, 0, 0.0, -1
    for rnd in range(1, max_rounds + 1):
        ref = _ranges_scalar(mat, l, u)
        l2, u2 = list(l), list(u)
        moved_columns, crossing = 0, []
        for c in range(mat.n):
            nl, nu = ic.implied_scalar(mat, l, u, ref, rlb, rub, c)
            if is_integer is not None and is_integer[c]:
                nl = float(np.ceil(nl - itol)) + 0.0
                nu = float(np.floor(nu + itol)) + 0.0
            moved = (nl - l[c] > tol) or (u[c] - nu > tol)
            if moved:
                l2[c], u2[c] = nl, nu
                moved_columns += 1
            cross = l2[c] - u2[c]
            if cross > tol:
                crossing.append((cross, c))
        l, u, rounds = l2, u2, rnd
        moves += moved_columns
        if crossing:
            worst = max(x for x, _ in crossing)
            worst_col = min(c for x, c in crossing if x == worst)
            status = INFEASIBLE
            break
        if moved_columns == 0:
            status = FIXPOINT
            break
    return l, u, status, rounds, moves, worst, worst_col


def changed_reference(NL, NU, base_lb, base_ub, tol):
    """(col_starts (k + 1, int64), cols (int32), new_lbs, new_ubs, kept (k)):
    per set the columns whose final bounds differ in bits from the base, or
    that cross."""
    with np.errstate(invalid="ignore", over="ignore"):
        crossing = NL - NU > tol
    keep = crossing | (bits(NL) != bits(base_lb)[None, :]) | (bits(NU) != bits(base_ub)[None, :])
    k = NL.shape[0]
    col_starts = np.zeros(k + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=col_starts[1:])
    child, col = np.nonzero(keep)
    return col_starts, col.astype(np.int32), NL[child, col], NU[child, col], keep.sum(axis=1)


def list_result(result, base_lb, base_ub, tol):
    """What the lists form returns for the dense reference result: (col_starts,
    cols, new_lbs, new_ubs, summaries) with kept = the list's length."""
    NL, NU, s = result
    col_starts, cols, lo, hi, kept = changed_reference(NL, NU, base_lb, base_ub, tol)
    s = s.copy()
    s["kept"] = kept
    return col_starts, cols, lo, hi, s


# --- hand cases -----------------------------------------------------------------------------------

def _matrix(m, n, entries):
    per_row = [([], []) for _ in range(m)]
    for r, c, a in sorted(entries):
        per_row[r][0].append(c)
        per_row[r][1].append(a)
    return Matrix(m, n, per_row)


@functools.lru_cache(maxsize=None)
def hand(name):
    """(mat, L, U, row_lb, row_ub, is_integer or None) of a hand case."""
    if name == "chain":  # x[i + 1] - x[i] >= 1
        n = 12
        mat = _matrix(n - 1, n, [(i, i, -1.0) for i in range(n - 1)] +
                      [(i, i + 1, 1.0) for i in range(n - 1)])
        L = np.zeros((4, n))
        U = np.repeat(np.array([20.0, 11.0, 10.0, 5.0])[:, None], n, axis=1)
        return mat, L, U, np.ones(n - 1), np.full(n - 1, INF), None
    if name == "halving":  # x - 0.5 y <= 0, y - 0.5 x <= 0
        mat = _matrix(2, 2, [(0, 0, 1.0), (0, 1, -0.5), (1, 0, -0.5), (1, 1, 1.0)])
        return mat, np.zeros((1, 2)), np.ones((1, 2)), np.full(2, -INF), np.zeros(2), None
    if name == "knapsack":  # 3 x + 5 y <= 7, both integer in [0, 10]
        mat = _matrix(1, 2, [(0, 0, 3.0), (0, 1, 5.0)])
        return (mat, np.zeros((1, 2)), np.full((1, 2), 10.0), np.array([-INF]), np.array([7.0]),
                np.array([1, 1], np.uint8))
    assert name == "negzero"  # 2 x >= -1, x integer in [-5, 5]: nl = -0.5, ceil gives -0.0
    mat = _matrix(1, 1, [(0, 0, 2.0)])
    return (mat, np.full((1, 1), -5.0), np.full((1, 1), 5.0), np.array([-1.0]), np.array([INF]),
            np.array([1], np.uint8))


# --- node cases -----------------------------------------------------------------------------------

def integer_columns(name):
    return (np.arange(ic.matrix(name).n) % 3 == 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def node(name, f):
    """(base_lb, base_ub, sets, row_lb, row_ub): CHILDREN override sets
    [(cols int32, new_lbs, new_ubs), ...] and the row bounds, read-only."""
    mat = ic.matrix(name)
    ints = integer_columns(name) != 0
    L, U = ic.pool(name)
    base_lb, base_ub = L[0].copy(), U[0].copy()
    assert np.isfinite(base_lb).all() and np.isfinite(base_ub).all()
    base_lb[ints], base_ub[ints] = np.floor(base_lb[ints]), np.ceil(base_ub[ints])
    x0 = 0.5 * (base_lb + base_ub)
    x0[ints] = np.round(x0[ints])
    lo, hi, lo_inf, hi_inf = bc.ranges(mat, base_lb[None, :], base_ub[None, :])
    assert not lo_inf.any() and not hi_inf.any()
    activity = bc.ranges(mat, x0[None, :], x0[None, :])[0][0]
    w = hi[0] - lo[0]
    r = np.arange(mat.m)
    row_lb, row_ub = np.full(mat.m, -INF), np.full(mat.m, INF)
    upper, lower = np.isin(r % 4, (0, 2)), np.isin(r % 4, (1, 2))
    row_ub[upper] = activity[upper] + f * w[upper]
    row_lb[lower] = activity[lower] - f * w[lower]
    rng = np.random.default_rng(NODE_SEED + len(name))
    candidates = np.arange(mat.n)
    if name == "wide":
        candidates = np.nonzero(ic.column_lengths(name) >= 63)[0]
    width = base_ub - base_lb
    sets = [(np.zeros(0, np.int32), np.zeros(0), np.zeros(0))]
    for j in range(1, CHILDREN):
        cols = np.sort(rng.choice(candidates, 1 + j % 3, replace=False)).astype(np.int32)
        if j % 2 == 0:
            lo_c, hi_c = x0[cols] - 0.05 * width[cols], x0[cols] + 0.05 * width[cols]
            lo_c = np.where(ints[cols], np.ceil(lo_c), lo_c)
            hi_c = np.where(ints[cols], np.floor(hi_c), hi_c)
        else:
            lo_c = x0[cols] + 0.6 * (base_ub[cols] - x0[cols])
            lo_c = np.where(ints[cols], np.ceil(lo_c), lo_c)
            hi_c = base_ub[cols].copy()
        sets.append((cols, lo_c, hi_c))
    for a in (base_lb, base_ub, row_lb, row_ub):
        a.setflags(write=False)
    return base_lb, base_ub, sets, row_lb, row_ub


def node_sets(name, f, k):
    """The first k children, dense: (L, U), each (k, n)."""
    base_lb, base_ub, sets, _, _ = node(name, f)
    return bc.materialise(base_lb, base_ub, sets[:k])


@functools.lru_cache(maxsize=None)
def trace(name, f, tol, integers):
    """{R: (new_lbs, new_ubs, summaries)} of the CHILDREN sets for every R of
    ROUNDS, computed once, read-only; dense-form kept."""
    base_lb, base_ub, sets, row_lb, row_ub = node(name, f)
    L, U = node_sets(name, f, CHILDREN)
    out = trace_rounds(ic.matrix(name), L, U, row_lb, row_ub,
                       integer_columns(name) if integers else None, tol, ITOL, ROUNDS,
                       implied=implied_columns)
    for result in out.values():
        for a in result:
            a.setflags(write=False)
    return out


def expected(name, f, tol, integers, max_rounds, k):
    """The dense result of the first k children."""
    return tuple(a[:k] for a in trace(name, f, tol, integers)[max_rounds])


def expected_lists(name, f, tol, integers, max_rounds, k):
    base_lb, base_ub = node(name, f)[:2]
    return list_result(expected(name, f, tol, integers, max_rounds, k), base_lb, base_ub, tol)


# (f, tolerance): what the tests run per matrix, with and without integers.
GRID = ((0.05, 0.0), (0.05, 1e-9), (0.05, 0.375), (0.15, 0.0))


def grid(name):
    """((f, tolerance, integers), ...) of a matrix: the same eight for all."""
    return tuple((f, tol, integers) for f, tol in GRID for integers in (False, True))


@functools.lru_cache(maxsize=None)
def own_crossing(name):
    """(sets, column): the first four children of node(name, f) for the first
    entry of grid(name), child 2 also given own bounds that cross (l = u + 2)
    in the first column that has entries, that child 2 does not override and
    that the base's first round leaves alone. That column crosses in round 1
    without having moved, beside columns that move: the case in which the
    kept keys' count is not the number of moves."""
    f, tol, integers = grid(name)[0]
    base_lb, base_ub, sets, _, _ = node(name, f)
    after = trace(name, f, tol, integers)[1]
    alone = (bits(after[0][0]) == bits(base_lb)) & (bits(after[1][0]) == bits(base_ub)) & \
        (ic.column_lengths(name) > 0)
    alone[sets[2][0]] = False
    c = int(np.nonzero(alone)[0][0])
    cols, lo, hi = sets[2]
    order = np.argsort(np.append(cols, c))
    child = (np.append(cols, c)[order].astype(np.int32), np.append(lo, base_ub[c] + 2.0)[order],
             np.append(hi, base_ub[c])[order])
    return [sets[0], sets[1], child, sets[3]], c


@functools.lru_cache(maxsize=None)
def own_crossing_reference(name, max_rounds=5):
    f, tol, integers = grid(name)[0]
    base_lb, base_ub, _, row_lb, row_ub = node(name, f)
    sets, _ = own_crossing(name)
    L, U = bc.materialise(base_lb, base_ub, sets)
    out = propagate(ic.matrix(name), L, U, row_lb, row_ub,
                    integer_columns(name) if integers else None, tol, ITOL, max_rounds)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def special_reference(name, which, max_rounds=3):
    """The pool's first 8 children (NaN own bound, l = +inf, +-2^1023, the box)
    of bound_implied_cases under its row-bound set `which`, with integer
    columns."""
    L, U = ic.pool(name)
    out = propagate(ic.matrix(name), L[:8], U[:8], *ic.row_bounds(name, which),
                    integer_columns(name), 0.0, ITOL, max_rounds)
    for a in out:
        a.setflags(write=False)
    return out


# --- comparisons ----------------------------------------------------------------------------------

def same_summaries(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for field in ("status", "rounds", "moves", "worst_col", "kept"):
        assert np.array_equal(got[field], want[field]), (what, field, got[field].tolist(),
                                                         want[field].tolist())
    assert np.array_equal(bits(got["worst"]), bits(want["worst"])), (what, "worst")


def same_result(got, want, what):
    """(new_lbs, new_ubs, summaries) on all 64 bits."""
    ic.same_bounds(got[:2], want[:2], what)
    same_summaries(got[2], want[2], what)


def same_lists(got, want, what):
    """(col_starts, cols, new_lbs, new_ubs, summaries) of the lists form."""
    for g, w, part in zip(got[:4], want[:4], ("col_starts", "cols", "new_lbs", "new_ubs")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, part, g.shape, w.shape)
        if part.startswith("new"):
            assert np.array_equal(bits(g), bits(w)), (what, part)
        else:
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, part)
    same_summaries(got[4], want[4], what)
