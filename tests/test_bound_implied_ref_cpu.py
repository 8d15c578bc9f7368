"""The reference and the inputs of the implied-column-bound tests
(tests/bound_implied_cases.py), checked without a GPU: the vectorised
reference against the header's loop in plain floats, that the result does not
depend on the order of a column's entries (and that it would without the
q + 0.0 step), candidates against the same formula in exact rationals, the
keep rule and the summaries against a straightforward loop, that an override
list re-applied to the base reproduces the result, that the inputs exercise
every branch of the rule, and cpsat.tightened_overrides.
"""
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest

import bound_implied_cases as ic
import bound_range_cases as bc
from device_ref import Matrix, bits
from mi_glop import cpsat

U53 = Fraction(1, 2 ** 53)
TINY = Fraction(1, 2 ** 1075)  # half the smallest subnormal


def test_wide_is_what_the_header_says():
    mat = ic.matrix("wide")
    lens = ic.column_lengths("wide")
    assert (mat.m, mat.n) == (ic.WIDE_M, ic.WIDE_N) == (320, 700)
    assert set(ic.WIDE_LENS) <= set(lens.tolist())
    g = bc.GATHER
    assert {0, 1, g - 1, g, g + 1, 2 * g - 1, 2 * g, 2 * g + 1} <= set(lens.tolist())
    for k in (1, 4, 16):  # one below, at and one above a slice round of the long shape
        slices = 256 // k
        assert {slices - 1, slices, slices + 1} <= set(lens.tolist()), k
    assert mat.m in lens
    assert mat.n // 256 == 2 and mat.n % 256 != 0  # two full filter tiles and a partial one
    for name in ic.CASES:  # a partial last workgroup at 256, 64 and 16 columns per workgroup
        n = ic.matrix(name).n
        assert all(n % cols != 0 for cols in (256, 64, 16)), name
        assert ic.long_by_itself(name) == (name == "wide")


@pytest.mark.parametrize("name", ic.CASES)
def test_reference_against_the_loop(name):
    """implied() equals implied_scalar(), the header's loop in Python floats,
    on every bit: all columns of the small matrices, a sample of `wide`."""
    mat = ic.matrix(name)
    L, U = ic.pool(name)
    ref = ic.ranges_reference(name)
    rng = np.random.default_rng(3)
    cols = range(mat.n) if name != "wide" else np.unique(
        np.concatenate([np.arange(15), rng.integers(0, mat.n, 40)]))
    children = range(ic.POOL) if name != "rows70" else (0, 1, 2, 3, 6, 7, 16, 25, 32)
    for which in ic.ROW_BOUND_SETS:
        lb, ub = ic.row_bounds(name, which)
        NL, NU = ic.reference(name, which)
        for j in children:
            ref_j = tuple(a[j] for a in ref)
            for c in cols:
                nl, nu = ic.implied_scalar(mat, L[j], U[j], ref_j, lb, ub, c)
                assert bits(nl) == bits(NL[j, c]) and bits(nu) == bits(NU[j, c]), \
                    (name, which, j, c)


@pytest.mark.parametrize("name", ic.CASES)
def test_entry_order_does_not_change_bits(name):
    mat = ic.matrix(name)
    L, U = ic.pool(name)
    ref = ic.ranges_reference(name)
    want = ic.reference(name, "mid")
    for order in ("reversed", 1, 2):
        got = ic.implied(mat, L, U, ref, *ic.row_bounds(name, "mid"), order=order)
        ic.same_bounds(got, want, f"{name} order {order}")


def test_without_normalising_zero_the_order_shows():
    """A column with a +0.0 and a -0.0 candidate for the same bound: with the
    q + 0.0 step both orders give +0.0; without it the first one met stays,
    since neither is larger than the other."""
    # x in [-1, 1]; rows 0 and 1 both say a x >= 0, once with a > 0 (q = +0.0 /
    # a = +0.0) and once with a < 0 (q = +0.0 / a = -0.0).
    mat = Matrix(2, 1, [([0], [2.0]), ([0], [-2.0])])
    L, U = np.array([[-1.0]]), np.array([[1.0]])
    ref = bc.ranges(mat, L, U)
    assert ref[0].tolist() == [[-2.0, -2.0]] and ref[1].tolist() == [[2.0, 2.0]]
    # Row 0: lb = hi - a u = 0 -> q = (0 - 0) / 2 = +0.0 tightens the lower
    # bound. Row 1: ub = lo - a u... a < 0: the lo side fed u; ub = -2 + 2 = 0
    # -> q = (0 - 0) / -2 = -0.0 tightens the lower bound too.
    rlb = np.array([0.0, -np.inf])
    rub = np.array([np.inf, 0.0])
    results = {}
    for normalise in (True, False):
        for order in (None, "reversed"):
            NL, NU = ic.implied(mat, L, U, ref, rlb, rub, order=order, normalise=normalise)
            assert NU[0, 0] == 1.0 and NL[0, 0] == 0.0
            results[normalise, order] = int(bits(NL)[0, 0])
            nl, _ = ic.implied_scalar(mat, L[0], U[0], tuple(a[0] for a in ref), rlb, rub, 0,
                                      normalise=normalise)
            if order is None:
                assert int(bits(nl)[0]) == results[normalise, order]
    assert results[True, None] == results[True, "reversed"] == int(bits(0.0)[0])
    assert results[False, None] != results[False, "reversed"]
    assert {results[False, None], results[False, "reversed"]} == {int(bits(0.0)[0]),
                                                                  int(bits(-0.0)[0])}


def _exact_sum_bound(terms):
    """(S, E): the exact sum of the products and exact_bound.within_gamma's
    bound on a k-term sum of them in any order, gamma_k sum |product| +
    k 2^-1075 / (1 - k u), as exact rationals."""
    k = len(terms)
    prods = [Fraction(a) * Fraction(b) for a, b in terms]
    if k == 0:
        return Fraction(0), Fraction(0)
    gamma = k * U53 / (1 - k * U53)
    return sum(prods), gamma * sum(abs(p) for p in prods) + k * TINY / (1 - k * U53)


@pytest.mark.parametrize("name", ic.CASES)
def test_candidates_against_exact_rationals(name):
    """On a sample of finite candidates: q against (rb - (S - a b)) / a, or
    (rb - S) / a where the column's own term is the infinite one, with S the
    exact sum of the finite terms of the range. The allowed error is derived,
    not tuned. With s the rounded range sum, |s - S| <= E (exact_bound's
    bound: a k-term sum in any order). Every later operation is one rounding,
    |fl(x) - x| <= u |fl(x)|, plus 2^-1075 where it may underflow: p =
    fl(a b), res = fl(s - p), d = fl(rb - res), q = fl(d / a). Hence
      |q - q_exact| <= u |q| + 2^-1075
                       + (u |d| + u |res| + u |p| + 2^-1075 + E) / |a|
    where the p and res terms fall away when the own term is not subtracted."""
    mat = ic.matrix(name)
    L, U = ic.pool(name)
    ref = ic.ranges_reference(name)
    lb, ub = ic.row_bounds(name, "mid")
    rng = np.random.default_rng(17)
    checked = Counter()
    # Every other draw is a (child, column) pair whose own bound is infinite:
    # the cnt == 1 branch is rare among all pairs.
    infinite = np.argwhere(np.isinf(L) | np.isinf(U))
    for attempt in range(6000):
        if min(checked["subtracted"], checked["own_infinite"]) >= 40:
            break
        if attempt % 2 == 0:
            j, c = int(rng.integers(0, ic.POOL)), int(rng.integers(0, mat.n))
        else:
            j, c = (int(x) for x in infinite[int(rng.integers(0, len(infinite)))])
        found = []
        ic.implied_scalar(mat, L[j], U[j], tuple(a[j] for a in ref), lb, ub, c, candidates=found)
        if not found:
            continue
        if attempt % 2 == 1:
            found = [f for f in found if f[4] == 1] or found
        r, a, rb, s, cnt, b, q, tightens_upper = found[int(rng.integers(0, len(found)))]
        lo_side = tightens_upper == (a > 0.0)  # the lo side tightens the upper bound iff a > 0
        terms = []
        for col, coeff in zip(mat.t_cols[r][:-1], mat.t_vals[r][:-1]):
            picks = (L[j, col], U[j, col]) if coeff > 0.0 else (U[j, col], L[j, col])
            bound = picks[0] if lo_side else picks[1]
            if not np.isinf(bound):
                terms.append((float(coeff), float(bound)))
        if not all(np.isfinite(x) for _, x in terms):
            continue  # a NaN bound: no exact value to compare with
        S, E = _exact_sum_bound(terms)
        A = Fraction(a)
        if cnt == 0:
            p = a * b
            res = s - p
            exact_q = (Fraction(rb) - (S - A * Fraction(b))) / A
            slack = U53 * abs(Fraction(res)) + U53 * abs(Fraction(p)) + TINY
            checked["subtracted"] += 1
        else:
            assert cnt == 1 and np.isinf(b)
            res = s
            exact_q = (Fraction(rb) - S) / A
            slack = Fraction(0)
            checked["own_infinite"] += 1
        d = rb - res
        allowed = U53 * abs(Fraction(q)) + TINY + (U53 * abs(Fraction(d)) + slack + E) / abs(A)
        assert abs(Fraction(q) - exact_q) <= allowed, (name, j, c, r, float(exact_q), q)
    print(name, dict(checked))
    assert checked["subtracted"] >= 40 and checked["own_infinite"] >= 40, (name, checked)


def _keep_loop(L, U, NL, NU, tol, base):
    """The keep rule and the summaries, one (child, column) at a time."""
    k, n = L.shape
    starts, cols, lo, hi, summaries = [0], [], [], [], []
    for j in range(k):
        count, worst, worst_col = 0, 0.0, -1
        for c in range(n):
            l, u, nl, nu = (float(x[j, c]) for x in (L, U, NL, NU))
            moved = (nl - l > tol) or (u - nu > tol)
            cross = nl - nu
            crossing = cross > tol
            changed = base is not None and (bits(l) != bits(base[0][c]) or
                                            bits(u) != bits(base[1][c]))
            if crossing and cross > worst:
                worst, worst_col = cross, c
            if moved or crossing or changed:
                count += 1
                cols.append(c)
                lo.append(nl)
                hi.append(nu)
        starts.append(len(cols))
        summaries.append((count, worst, worst_col))
    return starts, cols, lo, hi, summaries


@pytest.mark.parametrize("name", ic.CASES)
def test_keep_rule_and_summaries_against_a_loop(name):
    L, U = ic.pool(name)
    k = 33 if name != "wide" else 8
    with np.errstate(invalid="ignore", over="ignore"):
        for which in ic.ROW_BOUND_SETS:
            NL, NU = ic.first(ic.reference(name, which), k)
            for tol in ic.tolerances(name):
                for base in (None, (L[0], U[0])):
                    got = ic.keep_reference(L[:k], U[:k], NL, NU, tol, base=base)
                    starts, cols, lo, hi, summaries = _keep_loop(L[:k], U[:k], NL, NU, tol, base)
                    what = (name, which, tol, base is not None)
                    assert got[0].tolist() == starts and got[1].tolist() == cols, what
                    assert np.array_equal(bits(got[2]), bits(np.array(lo, np.float64))), what
                    assert np.array_equal(bits(got[3]), bits(np.array(hi, np.float64))), what
                    for j, (count, worst, worst_col) in enumerate(summaries):
                        s = got[4][j]
                        assert (s["count"], s["worst_row"]) == (count, worst_col), (what, j)
                        assert bits(s["worst"]) == bits(worst), (what, j)
                    if base is not None:  # child 0 is the base: nothing changed in it
                        assert got[4]["count"][0] == ic.keep_reference(
                            L[:1], U[:1], NL[:1], NU[:1], tol)[4]["count"][0]


@pytest.mark.parametrize("name", ic.CASES)
def test_override_list_reapplied_reproduces_the_result(name):
    """The override form's list, as overrides of the base, is (new_lbs,
    new_ubs) in bits, at every tolerance: what is not listed kept the base's
    bounds."""
    L, U = ic.pool(name)
    k = 17
    NL, NU = ic.first(ic.reference(name, "mid"), k)
    for tol in ic.tolerances(name):
        result = ic.keep_reference(L[:k], U[:k], NL, NU, tol, base=(L[0], U[0]))
        sets = cpsat.tightened_overrides(result)
        assert len(sets) == k
        gotL, gotU = bc.materialise(L[0], U[0], sets)
        kept = np.zeros(NL.shape, bool)
        for j, (cols, _, _) in enumerate(sets):
            kept[j, cols] = True
        # A kept column carries its implied bounds; any other one moved by at
        # most tol from own bounds that are the base's.
        assert np.array_equal(bits(gotL[kept]), bits(NL[kept])), (name, tol)
        assert np.array_equal(bits(gotU[kept]), bits(NU[kept])), (name, tol)
        assert np.array_equal(bits(gotL[~kept]), bits(L[:k][~kept])), (name, tol)
        assert np.array_equal(bits(gotU[~kept]), bits(U[:k][~kept])), (name, tol)
        if tol == 0.0:
            # At tolerance 0 only columns with NaN or infinite differences can
            # be left out while they differ from their own bounds.
            differ = (bits(gotL) != bits(NL)) | (bits(gotU) != bits(NU))
            with np.errstate(invalid="ignore", over="ignore"):
                odd = ~np.isfinite(NL - L[:k]) | ~np.isfinite(U[:k] - NU)
            assert not (differ & ~odd).any(), name


# A prototype of the header's formula gives, under `mid` over the 33 children
# (the same at tolerances 0 and 0.375):
#   kept columns per child   rows70 3..230 of 230, steps 3..29 of 30, groups
#                            5..30 of 30, wide 0..632 of 700
#   candidates through the cnt == 1 branch (finite q)   220, 225, 180, 3161
#   discarded non-finite q                              2521, 314, 373, 30976
#   sides skipped for other infinite bounds             29150, 2685, 2581, 457030
#   columns taken from an infinite to a finite bound    lower 24, 14, 16, 25;
#                                                       upper 20, 29, 27, 19
@pytest.mark.parametrize("name", ic.CASES)
def test_inputs_exercise_the_rule(name):
    mat = ic.matrix(name)
    L, U = ic.pool(name)
    stats = Counter()
    NL, NU = ic.implied(mat, L, U, ic.ranges_reference(name), *ic.row_bounds(name, "mid"),
                        stats=stats)
    ic.same_bounds((NL, NU), ic.reference(name, "mid"), name)
    print(name, dict(stats))
    for kind in ("own_infinite", "non_finite_q", "other_infinite", "lower_from_infinite",
                 "upper_from_infinite"):
        assert stats[kind] >= 1, (name, kind)
    ok = ~np.isnan(L) & ~np.isnan(U)
    assert np.all(NL[ok] >= L[ok]) and np.all(NU[ok] <= U[ok])
    assert np.isnan(NL[bc.WITH_NAN]).sum() == 1  # a NaN own bound stays NaN
    for tol in ic.TOLERANCES:
        summaries = ic.expected(name, "mid", ic.POOL, tol)[4]
        kept = summaries["count"]
        print(name, tol, "kept per child", int(kept.min()), "to", int(kept.max()), "of", mat.n)
        # groups' lowest child keeps 5 of 30 columns (one in six): its pool and
        # the row bounds are given, so that is its low end.
        low = 0.10 if name != "groups" else 1 / 6
        assert kept.min() <= low * mat.n and kept.max() >= 0.85 * mat.n, (name, tol)
        assert (summaries["worst_row"] >= 0).any() and (summaries["worst_row"] < 0).any()
        # count > 0 without a crossing column, the ordinary case of the fold:
        # in the dense form, or (wide, where every child that keeps a column
        # also crosses) in the override form without finite row bounds.
        lone = (kept > 0) & (summaries["worst_row"] < 0)
        if name == "wide":
            free = ic.keep_reference(L, U, *ic.reference(name, "free"), tol, base=(L[0], U[0]))[4]
            lone = (free["count"] > 0) & (free["worst_row"] < 0)
        assert lone.any(), (name, tol)
        # Within every panel of every k something is kept and something is not.
        for k in ic.KS:
            for first, count in bc.rc.panels(k):
                part = kept[first:first + count]
                assert part.sum() > 0 and part.sum() < count * mat.n, (name, k, first)
    for which in ("free", "crossed"):  # no finite row bound: no candidate
        ic.same_bounds(ic.reference(name, which), (L, U), f"{name} {which}")
        s = ic.expected(name, which, ic.POOL, 0.0)[4]
        # l = +inf > u is kept as crossing with worst = +inf, unless the pool
        # also drew u = +inf for that column (inf - inf: not crossing).
        if np.isfinite(U[bc.WRONG_INF, bc.most_held(mat)[0]]):
            assert s["worst"][bc.WRONG_INF] == np.inf and s["count"][bc.WRONG_INF] == 1
        else:
            assert name == "steps" and s["count"][bc.WRONG_INF] == 0
        assert s["count"][bc.WITH_NAN] == 0 and s["count"][bc.HUGE] == 0


@pytest.mark.parametrize("name", ic.CASES)
def test_edge_tolerances(name):
    tol, c = ic.edge(name)
    L, U = ic.pool(name)
    NL, NU = ic.reference(name, "mid")
    assert tol > 0.0 and bits(NL[0, c] - L[0, c]) == bits(tol)
    at = ic.expected(name, "mid", 1, tol)
    below = ic.expected(name, "mid", 1, float(np.nextafter(tol, 0.0)))
    assert c not in at[1].tolist() and c in below[1].tolist()


def test_tightened_overrides():
    starts = np.array([0, 2, 2, 3], np.int64)
    cols = np.array([4, 9, 1], np.int32)
    lo, hi = np.array([0.5, -1.0, 2.0]), np.array([1.5, np.inf, 2.0])
    sets = cpsat.tightened_overrides((starts, cols, lo, hi, None))
    assert [c.tolist() for c, _, _ in sets] == [[4, 9], [], [1]]
    assert [x.tolist() for _, x, _ in sets] == [[0.5, -1.0], [], [2.0]]
    assert [x.tolist() for _, _, x in sets] == [[1.5, np.inf], [], [2.0]]
    with pytest.raises(ValueError):
        cpsat.tightened_overrides((None, None, None, None, np.zeros(3)))
