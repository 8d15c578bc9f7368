"""The reference of the operation-level device tests (tests/device_ref.py) is
the judge there, so it is checked here against exact arithmetic, without the
engine and without a GPU."""
import functools

import numpy as np
import pytest

import device_cases as dc
from device_ref import (COL_BOXED, COL_CAN_DECREASE, COL_CAN_INCREASE, Matrix, RefState, bits,
                        column_scalar_products)
from exact_bound import within_gamma as _within_gamma


def _row_terms(mat, rows, rho, alg):
    """Per touched position the (multiplier, entry) pairs in filtered-row order
    (algorithm 0 assigns every product: the last one stands)."""
    terms = {}
    for r in rows:
        for c, a in zip(mat.t_cols[r].tolist(), mat.t_vals[r].tolist()):
            if alg == 0:
                terms[c] = [(rho[r], a)]
            else:
                terms.setdefault(c, []).append((rho[r], a))
    return terms


@functools.lru_cache(maxsize=None)
def _ref_after(name):
    """The reference run over the case; per row / column step what it computed."""
    b = dc.build(name)
    ref = RefState(b.mat)
    ref.set_relevant(b.mask)
    out = []
    for st in b.steps:
        if st["kind"] == "row":
            if st["mask"] is not None:
                ref.set_relevant(st["mask"])
            ref.row_wise(st["rows"], st["rho"], st["alg"], dc.DROP)
            out.append((st, ref.last_acc.copy(), ref.last_touched.copy()))
        elif st["kind"] == "col":
            before = ref.coeff.copy()
            ref.column_wise(st["rho"], dc.DROP)
            out.append((st, before, ref.coeff.copy(), ref.relevant.copy(), ref.list.copy()))
    return b, out


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_reference_within_the_dot_product_bound(name):
    """Every position of every row-wise and column-wise step: the reference
    lies within gamma_k * sum |rho_i a_i| of the exact sum of the exact
    products. Derived, not measured; catches a dropped, doubled or mis-signed
    term."""
    b, out = _ref_after(name)
    mat = b.mat
    checked = 0
    for rec in out:
        st = rec[0]
        if st["kind"] == "row":
            _, acc, touched = rec
            terms = _row_terms(mat, st["rows"].tolist(), st["rho"].tolist(), st["alg"])
            assert sorted(terms) == np.nonzero(touched)[0].tolist()
            for c, t in terms.items():
                assert _within_gamma(acc[c], t), (name, c, acc[c], t)
            assert not acc[~touched].any()
            checked += len(terms)
        else:
            _, before, after, relevant, listed = rec
            rel = np.nonzero(relevant)[0]
            dots = column_scalar_products(mat, rel, st["rho"])
            rho = st["rho"].tolist()
            for c, d in zip(rel.tolist(), dots.tolist()):
                s, e = mat.starts[c], mat.starts[c + 1]
                t = [(a, rho[r]) for a, r in zip(mat.c_vals[s:e].tolist(),
                                                 mat.c_rows[s:e].tolist())]
                assert (d == 0.0 and not any(y != 0.0 for _, y in t)) or _within_gamma(d, t), \
                    (name, c, d)
            # Kept columns are written, every other position keeps its value.
            keep = np.zeros(mat.N, bool)
            keep[rel[np.abs(dots) > dc.DROP]] = True
            assert np.array_equal(np.nonzero(keep)[0], listed)
            assert np.array_equal(bits(after[keep]), bits(dots[keep[rel]]))
            assert np.array_equal(bits(after[~keep]), bits(before[~keep]))
            checked += len(rel)
    assert checked > 0


def _order_sensitive(mat, st):
    """(positions with three or more products, how many of them change bits
    when the rows are applied in reversed order) -- on the reference alone."""
    fwd, rev = RefState(mat), RefState(mat)
    fwd.row_wise(st["rows"], st["rho"], st["alg"], dc.DROP)
    rev.row_wise(st["rows"][::-1], st["rho"], st["alg"], dc.DROP)
    count = np.zeros(mat.N, np.int64)
    for r in st["rows"]:
        count[mat.t_cols[r]] += 1
    many = count >= 3
    changed = bits(fwd.last_acc[many]) != bits(rev.last_acc[many])
    return int(many.sum()), int(changed.sum())


def _has_multi_row_step(name):
    return any(st["kind"] == "row" and len(st["rows"]) >= 3 and st["alg"] != 0 and
               st["path"] is not None for st in dc.build(name).steps)


@pytest.mark.parametrize("name", [n for n in sorted(dc.CASES) if _has_multi_row_step(n)])
def test_row_order_matters_in_every_case(name):
    """A kernel that adds a position's products in another order must not
    pass: every case with a step of three or more filtered rows (algorithms 1
    and 2; algorithm 0 adds nothing) has a step with at least 50 positions of
    three or more products, of which at least 20 % change bits when the rows
    are applied in reversed order. The slack-only steps (k entries in k rows:
    no position gets two products) and the steps built around one special
    position cannot meet that themselves; they share their case, matrix and
    kernel path with a step that does."""
    b, _ = _ref_after(name)
    steps = [st for st in b.steps
             if st["kind"] == "row" and len(st["rows"]) >= 3 and st["alg"] != 0]
    best = (0, 0)
    for st in steps:
        if st["path"] is None:
            continue
        many, changed = _order_sensitive(b.mat, st)
        if many >= 50 and changed >= 0.2 * many:
            best = max(best, (many, changed))
    print(name, "positions with >= 3 products:", best[0], "order-sensitive:", best[1])
    assert best[0] >= 50, name


def test_dual_ratio_reference_on_six_hand_worked_breakpoints():
    """sign +, threshold 1e-9, harris tolerance 0.5, minimum delta 0.25,
    variation 10. List slots (column, coefficient, bits, rc, upper - lower):

      slot 0: col 0, coeff 1e-10 -> below the threshold: not eligible
      slot 1: col 1, coeff 2, bits 0 -> may not move: not eligible
      slot 2: col 2, coeff 2, can decrease + boxed, rc -2, diff 1
              ratio 1, harris max(.125, 1 + .25) = 1.25, delta 2 < 10: flips
      slot 3: col 3, coeff -4, can increase + boxed, rc 8, diff 100
              ratio 2, harris 2.125, delta 400 >= 10: sets the bound
      slot 4: col 4, coeff 1, can decrease, rc -3 -> ratio 3, harris 3.5:
              not boxed, sets the bound
      slot 5: col 5, coeff 8, can decrease, rc -16 -> ratio 2 (a tie with
              slot 3), harris 2.0625: sets the bound

    B = min(2.125, 3.5, 2.0625) = 2.0625; kept = ratio <= B (1 + 1e-9) =
    slots {2, 3, 5}. Pop order: slot 2 (ratio 1; flips, variation 10 -> 8),
    then ratio 2 by larger magnitude: slot 5 (not boxed: accepted, the bound
    becomes 2.0625, entering), slot 3 (ratio 2 <= 2.0625: popped; boxed, 8 -
    400 < 0: no flip; magnitude 4 < 8: not entering). P = {2, 3, 5}."""
    mat = Matrix(1, 6, [(np.arange(6, dtype=np.int32), np.ones(6))])
    ref = RefState(mat)
    ref.list = np.arange(6, dtype=np.int32)
    ref.vals = np.array([1e-10, 2.0, 2.0, -4.0, 1.0, 8.0])
    dec, inc, box = COL_CAN_DECREASE, COL_CAN_INCREASE, COL_BOXED
    ref.dual_begin(np.array([-1.0, -1.0, -2.0, 8.0, -3.0, -16.0, 0.0]),
                   np.array([dec | inc, 0, dec | box, inc | box, dec, dec, 0], np.uint8),
                   np.array([0.0, 0.0, 1.0, 100.0, 0.0, 0.0, 0.0]))
    bp = ref.breakpoints(1.0, 1e-9, 0.5, 0.25, 10.0)
    assert bp["eligible"].tolist() == [False, False, True, True, True, True]
    assert bp["ratio"][2:].tolist() == [1.0, 2.0, 3.0, 2.0]
    assert bp["harris"][2:].tolist() == [1.25, 2.125, 3.5, 2.0625]
    assert bp["sets_bound"][2:].tolist() == [False, True, True, True]
    B, kept, popped, entering = ref.dual_ratio(1.0, 1e-9, 0.5, 0.25, 10.0)
    assert B == 2.0625
    assert kept.tolist() == [2, 3, 5]
    assert popped.tolist() == [2, 3, 5]
    assert entering == 5
    # The other sign mirrors the coefficients: nothing is eligible any more
    # except where the bits allow the other direction.
    B2, kept2, _, _ = ref.dual_ratio(-1.0, 1e-9, 0.5, 0.25, 10.0)
    assert B2 is None and kept2.tolist() == []
    # No bound-setting breakpoint: everything eligible is kept.
    ref.colbits[[3, 4, 5]] = 0
    B3, kept3, popped3, _ = ref.dual_ratio(1.0, 1e-9, 0.5, 0.25, 10.0)
    assert B3 is None and kept3.tolist() == [2] and popped3.tolist() == [2]
    # Reduced-cost update over the same list: the entering column is skipped.
    ref.update_reduced_costs(0.5, 6, 7.0, 5)
    assert ref.rc.tolist() == [-1.0 + 0.5e-10, 0.0, -1.0, 6.0, -2.5, 0.0, 7.0]
