"""The reference of tests/test_solveops_gpu.py (pricing, row sums, column
norms, boxed flips in tests/device_ref.py) and its inputs
(tests/solveops_cases.py), judged without the engine and without a GPU.

- Every reference value lies within the k-term dot-product bound of the exact
  sum of its exact products (tests/exact_bound.py): a dropped, doubled or
  mis-signed term does not pass.
- The inputs tell summation orders apart: a bit-for-bit comparison shows
  nothing if every order gives the same bits. In every length class that has
  two orders to tell apart, at least one column (row) changes bits.
- The flip rule on a hand-worked table.
"""
import numpy as np
import pytest

import solveops_cases as sc
from device_ref import RefState, bits, column_scalar_products
from exact_bound import is_one_rounding, within_gamma

PRICING = ("quad", "wave") + tuple(f"dense{m}" for m in sc.OLD_DENSE + sc.NEW_DENSE)
NORMS = ("quad", "wave", "rows70", "wide")
ROW_SUMS = ("rows70", "wide")


def _column_terms(mat, c, y):
    s, e = mat.starts[c], mat.starts[c + 1]
    return [(a, y[r]) for a, r in zip(mat.c_vals[s:e].tolist(), mat.c_rows[s:e].tolist())]


@pytest.mark.parametrize("name", PRICING)
def test_pricing_within_the_dot_product_bound(name):
    """The dot against the bound; then rc = c - dot as one exact rounding. The
    list dots of the fused call are the same function with w."""
    mat, p = sc.matrix(name), sc.pricing_inputs(name)
    ref = RefState(mat)
    cols = np.arange(mat.N)
    for v in (p["y"], p["w"]):
        dots = column_scalar_products(mat, cols, v)
        rc = ref.pricing(p["c"], v)
        yl = v.tolist()
        for c in cols.tolist():
            t = _column_terms(mat, c, yl)
            d = float(dots[c])
            assert (d == 0.0 and not any(b != 0.0 for _, b in t)) or within_gamma(d, t), (name, c)
            if np.isfinite(p["c"][c]):
                assert is_one_rounding(float(rc[c]), float(p["c"][c]), d), (name, c)
    assert np.isnan(rc[2]) and np.isinf(rc[1])


@pytest.mark.parametrize("name", PRICING)
def test_pricing_inputs_tell_orders_apart(name):
    """Each vector that the device test runs on this matrix, on its own: y
    (plain pricing, the rc of fused pricing), w (the list dots of fused
    pricing, and plain pricing) and rho (the update rows, and the second
    vector of one fused call). Against a left-to-right sum for every column
    length of at least 8 (up to 7 entries each of the four chains holds one
    product and the orders coincide), against the fold (r1 + r2) + (r3 + r4)
    for every length of at least 5: in every such class at least one column
    changes bits."""
    mat, p = sc.matrix(name), sc.pricing_inputs(name)
    for key in ("y", "w", "rho"):
        assert sc.orders_not_told_apart(mat, p[key]) == [], (name, key)
    assert name == "dense5" or (mat.col_len >= 8).any()


def _row_terms(mat, r, x, skip, sign):
    return [(sign * x[c], a) for c, a in zip(mat.t_cols[r].tolist(), mat.t_vals[r].tolist())
            if not skip[c] and sign * x[c] != 0.0]


@pytest.mark.parametrize("name", ROW_SUMS)
def test_row_sums_within_the_dot_product_bound(name):
    mat, p = sc.matrix(name), sc.row_sum_inputs(name)
    ref = RefState(mat)
    none = np.zeros(mat.N, bool)
    for sign in (1.0, -1.0):
        for skip in (none, p["basic"], p["basic3"], p["flipped"]):
            out = ref.row_sums(p["x"], skip, sign)
            xl = p["x"].tolist()
            for r in range(mat.m):
                t = _row_terms(mat, r, xl, skip, sign)
                assert (len(t) == 0 and bits(out[r]) == 0) or within_gamma(float(out[r]), t), \
                    (name, r)
    if name == "rows70":
        # Live multipliers all zero: +0.0, also with sign -1.
        r = sc.ROWS70_ZERO_ROW
        assert bits(ref.row_sums(p["x"], None, -1.0)[r]) == 0
        assert np.all(bits(p["x"][mat.t_cols[r]]) == bits(np.array([0.0, -0.0])))
    # The NaN and the inf reach every row holding their column, and no other.
    for key, test in (("x_nan", np.isnan), ("x_inf", np.isinf)):
        col = int(np.nonzero(bits(p[key]) != bits(p["x"]))[0][0])
        out = ref.row_sums(p[key], None, 1.0)
        holds = np.array([col in c for c in mat.t_cols])
        assert holds.sum() >= 2 and np.array_equal(test(out), holds), (name, key)


@pytest.mark.parametrize("name", ROW_SUMS)
def test_row_sum_inputs_tell_orders_apart(name):
    """Against the entries taken last to first, in every class of row length
    with at least 3 entries."""
    mat, p = sc.matrix(name), sc.row_sum_inputs(name)
    ref = RefState(mat)
    fwd = [ref.row_sums(p["x"], skip, sign) for sign in (1.0, -1.0) for skip in (None, p["basic"])]
    rev = [sc.row_sums_reversed(mat, p["x"], skip, sign)
           for sign in (1.0, -1.0) for skip in (None, p["basic"])]
    changed = np.any(bits(np.stack(fwd)) != bits(np.stack(rev)), axis=0)
    classes = [L for L in np.unique(mat.row_len) if L >= 3]
    assert classes
    for L in classes:
        rows = mat.row_len == L
        print(name, "row length", L, "rows", rows.sum(), "changed", changed[rows].sum())
        assert changed[rows].any(), (name, L)


@pytest.mark.parametrize("name", NORMS)
def test_norms_within_the_bound_and_tell_orders_apart(name):
    """1 + sum v v: the squares and the 1.0 as k + 1 terms. Against the
    four-chain order of ColumnScalarProduct for every column length of at
    least 8 (up to 7 entries both orders are the same additions)."""
    mat, mask = sc.matrix(name), sc.relevant_mask(name)
    ref = RefState(mat)
    ref.set_relevant(mask)
    out = ref.column_squared_norms()
    assert np.array_equal(np.isnan(out), ~mask)
    off = 64 * sc.OFF_WORD.get(name, 1)
    assert mask[0] and mask[mat.N - 1] and not mask[off:off + 64].any()
    assert mask[:off].any() and mask[off + 64:].any()
    rel = np.nonzero(mask)[0]
    for c in rel.tolist():
        v = mat.c_vals[mat.starts[c]:mat.starts[c + 1]].tolist()
        assert within_gamma(float(out[c]), [(a, a) for a in v] + [(1.0, 1.0)]), (name, c)
    empty = rel[mat.col_len[rel] == 0]
    assert np.all(out[empty] == 1.0)
    for L in np.unique(mat.col_len[rel]):
        if L < 8:
            continue
        cols = rel[mat.col_len[rel] == L]
        changed = int(np.sum(bits(out[cols]) != bits(sc.norms_four_chains(mat, cols))))
        print(name, "length", L, "columns", len(cols), "changed", changed)
        assert changed > 0, (name, L)


def test_norm_lengths_present():
    """Every length around the kernel's 64-entry steps is among the relevant
    columns of the norm cases (all of them on wave)."""
    mat, mask = sc.matrix("wave"), sc.relevant_mask("wave")
    assert set(sc.NORM_LENGTHS) <= set(mat.col_len[mask].tolist())


def test_case_shapes():
    for u, ms in sc.DENSE_UNROLL_ROWS.items():
        for m in ms:
            mat = sc.matrix(f"dense{m}")
            full = mat.col_len[:mat.n] == m
            assert full.sum() == 70 and (m >> 3) >= u  # the unrolled loop runs
            assert mat.col_len[~np.concatenate([full, np.zeros(m, bool)])].mean() < 32
    mat = sc.matrix("rows70")
    assert mat.m == 70 and mat.n >= 199 and tuple(mat.row_len) == sc.ROWS70_LENS
    assert set(mat.row_len[:32]) == {1, 2, 63, 64, 65, 128, 129, 200}
    assert set(mat.row_len[32:64]) == {1} and len(mat.row_len[64:]) == 6
    wide = sc.matrix("wide")
    assert wide.N >= 33000 and wide.m == 40 and set(wide.col_len[:wide.n]) == {1, 2}
    words = (wide.N + 63) // 64
    assert words > 512
    p = sc.row_sum_inputs("wide")
    assert sc.changed_words(p["basic"], p["flipped"]) == words
    mask = sc.relevant_mask("wide")
    assert sc.changed_words(mask, sc.relevant_flipped("wide")) == words
    small = sc.row_sum_inputs("rows70")
    assert sc.changed_words(small["basic"], small["basic3"]) == 3
    for name in ("rows70", "wide"):
        x = sc.row_sum_inputs(name)["x"]
        zero = x == 0.0
        assert 0.05 < np.mean(zero & ~np.signbit(x)) < 0.15 and 0.005 < np.mean(
            zero & np.signbit(x)) < 0.04, name


def test_flip_rule_on_the_hand_worked_table():
    """Each row of FLIP_TABLE alone: threshold, rc, the column's byte, and
    whether it flips without a list (the boxed bit decides) and in a list."""
    mat = sc.matrix("quad")
    for i, (threshold, rc, byte, full, listed) in enumerate(sc.FLIP_TABLE):
        ref = RefState(mat)
        col = (7 * i + 3) % mat.N
        rcs = np.zeros(mat.N)
        colbits = np.zeros(mat.N, np.uint8)
        rcs[col], colbits[col] = rc, byte
        ref.dual_begin(rcs, colbits, np.ones(mat.N))
        got = ref.boxed_flips(None, threshold)
        assert got.dtype == np.uint8 and got[col] == full and got.sum() == full, (i, got[col])
        got = ref.boxed_flips([col, (col + 1) % mat.N], threshold)
        assert got.tolist() == [listed, 0], (i, got)
    table = sc.FLIP_TABLE
    assert {t[0] for t in table} == {0.5, 0.0}
    assert any(t[1] == t[0] and not t[3] for t in table)
    assert any(t[1] == -t[0] and t[0] > 0 and not t[3] for t in table)
    assert any(np.isnan(t[1]) for t in table) and any(np.isinf(t[1]) and t[3] for t in table)
    assert any(t[4] and not t[3] for t in table)  # the boxed bit matters only without a list
    assert {(t[2] >> 3) & 7 for t in table} >= {0, 1, 2, 3, 4, 7}


def test_take_and_set_reduced_costs():
    mat, p = sc.matrix("quad"), sc.pricing_inputs("quad")
    ref = RefState(mat)
    ref.dual_begin(np.zeros(mat.N), np.zeros(mat.N, np.uint8), np.zeros(mat.N))
    rc = ref.pricing(p["c"], p["y"])
    ref.take_priced()
    assert np.array_equal(bits(ref.rc), bits(rc))
    ref.set_reduced_cost(mat.n, -0.0)
    assert bits(ref.rc[mat.n]) == bits(-0.0) and np.array_equal(
        bits(np.delete(ref.rc, mat.n)), bits(np.delete(rc, mat.n)))
    rc2, dots = ref.pricing_with_dots(p["c"], p["y"], p["w"])
    assert np.array_equal(bits(rc2), bits(rc)) and len(dots) == len(ref.list) == 0
