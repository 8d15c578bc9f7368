"""Glop's dense triangular loops (lp_data/sparse.cc:776-955, restated by
engine/lu.h) written out directly in Python floats: the reference of
tests/test_tri_ref_cpu.py, tests/test_tri_ops_gpu.py and
tests/test_dense_tail_ops_gpu.py.

TEST INFRASTRUCTURE ONLY. Nothing here is shared with kernels/tri_eval.h.
Python floats are IEEE doubles, every operation is rounded once (no
contraction), and `a * b + c * d + e * f + g * h` is evaluated left to right,
which is the grouped sum of the host loops.

The six kinds of engine/device_solver.h run four loops, one function each:
  transpose_lower_solve      kUpperT, kLowerT   entries from the column's end
  transpose_upper_solve      kUpperTUp          entries from the column's start
  lower_solve_starting_at    kLower, kUnitRow   scatter by ascending columns
  upper_solve                kUpper             scatter by descending columns
solve(kind, ...) picks the loop.

A matrix is a Tri: column c holds the entries [starts[c], starts[c + 1]) of
rows / vals (the diagonal apart, in diag), kept as Python lists. `touched`,
when given, is a list of n bools: the loop sets it for every output it wrote
with the result of an arithmetic operation (a subtraction or a division).
"""
import numpy as np

UPPER_T, LOWER, UPPER_T_UP, LOWER_T, UNIT_ROW, UPPER = range(6)
KIND_NAMES = ("upper_t", "lower", "upper_t_up", "lower_t", "unit_row", "upper")
GROUPED = (UPPER_T, UPPER_T_UP, LOWER_T)
SEQUENTIAL = (LOWER, UNIT_ROW, UPPER)
# Kinds whose matrix holds rows > column (the others: rows < column).
ROWS_BELOW = (UPPER_T, LOWER, LOWER_T, UNIT_ROW)


class Tri:
    def __init__(self, n, starts, rows, vals, diag):
        self.n = int(n)
        self.starts = np.ascontiguousarray(starts, dtype=np.int64)
        self.rows = np.ascontiguousarray(rows, dtype=np.int32)
        self.vals = np.ascontiguousarray(vals, dtype=np.float64)
        self.diag = np.ascontiguousarray(diag, dtype=np.float64)
        assert len(self.starts) == self.n + 1 and len(self.diag) == self.n
        assert len(self.rows) == len(self.vals) == int(self.starts[-1])
        # TriangularMatrix::CloseCurrentColumn: the leading columns without
        # entries whose diagonal is 1.0.
        has = (np.diff(self.starts) > 0) | (self.diag != 1.0)
        self.first_non_identity = int(np.argmax(has)) if has.any() else self.n
        self.ones = bool((self.diag == 1.0).all())
        self._lists = None

    def lists(self):
        if self._lists is None:
            self._lists = (self.starts.tolist(), self.rows.tolist(), self.vals.tolist(),
                           self.diag.tolist())
        return self._lists


def transpose_lower_solve(t, x, touched=None):
    """TriangularMatrix::TransposeLowerSolve (sparse.cc:899-955)."""
    st, rows, vals, diag = t.lists()
    x = list(x)
    end = t.first_non_identity
    col = t.n - 1
    while col >= end and x[col] == 0.0:
        col -= 1
    ones = t.ones
    while col >= end:
        s = x[col]
        b = st[col]
        i = st[col + 1] - 1
        while i >= b + 3:
            s -= (vals[i] * x[rows[i]] + vals[i - 1] * x[rows[i - 1]] +
                  vals[i - 2] * x[rows[i - 2]] + vals[i - 3] * x[rows[i - 3]])
            i -= 4
        if i >= b:
            s -= vals[i] * x[rows[i]]
            if i >= b + 1:
                s -= vals[i - 1] * x[rows[i - 1]]
                if i >= b + 2:
                    s -= vals[i - 2] * x[rows[i - 2]]
        x[col] = s if ones else s / diag[col]
        if touched is not None and (not ones or st[col + 1] > b):
            touched[col] = True
        col -= 1
    return x


def transpose_upper_solve(t, x, touched=None):
    """TriangularMatrix::TransposeUpperSolve (sparse.cc:848-897)."""
    st, rows, vals, diag = t.lists()
    x = list(x)
    ones = t.ones
    for col in range(t.first_non_identity, t.n):
        s = x[col]
        i = st[col]
        e = st[col + 1]
        while i < e - 3:
            s -= (vals[i] * x[rows[i]] + vals[i + 1] * x[rows[i + 1]] +
                  vals[i + 2] * x[rows[i + 2]] + vals[i + 3] * x[rows[i + 3]])
            i += 4
        if i < e:
            s -= vals[i] * x[rows[i]]
            if i + 1 < e:
                s -= vals[i + 1] * x[rows[i + 1]]
                if i + 2 < e:
                    s -= vals[i + 2] * x[rows[i + 2]]
        x[col] = s if ones else s / diag[col]
        if touched is not None and (not ones or e > st[col]):
            touched[col] = True
    return x


def lower_solve_starting_at(t, start, x, touched=None):
    """TriangularMatrix::LowerSolveStartingAt (sparse.cc:793-812)."""
    st, rows, vals, diag = t.lists()
    x = list(x)
    ones = t.ones
    for col in range(max(start, t.first_non_identity), t.n):
        value = x[col]
        if value == 0.0:
            continue
        coeff = value if ones else value / diag[col]
        if not ones:
            x[col] = coeff
            if touched is not None:
                touched[col] = True
        for i in range(st[col], st[col + 1]):
            x[rows[i]] -= coeff * vals[i]
            if touched is not None:
                touched[rows[i]] = True
    return x


def upper_solve(t, x, touched=None):
    """TriangularMatrix::UpperSolve (sparse.cc:814-846)."""
    st, rows, vals, diag = t.lists()
    x = list(x)
    ones = t.ones
    for col in range(t.n - 1, t.first_non_identity - 1, -1):
        value = x[col]
        if value == 0.0:
            continue
        coeff = value if ones else value / diag[col]
        if not ones:
            x[col] = coeff
            if touched is not None:
                touched[col] = True
        for i in range(st[col + 1] - 1, st[col] - 1, -1):
            x[rows[i]] -= coeff * vals[i]
            if touched is not None:
                touched[rows[i]] = True
    return x


def solve(kind, t, x, start=0, touched=None):
    """The host loop of `kind` on x (any sequence of n floats); returns a
    float64 array."""
    x = np.asarray(x, np.float64).tolist()
    if kind in (UPPER_T, LOWER_T):
        out = transpose_lower_solve(t, x, touched)
    elif kind == UPPER_T_UP:
        out = transpose_upper_solve(t, x, touched)
    elif kind in (LOWER, UNIT_ROW):
        out = lower_solve_starting_at(t, start, x, touched)
    else:
        assert kind == UPPER
        out = upper_solve(t, x, touched)
    return np.array(out, np.float64)


def top_row(kind, t, x):
    """The last row a device solve computes (DeviceLp::TriBegin): the last
    non-zero for the TransposeLowerSolve kinds, else n - 1; below the
    schedule's first output when there is nothing to compute."""
    top = t.n - 1
    if kind in (UPPER_T, LOWER_T):
        while top >= t.first_non_identity and x[top] == 0.0:
            top -= 1
    return top


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
