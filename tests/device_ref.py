"""Plain numpy reference of single DeviceLp operations.

TEST INFRASTRUCTURE ONLY. Pure Python/numpy, no C: it cannot share a mistake
with the engine. RefState holds what the device holds between operations: the
coefficient array, the last list, rc / colbits / bound_diff, the relevant mask
and the last pricing result. Every product is one IEEE double multiplication
and every sum one IEEE addition in the order the operation defines (numpy
element-wise arithmetic does not fuse), so results are compared with the
device on bit patterns.
"""
import numpy as np

COL_CAN_DECREASE, COL_CAN_INCREASE, COL_BOXED = 1, 2, 4
# glop::VariableStatus in bits 3-5 of a column's byte (lp_types.h:188-219).
STATUS_SHIFT, STATUS_AT_LOWER, STATUS_AT_UPPER = 3, 2, 3


def bits(a):
    """The 64-bit patterns of a float64 array (-0.0 != +0.0, NaN never equal
    by accident)."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Matrix:
    """[A | I]: A is m x n, given by rows (sorted unique columns < n)."""

    def __init__(self, m, n, rows):
        self.m, self.n, self.N = m, n, n + m
        assert len(rows) == m
        lens = np.array([len(c) for c, _ in rows], dtype=np.int64)
        r_idx = np.repeat(np.arange(m, dtype=np.int32), lens)
        c_idx = (np.concatenate([np.asarray(c, np.int32) for c, _ in rows])
                 if lens.sum() else np.zeros(0, np.int32))
        v = (np.concatenate([np.asarray(x, np.float64) for _, x in rows])
             if lens.sum() else np.zeros(0))
        for c, _ in rows:
            c = np.asarray(c)
            assert len(c) == 0 or (np.all(np.diff(c) > 0) and c[0] >= 0 and c[-1] < n)
        order = np.argsort(c_idx, kind="stable")  # rows ascend within a column
        # CSC of A (what the device probe is given).
        self.col_starts = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(c_idx, minlength=n), out=self.col_starts[1:])
        self.row_idx = r_idx[order]
        self.vals = v[order]
        # CSC of [A | I].
        self.starts = np.concatenate([self.col_starts, self.col_starts[-1] + 1 +
                                      np.arange(m, dtype=np.int64)])
        self.c_rows = np.concatenate([self.row_idx, np.arange(m, dtype=np.int32)])
        self.c_vals = np.concatenate([self.vals, np.ones(m)])
        # CSR of [A | I]: row r = its A entries, then the slack n + r.
        self.t_cols = [np.concatenate([np.asarray(c, np.int32), [n + r]]).astype(np.int32)
                       for r, (c, _) in enumerate(rows)]
        self.t_vals = [np.concatenate([np.asarray(x, np.float64), [1.0]]) for _, x in rows]
        self.row_len = lens + 1
        self.col_len = np.diff(self.starts)

    def entries(self, rows):
        return int(sum(self.row_len[r] for r in rows))


def column_scalar_products(mat, cols, v):
    """CompactSparseMatrix::ColumnScalarProduct (lp_data.h:547-567) per column:
    four accumulators over groups of four entries, r1 + r2 + r3 + r4, then up
    to three tail terms in order. Vectorised over the columns of equal length."""
    cols = np.asarray(cols, dtype=np.int64)
    v = np.asarray(v, dtype=np.float64)
    out = np.zeros(len(cols))
    lens = mat.col_len[cols]
    for L in np.unique(lens):
        sel = np.nonzero(lens == L)[0]
        idx = mat.starts[cols[sel]][:, None] + np.arange(L)[None, :]
        prod = mat.c_vals[idx] * v[mat.c_rows[idx]]
        r = [np.zeros(len(sel)) for _ in range(4)]
        full = (L // 4) * 4
        for g in range(0, full, 4):
            for k in range(4):
                r[k] = r[k] + prod[:, g + k]
        res = ((r[0] + r[1]) + r[2]) + r[3]
        for t in range(full, L):
            res = res + prod[:, t]
        out[sel] = res
    return out


class RefState:
    def __init__(self, mat):
        self.mat = mat
        self.coeff = np.zeros(mat.N)  # UploadMatrix zeroes the coefficients
        self.relevant = np.ones(mat.N, bool)
        self.list = np.zeros(0, np.int32)
        self.vals = np.zeros(0)
        self.rc = self.colbits = self.bound_diff = None

    def set_relevant(self, mask):
        self.relevant = np.asarray(mask, bool).copy()

    # --- update rows ------------------------------------------------------
    def row_wise(self, rows, rho, algorithm, drop):
        """Rows applied in filtered order. Per position the first write assigns
        (0.0 + v for algorithm 2), later writes add; algorithm 0 always
        assigns. Then row_wise_store's three rules."""
        mat = self.mat
        acc = np.zeros(mat.N)
        touched = np.zeros(mat.N, bool)
        for r in rows:
            cols = mat.t_cols[r]
            prod = rho[r] * mat.t_vals[r]
            if algorithm == 0:
                acc[cols] = prod
            else:
                first = ~touched[cols]
                acc[cols[first]] = (0.0 + prod[first]) if algorithm == 2 else prod[first]
                later = cols[~first]
                acc[later] = acc[later] + prod[~first]
            touched[cols] = True
        big = np.abs(acc) > drop
        if algorithm == 0:
            listed = touched & self.relevant & big
            self.coeff[listed] = acc[listed]
        elif algorithm == 1:
            listed = touched & self.relevant & big
            self.coeff[touched] = acc[touched]
        else:
            listed = self.relevant & big
            self.coeff = np.where(touched, acc, 0.0)
        self.list = np.nonzero(listed)[0].astype(np.int32)
        self.vals = acc[self.list].copy()
        self.last_acc, self.last_touched = acc, touched  # for the checks of the reference

    def column_wise(self, rho, drop):
        """coefficient[j] = a_j . rho for the relevant j with |dot| > drop; the
        other positions keep their stale value."""
        rel = np.nonzero(self.relevant)[0]
        dots = column_scalar_products(self.mat, rel, rho)
        keep = np.abs(dots) > drop
        self.list = rel[keep].astype(np.int32)
        self.vals = dots[keep].copy()
        self.coeff[self.list] = self.vals

    def list_dots(self, cols, v):
        return column_scalar_products(self.mat, cols, v)

    # --- pricing, row sums, norms -------------------------------------------
    def pricing(self, c, y):
        """rc[j] = c[j] - a_j . y for every column of [A | I]
        (reduced_costs.cc:372-381); kept for take_priced(), the dots as
        priced_dots."""
        dots = column_scalar_products(self.mat, np.arange(self.mat.N), y)
        self.priced_dots = dots
        self.priced = np.asarray(c, np.float64) - dots
        return self.priced.copy()

    def pricing_with_dots(self, c, y, w):
        """(rc, a_j . w over the last update row's list, in list order)."""
        return self.pricing(c, y), column_scalar_products(self.mat, self.list, w)

    def row_sums(self, x, skip, sign):
        """Per row: +0.0, then (sign * x_j) * a_rj added in increasing column
        order. An entry is left out when skip[j] is set or its multiplier
        sign * x_j == 0.0 (+-0.0; a NaN multiplier compares unequal and stays)
        (variable_values.cc:101-131, sparse.h:393)."""
        mat = self.mat
        x = np.asarray(x, np.float64)
        skip = np.zeros(mat.N, bool) if skip is None else np.asarray(skip, bool)
        out = np.zeros(mat.m)
        for r in range(mat.m):
            cols = mat.t_cols[r]
            mult = sign * x[cols]
            live = ~skip[cols] & (mult != 0.0)
            acc = np.float64(0.0)
            for p in (mult[live] * mat.t_vals[r][live]):
                acc = acc + p
            out[r] = acc
        return out

    def column_squared_norms(self):
        """1.0 + (v_0 v_0 + v_1 v_1 + ... in entry order, from +0.0) at the
        relevant columns (primal_edge_norms.cc:153-158 with an identity
        basis); NaN marks the other positions, which are undefined."""
        mat = self.mat
        out = np.full(mat.N, np.nan)
        rel = np.nonzero(self.relevant)[0]
        lens = mat.col_len[rel]
        for L in np.unique(lens):
            sel = rel[lens == L]
            v = mat.c_vals[mat.starts[sel][:, None] + np.arange(L)[None, :]]
            sq = v * v
            acc = np.zeros(len(sel))
            for t in range(L):
                acc = acc + sq[:, t]
            out[sel] = 1.0 + acc
        return out

    # --- dual device mode ---------------------------------------------------
    def dual_begin(self, rc, colbits, bound_diff):
        self.rc = np.asarray(rc, np.float64).copy()
        self.colbits = np.asarray(colbits, np.uint8).copy()
        self.bound_diff = np.asarray(bound_diff, np.float64).copy()

    def dual_set_col_bits(self, cols, b):
        self.colbits[np.asarray(cols)] = np.asarray(b, np.uint8)

    def breakpoints(self, sign, threshold, harris_tolerance, minimum_delta, variation):
        """dual_breakpoint per list slot (entering_variable.cc:68-96): dict of
        arrays over the slots: eligible, ratio, harris, sets_bound, mag, delta."""
        col = self.list
        c = self.vals
        coeff = c if sign > 0.0 else -c
        b = self.colbits[col]
        dec = ((b & COL_CAN_DECREASE) != 0) & (coeff > threshold)
        inc = ~dec & ((b & COL_CAN_INCREASE) != 0) & (coeff < -threshold)
        elig = dec | inc
        rcv = np.where(dec, -self.rc[col], self.rc[col])
        mag = np.where(dec, coeff, -coeff)
        mag = np.where(elig, mag, 1.0)  # unused slots: no division by zero
        ratio = rcv / mag
        harris = np.maximum(minimum_delta / mag, ratio + harris_tolerance / mag)
        boxed = (b & COL_BOXED) != 0
        delta = np.where(boxed, self.bound_diff[col] * mag, 0.0)
        sets_bound = ~boxed | (self.bound_diff[col] * mag >= variation)
        return dict(eligible=elig, ratio=ratio, harris=harris, sets_bound=sets_bound, mag=mag,
                    delta=delta, boxed=boxed)

    def dual_ratio(self, sign, threshold, harris_tolerance, minimum_delta, variation):
        """(B or None, kept slots in list order, P = the slots Glop's second
        loop pops out of the kept ones, entering slot or -1)."""
        assert minimum_delta > 0.0
        bp = self.breakpoints(sign, threshold, harris_tolerance, minimum_delta, variation)
        setters = bp["eligible"] & bp["sets_bound"]
        B = float(bp["harris"][setters].min()) if setters.any() else None
        if B is None:
            kept = np.nonzero(bp["eligible"])[0]
        else:
            kept = np.nonzero(bp["eligible"] & (bp["ratio"] <= B * (1.0 + 1e-9)))[0]
        # The heap's pop order (ColWithRatio::operator<): ratio ascending, then
        # the larger magnitude, then the smaller column.
        order = sorted(kept.tolist(), key=lambda s: (bp["ratio"][s], -bp["mag"][s], self.list[s]))
        harris_ratio = np.finfo(np.float64).max
        var = variation
        best_coeff, entering, popped = -1.0, -1, []
        for s in order:
            ratio, mag = bp["ratio"][s], bp["mag"][s]
            if ratio > harris_ratio:
                break
            if var > 0.0 and bp["boxed"][s]:
                var -= self.bound_diff[self.list[s]] * mag
                if var > 0.0:
                    popped.append(s)
                    continue
            if mag >= best_coeff:
                harris_ratio = min(harris_ratio, max(minimum_delta / mag,
                                                     ratio + harris_tolerance / mag))
                if not (mag == best_coeff and entering >= 0 and ratio == bp["ratio"][entering]):
                    best_coeff, entering = mag, s
            popped.append(s)
        return B, kept, np.array(sorted(popped), dtype=np.int64), entering

    def boxed_flips(self, cols, threshold):
        """boxed_flips_kernel (revised_simplex.cc:2391-2437): with status =
        (bits >> 3) & 7, a column flips when it sits at its upper bound
        (status 3) with rc > threshold, or at its lower bound (status 2) with
        rc < -threshold. cols None: all N columns, and only those with
        COL_BOXED set can flip; with a list the bit is not consulted. uint8
        flags, one per column (or list slot)."""
        if cols is None:
            col = np.arange(self.mat.N)
            allowed = (self.colbits & COL_BOXED) != 0
        else:
            col = np.asarray(cols, np.int64)
            allowed = np.ones(len(col), bool)
        rc = self.rc[col]
        status = (self.colbits[col] >> STATUS_SHIFT) & 7
        flip = ((rc > threshold) & (status == STATUS_AT_UPPER)) | \
               ((rc < -threshold) & (status == STATUS_AT_LOWER))
        return (allowed & flip).astype(np.uint8)

    def take_priced(self):
        """The last pricing() result becomes the reduced costs."""
        self.rc = self.priced.copy()

    def set_reduced_cost(self, col, value):
        self.rc[col] = value

    def update_reduced_costs(self, mult, leaving_col, leaving_value, entering_col):
        """rc[list[i]] += mult * coeff[i] except the entering column; then
        rc[leaving] = its value and rc[entering] = 0."""
        sel = self.list != entering_col
        cols = self.list[sel]
        self.rc[cols] = self.rc[cols] + mult * self.vals[sel]
        if leaving_col >= 0:
            self.rc[leaving_col] = leaving_value
        if entering_col >= 0:
            self.rc[entering_col] = 0.0
