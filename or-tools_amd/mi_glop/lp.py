"""In-memory LP in the shape Glop's RevisedSimplex::Solve consumes.

Mirrors the subset of glop::LinearProgram (ortools/lp_data/lp_data.h:56) the
revised simplex reads: A in CSC with rows sorted per column and no explicit
zeros (LinearProgram::IsCleanedUp, lp_solver.cc:185-191), variable and
constraint bounds, objective, offset, scaling factor and sense.
"""
from dataclasses import dataclass, field

import numpy as np

INF = np.inf


@dataclass
class LinearProgram:
    m: int
    n: int
    col_starts: np.ndarray  # int64[n+1]
    row_idx: np.ndarray  # int32[nnz]
    vals: np.ndarray  # float64[nnz]
    col_lb: np.ndarray
    col_ub: np.ndarray
    row_lb: np.ndarray
    row_ub: np.ndarray
    obj: np.ndarray
    obj_offset: float = 0.0
    obj_scale: float = 1.0
    maximize: bool = False
    name: str = field(default="lp")

    @property
    def nnz(self):
        return int(self.col_starts[-1])

    def validate(self):
        """LinearProgram::IsValid / IsCleanedUp checks (lp_solver.cc:185-202)."""
        cs = self.col_starts
        if cs.shape != (self.n + 1,) or cs[0] != 0 or np.any(np.diff(cs) < 0):
            return False
        for c in range(self.n):
            r = self.row_idx[cs[c]:cs[c + 1]]
            if np.any(np.diff(r) <= 0):
                return False
        if np.any(self.row_idx < 0) or np.any(self.row_idx >= self.m):
            return False
        if np.any(self.vals == 0) or not np.all(np.isfinite(self.vals)):
            return False
        for lo, hi in ((self.col_lb, self.col_ub), (self.row_lb, self.row_ub)):
            if np.any(lo > hi) or np.any(lo == INF) or np.any(hi == -INF):
                return False
        return bool(np.all(np.isfinite(self.obj)))

    def with_rows(self, row_starts, cols, vals, row_lb, row_ub):
        """The LP extended by k rows given as lists (LpHandle.add_rows'
        arguments): row j, columns cols[row_starts[j]:row_starts[j+1]]
        ascending, becomes row m + j; every column keeps its entries and takes
        the new ones at its end. Bounds, objective and sense are shared."""
        row_starts = np.asarray(row_starts, np.int64)
        cols = np.asarray(cols, np.int64)
        vals = np.asarray(vals, np.float64)
        k = len(row_starts) - 1
        new_rows = self.m + np.repeat(np.arange(k, dtype=np.int64), np.diff(row_starts))
        old_cols = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.col_starts))
        all_cols = np.concatenate([old_cols, cols])
        all_rows = np.concatenate([self.row_idx.astype(np.int64), new_rows])
        # Old entries are column-major already and every new row lies below
        # them, so a stable sort by column alone leaves the rows ascending.
        order = np.argsort(all_cols, kind="stable")
        starts = np.zeros(self.n + 1, np.int64)
        np.cumsum(np.bincount(all_cols, minlength=self.n), out=starts[1:])
        return LinearProgram(
            self.m + k, self.n, starts, all_rows[order].astype(np.int32),
            np.concatenate([self.vals, vals])[order], self.col_lb, self.col_ub,
            np.concatenate([self.row_lb, np.asarray(row_lb, np.float64)]),
            np.concatenate([self.row_ub, np.asarray(row_ub, np.float64)]), self.obj,
            self.obj_offset, self.obj_scale, self.maximize, self.name)

    def without_rows(self, mask):
        """The LP without the rows that the boolean mask (length m) names:
        kept rows keep their order and are renumbered, every column keeps its
        other entries in order. Column bounds, objective and sense are
        shared."""
        mask = np.asarray(mask, bool)
        if mask.shape != (self.m,):
            raise ValueError("a row mask has one entry per row")
        new_row = np.cumsum(~mask) - 1
        keep = ~mask[self.row_idx]
        cols = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.col_starts))
        starts = np.zeros(self.n + 1, np.int64)
        np.cumsum(np.bincount(cols[keep], minlength=self.n), out=starts[1:])
        return LinearProgram(
            int((~mask).sum()), self.n, starts, new_row[self.row_idx[keep]].astype(np.int32),
            self.vals[keep], self.col_lb, self.col_ub, self.row_lb[~mask], self.row_ub[~mask],
            self.obj, self.obj_offset, self.obj_scale, self.maximize, self.name)

    @staticmethod
    def from_dense(A, col_lb, col_ub, row_lb, row_ub, obj, offset=0.0,
                   maximize=False, name="lp"):
        A = np.asarray(A, dtype=np.float64)
        m, n = A.shape
        starts = [0]
        rows, vals = [], []
        for c in range(n):
            nz = np.nonzero(A[:, c])[0]
            rows.extend(nz.tolist())
            vals.extend(A[nz, c].tolist())
            starts.append(len(rows))
        return LinearProgram(
            m, n, np.asarray(starts, np.int64), np.asarray(rows, np.int32),
            np.asarray(vals, np.float64), np.asarray(col_lb, np.float64),
            np.asarray(col_ub, np.float64), np.asarray(row_lb, np.float64),
            np.asarray(row_ub, np.float64), np.asarray(obj, np.float64),
            float(offset), 1.0, bool(maximize), name)

    @staticmethod
    def from_triplets(m, n, triplets, col_lb, col_ub, row_lb, row_ub, obj,
                      offset=0.0, maximize=False, name="lp"):
        A = np.zeros((m, n))
        for r, c, v in triplets:
            A[r, c] = v
        return LinearProgram.from_dense(A, col_lb, col_ub, row_lb, row_ub, obj,
                                        offset, maximize, name)
