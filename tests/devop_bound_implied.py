"""The probe entries appended after last_bound_ranges
(include/mi_lp_devop.h): bound_implied_panel, bound_implied_panel_from,
bound_tightened_panel, bound_tightened_panel_from, last_bound_implied.

TEST INFRASTRUCTURE ONLY. BoundImpliedDevOp is
devop_bound_ranges.BoundRangesDevOp (every older entry goes through the older
bindings of the table's prefix) plus these calls, bound here through the
longer struct. A library without the entries is an error, never a skip: api()
refuses a library that lacks mi_lp_bound_implied_bounds (the table of such a
library ends before these entries).
"""
import ctypes

import numpy as np

import devop_bound_ranges as dbr
from mi_glop import engine

CAPACITY = dbr.CAPACITY
CapacityError = dbr.CapacityError
SUMMARY = dbr.SUMMARY
SHORT_COLUMNS, LONG_COLUMNS = 1, 2  # MI_DEVOP_PANEL_SHORT_COLUMNS, MI_DEVOP_PANEL_LONG_COLUMNS

_vp = ctypes.c_void_p
_i = ctypes.c_int
_d = ctypes.c_double
_i64 = ctypes.c_int64


class BoundImplied(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in ("panels", "width", "columns", "lists")] +
                [(n, ctypes.c_int64) for n in ("kept", "bytes_up", "bytes_down")])


class BoundImpliedApi(ctypes.Structure):
    _fields_ = dbr.BoundRangesApi._fields_ + [
        ("bound_implied_panel", ctypes.CFUNCTYPE(_i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp)),
        ("bound_implied_panel_from", ctypes.CFUNCTYPE(_i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp,
                                                      _vp, _vp, _vp, _vp)),
        ("bound_tightened_panel", ctypes.CFUNCTYPE(_i, _vp, _vp, _vp, _i, _vp, _vp, _d, _vp, _vp,
                                                   _vp, _vp, _i64, _vp)),
        ("bound_tightened_panel_from", ctypes.CFUNCTYPE(_i, _vp, _vp, _vp, _i, _vp, _vp, _vp,
                                                        _vp, _vp, _vp, _d, _vp, _vp, _vp, _vp,
                                                        _i64, _vp)),
        ("last_bound_implied", ctypes.CFUNCTYPE(_i, _vp, ctypes.POINTER(BoundImplied))),
    ]


_api = None


def api():
    global _api
    if _api is None:
        lib = engine.lib()
        assert hasattr(lib, "mi_lp_bound_implied_bounds"), \
            "the library has no implied column bounds (mi_devop_table ends before them)"
        _api = BoundImpliedApi.in_dll(lib, "mi_devop_table")
    return _api


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class BoundImpliedDevOp(dbr.BoundRangesDevOp):
    def _row_bounds(self, lb, ub):
        lb, ub = _f64(lb), _f64(ub)
        assert len(lb) == len(ub) == self.m
        return lb, ub

    def _dense(self, call, lead, k, lb, ub, buffers):
        """buffers: optional dict of new_lbs, new_ubs (flat float64) that
        receive the result in place."""
        lb, ub = self._row_bounds(lb, ub)
        buffers = dict(buffers or {})
        lo, hi = buffers.get("new_lbs"), buffers.get("new_ubs")
        if lo is None:
            lo = np.zeros(max(1, k * self.n))
        if hi is None:
            hi = np.zeros(max(1, k * self.n))
        assert lo.dtype == hi.dtype == np.float64 and min(len(lo), len(hi)) >= k * self.n
        self._check(call(self.h, *lead, _p(lb), _p(ub), _p(lo), _p(hi)))
        return lo[:k * self.n].reshape(k, self.n), hi[:k * self.n].reshape(k, self.n)

    def bound_implied_panel(self, L, U, lb, ub, buffers=None):
        """L, U: (k, n). Returns (new_lbs, new_ubs), each (k, n)."""
        L, U, k = self._sets(L, U)
        return self._dense(api().bound_implied_panel, (_p(L), _p(U), k), k, lb, ub, buffers)

    def bound_implied_panel_from(self, base_lb, base_ub, starts, cols, ov_lbs, ov_ubs, lb, ub,
                                 buffers=None):
        lead, k, _keep = self._overrides(base_lb, base_ub, starts, cols, ov_lbs, ov_ubs)
        return self._dense(api().bound_implied_panel_from, lead, k, lb, ub, buffers)

    def _tightened(self, call, lead, k, lb, ub, tolerance, lists, capacity, buffers):
        """buffers: optional dict of col_starts, cols, new_lbs, new_ubs,
        summaries that receive the result in place (capacity defaults to
        len(cols), or to k * n)."""
        lb, ub = self._row_bounds(lb, ub)
        buffers = dict(buffers or {})
        summaries = buffers.get("summaries")
        if summaries is None:
            summaries = np.zeros(max(k, 1), SUMMARY)
        assert summaries.dtype == SUMMARY and len(summaries) >= k
        col_starts = cols = lo = hi = None
        if lists:
            cols, lo, hi = buffers.get("cols"), buffers.get("new_lbs"), buffers.get("new_ubs")
            if capacity is None:
                capacity = k * self.n if cols is None else len(cols)
            col_starts = buffers.get("col_starts")
            if col_starts is None:
                col_starts = np.zeros(k + 1, np.int64)
            if cols is None:
                cols = np.zeros(max(1, capacity), np.int32)
            if lo is None:
                lo = np.zeros(max(1, capacity), np.float64)
            if hi is None:
                hi = np.zeros(max(1, capacity), np.float64)
            assert col_starts.dtype == np.int64 and len(col_starts) >= k + 1
            assert cols.dtype == np.int32 and lo.dtype == hi.dtype == np.float64
            assert min(len(cols), len(lo), len(hi)) >= capacity
        rc = call(self.h, *lead, _p(lb), _p(ub), tolerance, _p(col_starts), _p(cols), _p(lo),
                  _p(hi), capacity or 0, _p(summaries))
        if rc == CAPACITY:
            raise CapacityError(self._a.last_error(self.h).decode())
        self._check(rc)
        if not lists:
            return None, None, None, None, summaries[:k]
        kept = int(col_starts[k])
        return col_starts[:k + 1], cols[:kept], lo[:kept], hi[:kept], summaries[:k]

    def bound_tightened_panel(self, L, U, lb, ub, tolerance, lists=True, capacity=None,
                              buffers=None):
        """Returns (col_starts, cols, new_lbs, new_ubs, summaries) cut to the
        result; with lists=False (col_starts NULL) the first four are None."""
        L, U, k = self._sets(L, U)
        return self._tightened(api().bound_tightened_panel, (_p(L), _p(U), k), k, lb, ub,
                               tolerance, lists, capacity, buffers)

    def bound_tightened_panel_from(self, base_lb, base_ub, starts, cols, ov_lbs, ov_ubs, lb, ub,
                                   tolerance, lists=True, capacity=None, buffers=None):
        lead, k, _keep = self._overrides(base_lb, base_ub, starts, cols, ov_lbs, ov_ubs)
        return self._tightened(api().bound_tightened_panel_from, lead, k, lb, ub, tolerance,
                               lists, capacity, buffers)

    def last_bound_implied(self):
        p = BoundImplied()
        self._check(api().last_bound_implied(self.h, ctypes.byref(p)))
        return {"panels": p.panels, "width": p.width, "columns": p.columns,
                "lists": bool(p.lists), "kept": p.kept, "bytes_up": p.bytes_up,
                "bytes_down": p.bytes_down}
