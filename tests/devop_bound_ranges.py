"""The probe entries appended after last_row_violations
(include/mi_lp_devop.h): bound_ranges_panel, bound_ranges_panel_from,
bound_infeasible_panel, bound_infeasible_panel_from, last_bound_ranges.

TEST INFRASTRUCTURE ONLY. BoundRangesDevOp is
devop_row_violations.RowViolationsDevOp (every older entry goes through the
older bindings of the table's prefix) plus these calls, bound here through
the longer struct. A library without the entries is an error, never a skip:
api() refuses a library that lacks mi_lp_bound_activity_ranges (the table of
such a library ends before these entries).
"""
import ctypes

import numpy as np

import devop_row_violations as drv
from mi_glop import engine

CAPACITY = drv.CAPACITY
CapacityError = drv.CapacityError
SUMMARY = drv.SUMMARY

_vp = ctypes.c_void_p
_i = ctypes.c_int
_d = ctypes.c_double
_i64 = ctypes.c_int64


class BoundRangesApi(ctypes.Structure):
    _fields_ = drv.RowViolationsApi._fields_ + [
        ("bound_ranges_panel", ctypes.CFUNCTYPE(_i, _vp, _vp, _vp, _i, _vp, _vp, _vp)),
        ("bound_ranges_panel_from", ctypes.CFUNCTYPE(_i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp,
                                                     _vp, _vp, _vp)),
        ("bound_infeasible_panel", ctypes.CFUNCTYPE(_i, _vp, _vp, _vp, _i, _vp, _vp, _d, _vp, _vp,
                                                    _vp, _i64, _vp)),
        ("bound_infeasible_panel_from", ctypes.CFUNCTYPE(_i, _vp, _vp, _vp, _i, _vp, _vp, _vp,
                                                         _vp, _vp, _vp, _d, _vp, _vp, _vp, _i64,
                                                         _vp)),
        ("last_bound_ranges", ctypes.CFUNCTYPE(_i, _vp, ctypes.POINTER(drv.RowViolations))),
    ]


_api = None


def api():
    global _api
    if _api is None:
        lib = engine.lib()
        assert hasattr(lib, "mi_lp_bound_activity_ranges"), \
            "the library has no bound-set activity ranges (mi_devop_table ends before them)"
        _api = BoundRangesApi.in_dll(lib, "mi_devop_table")
    return _api


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class BoundRangesDevOp(drv.RowViolationsDevOp):
    def _sets(self, L, U):
        L, U = _f64(L), _f64(U)
        assert L.ndim == 2 and L.shape == U.shape and L.shape[1] == self.n
        return L, U, L.shape[0]

    def _overrides(self, base_lb, base_ub, starts, cols, new_lbs, new_ubs):
        base_lb, base_ub = _f64(base_lb), _f64(base_ub)
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        new_lbs, new_ubs = _f64(new_lbs), _f64(new_ubs)
        assert len(base_lb) == len(base_ub) == self.n
        assert len(cols) == len(new_lbs) == len(new_ubs) == starts[-1]
        k = len(starts) - 1
        some = len(cols) > 0
        keep = (base_lb, base_ub, starts, cols, new_lbs, new_ubs)
        lead = (_p(base_lb), _p(base_ub), k, _p(starts), _p(cols) if some else None,
                _p(new_lbs) if some else None, _p(new_ubs) if some else None)
        return lead, k, keep

    def _ranges(self, call, lead, k, counts, buffers):
        """buffers: optional dict of lo, hi (flat float64) and counts (flat
        int32) that receive the result in place."""
        buffers = dict(buffers or {})
        lo = buffers.get("lo")
        hi = buffers.get("hi")
        inf = buffers.get("counts")
        if lo is None:
            lo = np.zeros(max(1, k * self.m))
        if hi is None:
            hi = np.zeros(max(1, k * self.m))
        if inf is None and counts:
            inf = np.zeros(max(1, k * self.m * 2), np.int32)
        assert lo.dtype == hi.dtype == np.float64 and min(len(lo), len(hi)) >= k * self.m
        assert inf is None or (inf.dtype == np.int32 and len(inf) >= 2 * k * self.m)
        self._check(call(self.h, *lead, _p(lo), _p(hi), _p(inf) if counts else None))
        shape = (k, self.m)
        if not counts:
            return lo[:k * self.m].reshape(shape), hi[:k * self.m].reshape(shape), None, None
        pairs = inf[:2 * k * self.m].reshape(k, self.m, 2)
        return (lo[:k * self.m].reshape(shape), hi[:k * self.m].reshape(shape),
                pairs[:, :, 0].copy(), pairs[:, :, 1].copy())

    def bound_ranges_panel(self, L, U, counts=True, buffers=None):
        """L, U: (k, n). Returns (lo, hi, lo_inf, hi_inf), each (k, m); with
        counts=False (inf_counts NULL) the last two are None."""
        L, U, k = self._sets(L, U)
        return self._ranges(api().bound_ranges_panel, (_p(L), _p(U), k), k, counts, buffers)

    def bound_ranges_panel_from(self, base_lb, base_ub, starts, cols, new_lbs, new_ubs,
                                counts=True, buffers=None):
        """base_lb, base_ub: n; the rest as bound_range_cases.flatten."""
        lead, k, _keep = self._overrides(base_lb, base_ub, starts, cols, new_lbs, new_ubs)
        return self._ranges(api().bound_ranges_panel_from, lead, k, counts, buffers)

    def bound_infeasible_panel(self, L, U, lb, ub, tolerance, lists=True, capacity=None,
                               buffers=None):
        """Returns (row_starts, rows, amounts, summaries) cut to the result;
        with lists=False (row_starts NULL) the first three are None."""
        L, U, k = self._sets(L, U)
        return self._violations(api().bound_infeasible_panel, (_p(L), _p(U), k), k, lb, ub,
                                tolerance, lists, capacity, buffers)

    def bound_infeasible_panel_from(self, base_lb, base_ub, starts, cols, new_lbs, new_ubs, lb, ub,
                                    tolerance, lists=True, capacity=None, buffers=None):
        lead, k, _keep = self._overrides(base_lb, base_ub, starts, cols, new_lbs, new_ubs)
        return self._violations(api().bound_infeasible_panel_from, lead, k, lb, ub, tolerance,
                                lists, capacity, buffers)

    def last_bound_ranges(self):
        p = drv.RowViolations()
        self._check(api().last_bound_ranges(self.h, ctypes.byref(p)))
        return {"panels": p.panels, "width": p.width, "lists": bool(p.lists), "kept": p.kept,
                "bytes_down": p.bytes_down, "overrides_up_bytes": p.overrides_up_bytes}
