"""The probe entries appended after row_panel_geometry
(include/mi_lp_devop.h): row_violations_panel, row_violations_panel_from,
last_row_violations.

TEST INFRASTRUCTURE ONLY. RowViolationsDevOp is devop_row_panel.RowPanelDevOp
(every older entry goes through the older bindings of the table's prefix)
plus these calls, bound here through the longer struct.
"""
import ctypes

import numpy as np

import devop_panel_sparse
import devop_row_panel
from mi_glop import engine

CAPACITY = devop_panel_sparse.CAPACITY  # MI_DEVOP_CAPACITY
CapacityError = devop_panel_sparse.CapacityError
SUMMARY = engine.POINT_VIOLATIONS  # mi_devop_point_violations

_vp = ctypes.c_void_p
_i = ctypes.c_int
_d = ctypes.c_double
_i64 = ctypes.c_int64


class RowViolations(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in ("panels", "width", "lists", "reserved")] +
                [(n, ctypes.c_int64) for n in ("kept", "bytes_down", "overrides_up_bytes")])


class RowViolationsApi(ctypes.Structure):
    _fields_ = devop_row_panel.RowPanelApi._fields_ + [
        ("row_violations_panel", ctypes.CFUNCTYPE(_i, _vp, _vp, _i, _vp, _vp, _d, _vp, _vp, _vp,
                                                  _i64, _vp)),
        ("row_violations_panel_from", ctypes.CFUNCTYPE(_i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp,
                                                       _d, _vp, _vp, _vp, _i64, _vp)),
        ("last_row_violations", ctypes.CFUNCTYPE(_i, _vp, ctypes.POINTER(RowViolations))),
    ]


_api = None


def api():
    global _api
    if _api is None:
        _api = RowViolationsApi.in_dll(engine.lib(), "mi_devop_table")
    return _api


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


class RowViolationsDevOp(devop_row_panel.RowPanelDevOp):
    def _violations(self, call, lead, k, lb, ub, tolerance, lists, capacity, buffers):
        """The shared tail of the two calls. buffers: optional dict of
        row_starts, rows, activities, summaries that receive the result in
        place (capacity defaults to len(rows), or to k * m)."""
        lb = np.ascontiguousarray(lb, dtype=np.float64)
        ub = np.ascontiguousarray(ub, dtype=np.float64)
        assert len(lb) == len(ub) == self.m
        buffers = dict(buffers or {})
        summaries = buffers.get("summaries")
        if summaries is None:
            summaries = np.zeros(max(k, 1), SUMMARY)
        assert summaries.dtype == SUMMARY and len(summaries) >= k
        row_starts = rows = activities = None
        if lists:
            rows, activities = buffers.get("rows"), buffers.get("activities")
            if capacity is None:
                capacity = k * self.m if rows is None else len(rows)
            row_starts = buffers.get("row_starts")
            if row_starts is None:
                row_starts = np.zeros(k + 1, np.int64)
            if rows is None:
                rows = np.zeros(max(1, capacity), np.int32)
            if activities is None:
                activities = np.zeros(max(1, capacity), np.float64)
            assert row_starts.dtype == np.int64 and len(row_starts) >= k + 1
            assert rows.dtype == np.int32 and activities.dtype == np.float64
            assert len(rows) >= capacity and len(activities) >= capacity
        rc = call(self.h, *lead, _p(lb), _p(ub), tolerance, _p(row_starts), _p(rows),
                  _p(activities), capacity or 0, _p(summaries))
        if rc == CAPACITY:
            raise CapacityError(self._a.last_error(self.h).decode())
        self._check(rc)
        if not lists:
            return None, None, None, summaries[:k]
        kept = int(row_starts[k])
        return row_starts[:k + 1], rows[:kept], activities[:kept], summaries[:k]

    def row_violations_panel(self, X, lb, ub, tolerance, lists=True, capacity=None, buffers=None):
        """X: (k, N). Returns (row_starts, rows, activities, summaries) cut to
        the result; with lists=False (row_starts NULL) the first three are
        None."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        assert X.ndim == 2 and X.shape[1] == self.N
        k = X.shape[0]
        return self._violations(api().row_violations_panel, (_p(X), k), k, lb, ub, tolerance,
                                lists, capacity, buffers)

    def row_violations_panel_from(self, base, starts, cols, vals, lb, ub, tolerance, lists=True,
                                  capacity=None, buffers=None):
        """base: N; starts (k + 1), cols, vals as row_panel_cases.flatten."""
        base = np.ascontiguousarray(base, dtype=np.float64)
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        assert len(base) == self.N and len(cols) == len(vals) == starts[-1]
        k = len(starts) - 1
        lead = (_p(base), k, _p(starts), _p(cols) if len(cols) else None,
                _p(vals) if len(vals) else None)
        return self._violations(api().row_violations_panel_from, lead, k, lb, ub, tolerance,
                                lists, capacity, buffers)

    def last_row_violations(self):
        p = RowViolations()
        self._check(api().last_row_violations(self.h, ctypes.byref(p)))
        return {"panels": p.panels, "width": p.width, "lists": bool(p.lists), "kept": p.kept,
                "bytes_down": p.bytes_down, "overrides_up_bytes": p.overrides_up_bytes}
