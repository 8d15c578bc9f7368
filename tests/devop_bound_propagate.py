"""The probe entries appended after last_bound_implied
(include/mi_lp_devop.h): bound_propagate_panel, bound_propagate_panel_from,
bound_propagated_columns_from, last_bound_propagate.

TEST INFRASTRUCTURE ONLY. BoundPropagateDevOp is
devop_bound_implied.BoundImpliedDevOp (every older entry goes through the
older bindings of the table's prefix) plus these calls, bound here through the
longer struct. A library without the entries is an error, never a skip: api()
refuses a library that lacks mi_lp_bound_propagate (the table of such a library
ends before these entries).
"""
import ctypes

import numpy as np

import devop_bound_implied as dbi
from mi_glop import engine

CAPACITY = dbi.CAPACITY
CapacityError = dbi.CapacityError
SHORT_COLUMNS, LONG_COLUMNS = dbi.SHORT_COLUMNS, dbi.LONG_COLUMNS
SUMMARY = np.dtype([("status", np.int32), ("rounds", np.int32), ("moves", np.int64),
                    ("worst", np.float64), ("worst_col", np.int32), ("kept", np.int32)])
assert SUMMARY.itemsize == 32

_vp = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64


class PropagateParams(ctypes.Structure):
    _fields_ = [("is_integer", _vp), ("tolerance", ctypes.c_double),
                ("integrality_tolerance", ctypes.c_double), ("max_rounds", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class BoundPropagate(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in ("panels", "width", "columns", "lists")] +
                [(n, ctypes.c_int64) for n in ("rounds", "kept", "bytes_up", "bytes_down")])


_pp = ctypes.POINTER(PropagateParams)


class BoundPropagateApi(ctypes.Structure):
    _fields_ = dbi.BoundImpliedApi._fields_ + [
        ("bound_propagate_panel", ctypes.CFUNCTYPE(_i, _vp, _vp, _vp, _i, _pp, _vp, _vp, _vp, _vp,
                                                   _vp)),
        ("bound_propagate_panel_from", ctypes.CFUNCTYPE(_i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp,
                                                        _pp, _vp, _vp, _vp, _vp, _vp)),
        ("bound_propagated_columns_from", ctypes.CFUNCTYPE(_i, _vp, _vp, _vp, _i, _vp, _vp, _vp,
                                                           _vp, _pp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                           _i64, _vp)),
        ("last_bound_propagate", ctypes.CFUNCTYPE(_i, _vp, ctypes.POINTER(BoundPropagate))),
    ]


_api = None


def api():
    global _api
    if _api is None:
        lib = engine.lib()
        assert hasattr(lib, "mi_lp_bound_propagate"), \
            "the library has no bound propagation (mi_devop_table ends before it)"
        _api = BoundPropagateApi.in_dll(lib, "mi_devop_table")
    return _api


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class BoundPropagateDevOp(dbi.BoundImpliedDevOp):
    def _params(self, is_integer, tolerance, integrality_tolerance, max_rounds):
        """(params, keep): keep holds the array behind the pointer."""
        if is_integer is not None:
            is_integer = np.ascontiguousarray(is_integer, dtype=np.uint8)
            assert is_integer.shape == (self.n,)
        p = PropagateParams(None if is_integer is None else is_integer.ctypes.data, tolerance,
                            integrality_tolerance, max_rounds, 0)
        return p, is_integer

    def _dense_propagate(self, call, lead, k, params, lb, ub, buffers):
        """buffers: optional dict of new_lbs, new_ubs (flat float64) and
        summaries (SUMMARY) that receive the result in place."""
        lb, ub = self._row_bounds(lb, ub)
        buffers = dict(buffers or {})
        lo, hi, s = buffers.get("new_lbs"), buffers.get("new_ubs"), buffers.get("summaries")
        if lo is None:
            lo = np.zeros(max(1, k * self.n))
        if hi is None:
            hi = np.zeros(max(1, k * self.n))
        if s is None:
            s = np.zeros(max(1, k), SUMMARY)
        assert lo.dtype == hi.dtype == np.float64 and min(len(lo), len(hi)) >= k * self.n
        assert s.dtype == SUMMARY and len(s) >= k
        p, _keep = self._params(*params)
        self._check(call(self.h, *lead, ctypes.byref(p), _p(lb), _p(ub), _p(lo), _p(hi), _p(s)))
        return lo[:k * self.n].reshape(k, self.n), hi[:k * self.n].reshape(k, self.n), s[:k]

    def bound_propagate_panel(self, L, U, lb, ub, is_integer, tolerance, integrality_tolerance,
                              max_rounds, buffers=None):
        """L, U: (k, n). Returns (new_lbs, new_ubs, summaries)."""
        L, U, k = self._sets(L, U)
        return self._dense_propagate(api().bound_propagate_panel, (_p(L), _p(U), k), k,
                                     (is_integer, tolerance, integrality_tolerance, max_rounds),
                                     lb, ub, buffers)

    def bound_propagate_panel_from(self, base_lb, base_ub, starts, cols, ov_lbs, ov_ubs, lb, ub,
                                   is_integer, tolerance, integrality_tolerance, max_rounds,
                                   buffers=None):
        lead, k, _keep = self._overrides(base_lb, base_ub, starts, cols, ov_lbs, ov_ubs)
        return self._dense_propagate(api().bound_propagate_panel_from, lead, k,
                                     (is_integer, tolerance, integrality_tolerance, max_rounds),
                                     lb, ub, buffers)

    def bound_propagated_columns_from(self, base_lb, base_ub, starts, cols, ov_lbs, ov_ubs, lb,
                                      ub, is_integer, tolerance, integrality_tolerance,
                                      max_rounds, lists=True, capacity=None, buffers=None):
        """Returns (col_starts, cols, new_lbs, new_ubs, summaries) cut to the
        result; with lists=False (col_starts NULL) the first four are None.
        buffers: optional dict of col_starts, cols, new_lbs, new_ubs,
        summaries that receive the result in place (capacity defaults to
        len(cols), or to k * n)."""
        lead, k, _keep = self._overrides(base_lb, base_ub, starts, cols, ov_lbs, ov_ubs)
        lb, ub = self._row_bounds(lb, ub)
        buffers = dict(buffers or {})
        summaries = buffers.get("summaries")
        if summaries is None:
            summaries = np.zeros(max(k, 1), SUMMARY)
        assert summaries.dtype == SUMMARY and len(summaries) >= k
        col_starts = out_cols = lo = hi = None
        if lists:
            out_cols, lo, hi = buffers.get("cols"), buffers.get("new_lbs"), buffers.get("new_ubs")
            if capacity is None:
                capacity = k * self.n if out_cols is None else len(out_cols)
            col_starts = buffers.get("col_starts")
            if col_starts is None:
                col_starts = np.zeros(k + 1, np.int64)
            if out_cols is None:
                out_cols = np.zeros(max(1, capacity), np.int32)
            if lo is None:
                lo = np.zeros(max(1, capacity), np.float64)
            if hi is None:
                hi = np.zeros(max(1, capacity), np.float64)
            assert col_starts.dtype == np.int64 and len(col_starts) >= k + 1
            assert out_cols.dtype == np.int32 and lo.dtype == hi.dtype == np.float64
            assert min(len(out_cols), len(lo), len(hi)) >= capacity
        p, _keep_int = self._params(is_integer, tolerance, integrality_tolerance, max_rounds)
        rc = api().bound_propagated_columns_from(
            self.h, *lead, ctypes.byref(p), _p(lb), _p(ub), _p(col_starts), _p(out_cols), _p(lo),
            _p(hi), capacity or 0, _p(summaries))
        if rc == CAPACITY:
            raise CapacityError(self._a.last_error(self.h).decode())
        self._check(rc)
        if not lists:
            return None, None, None, None, summaries[:k]
        kept = int(col_starts[k])
        return col_starts[:k + 1], out_cols[:kept], lo[:kept], hi[:kept], summaries[:k]

    def last_bound_propagate(self):
        p = BoundPropagate()
        self._check(api().last_bound_propagate(self.h, ctypes.byref(p)))
        return {"panels": p.panels, "width": p.width, "columns": p.columns,
                "lists": bool(p.lists), "rounds": p.rounds, "kept": p.kept,
                "bytes_up": p.bytes_up, "bytes_down": p.bytes_down}
