"""The probe entries appended after last_penalties (include/mi_lp_devop.h):
column_cuts_panel, last_cuts.

TEST INFRASTRUCTURE ONLY. CutsDevOp is devop_penalties.PenaltiesDevOp (every
older entry goes through the older bindings of the table's prefix) plus these
calls, bound here through the longer struct. A library without the entries is
an error, never a skip: api() refuses a library that lacks
mi_lp_row_gomory_cuts (the table of such a library ends before these entries).
"""
import ctypes

import numpy as np

import devop_panel
import devop_panel_sparse
import devop_penalties as dpn
from mi_glop import engine

SUMMARY = engine.CUT_SUMMARY

_vp = ctypes.c_void_p
_i = ctypes.c_int


class Cuts(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in ("sparse", "dense", "panels", "width", "tiles",
                                               "structural_tiles", "lists", "reserved")] +
                [("kept", ctypes.c_int64), ("bytes_down", ctypes.c_int64)])


class CutsApi(ctypes.Structure):
    _fields_ = dpn.PenaltiesApi._fields_ + [
        ("column_cuts_panel", ctypes.CFUNCTYPE(_i, _vp, _vp, _i, _vp, _vp, _vp, _vp,
                                               ctypes.c_double, ctypes.c_double, _vp, _vp, _vp,
                                               ctypes.c_int64, _vp)),
        ("last_cuts", ctypes.CFUNCTYPE(_i, _vp, ctypes.POINTER(Cuts))),
    ]


_api = None


def api():
    global _api
    if _api is None:
        lib = engine.lib()
        assert hasattr(lib, "mi_lp_row_gomory_cuts"), \
            "the library has no Gomory cuts (mi_devop_table ends before them)"
        _api = CutsApi.in_dll(lib, "mi_devop_table")
    return _api


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


class CutsDevOp(dpn.PenaltiesDevOp):
    def column_cuts_panel(self, Y, status, unit, f0, row_unit, zero_tolerance, drop_tolerance,
                          lists=True, summaries=None, capacity=None):
        """Y: (k, m); status (int8): N; unit: N or None; f0, row_unit: k.
        Returns (row_starts, cols, vals, summaries) (engine.CUT_SUMMARY), the
        first three None with lists=False; `summaries` (at least k records)
        receives them in place when given."""
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        assert Y.ndim == 2 and Y.shape[1] == self.m
        k = Y.shape[0]
        status = np.ascontiguousarray(status, dtype=np.int8)
        unit = None if unit is None else np.ascontiguousarray(unit, dtype=np.float64)
        f0 = np.ascontiguousarray(f0, dtype=np.float64)
        row_unit = np.ascontiguousarray(row_unit, dtype=np.float64)
        assert status.shape == (self.N,) and (unit is None or unit.shape == (self.N,))
        assert f0.shape == row_unit.shape == (k,)
        if summaries is None:
            summaries = np.zeros(k, SUMMARY)
        assert summaries.dtype == SUMMARY and summaries.flags.c_contiguous and len(summaries) >= k
        if capacity is None:
            capacity = k * self.n
        starts = np.zeros(k + 1, np.int64) if lists else None
        cols = np.zeros(max(1, capacity), np.int32) if lists else None
        vals = np.zeros(max(1, capacity), np.float64) if lists else None
        rc = api().column_cuts_panel(self.h, _p(Y), k, _p(status), _p(unit), _p(f0), _p(row_unit),
                                     zero_tolerance, drop_tolerance, _p(starts), _p(cols),
                                     _p(vals), capacity, _p(summaries))
        if rc == devop_panel_sparse.CAPACITY:
            raise devop_panel_sparse.CapacityError(self._a.last_error(self.h).decode())
        self._check(rc)
        if not lists:
            return None, None, None, summaries[:k]
        kept = int(starts[k])
        return starts, cols[:kept], vals[:kept], summaries[:k]

    def last_cuts(self):
        p = Cuts()
        self._check(api().last_cuts(self.h, ctypes.byref(p)))
        return {"sparse": devop_panel.PANEL_SPARSE[p.sparse], "dense": bool(p.dense),
                "panels": p.panels, "width": p.width, "tiles": p.tiles,
                "structural_tiles": p.structural_tiles, "lists": bool(p.lists), "kept": p.kept,
                "bytes_down": p.bytes_down}
