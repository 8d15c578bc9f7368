"""The probe entries appended after last_bound_propagate
(include/mi_lp_devop.h): column_penalties_panel, last_penalties.

TEST INFRASTRUCTURE ONLY. PenaltiesDevOp is
devop_bound_propagate.BoundPropagateDevOp (every older entry goes through the
older bindings of the table's prefix) plus these calls, bound here through the
longer struct. A library without the entries is an error, never a skip: api()
refuses a library that lacks mi_lp_row_penalties (the table of such a library
ends before these entries).
"""
import ctypes

import numpy as np

import devop_bound_propagate as dbp
import devop_panel
from mi_glop import engine

RECORD = engine.BRANCH_PENALTY

_vp = ctypes.c_void_p
_i = ctypes.c_int


class Penalties(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in ("sparse", "dense", "panels", "width", "tiles",
                                               "reserved")] +
                [("bytes_down", ctypes.c_int64)])


class PenaltiesApi(ctypes.Structure):
    _fields_ = dbp.BoundPropagateApi._fields_ + [
        ("column_penalties_panel", ctypes.CFUNCTYPE(_i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp,
                                                    ctypes.c_double, _vp)),
        ("last_penalties", ctypes.CFUNCTYPE(_i, _vp, ctypes.POINTER(Penalties))),
    ]


_api = None


def api():
    global _api
    if _api is None:
        lib = engine.lib()
        assert hasattr(lib, "mi_lp_row_penalties"), \
            "the library has no branching penalties (mi_devop_table ends before them)"
        _api = PenaltiesApi.in_dll(lib, "mi_devop_table")
    return _api


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


class PenaltiesDevOp(dbp.BoundPropagateDevOp):
    def column_penalties_panel(self, Y, d, status, unit, down, up, pivot_tolerance, out=None):
        """Y: (k, m); d, status (int8): N; unit: N or None; down, up: k.
        Returns k records (engine.BRANCH_PENALTY); `out` (at least k records)
        receives them in place when given."""
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        assert Y.ndim == 2 and Y.shape[1] == self.m
        k = Y.shape[0]
        d = np.ascontiguousarray(d, dtype=np.float64)
        status = np.ascontiguousarray(status, dtype=np.int8)
        unit = None if unit is None else np.ascontiguousarray(unit, dtype=np.float64)
        down = np.ascontiguousarray(down, dtype=np.float64)
        up = np.ascontiguousarray(up, dtype=np.float64)
        assert d.shape == status.shape == (self.N,) and (unit is None or unit.shape == (self.N,))
        assert down.shape == up.shape == (k,)
        if out is None:
            out = np.zeros(k, RECORD)
        assert out.dtype == RECORD and out.flags.c_contiguous and len(out) >= k
        self._check(api().column_penalties_panel(self.h, _p(Y), k, _p(d), _p(status), _p(unit),
                                                 _p(down), _p(up), pivot_tolerance, _p(out)))
        return out[:k]

    def last_penalties(self):
        p = Penalties()
        self._check(api().last_penalties(self.h, ctypes.byref(p)))
        return {"sparse": devop_panel.PANEL_SPARSE[p.sparse], "dense": bool(p.dense),
                "panels": p.panels, "width": p.width, "tiles": p.tiles,
                "bytes_down": p.bytes_down}
