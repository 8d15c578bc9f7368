"""The probe entries appended after take_kernel_ms (include/mi_lp_devop.h):
column_dots_panel_sparse, last_panel_sparse, panel_sparse_geometry.

TEST INFRASTRUCTURE ONLY. SparsePanelDevOp is devop_panel.PanelDevOp (every
older entry goes through the older bindings of the table's prefix) plus the
sparse panel calls, bound here through the longer struct.
"""
import ctypes

import numpy as np

import devop
import devop_panel
from mi_glop import engine

CAPACITY = 2  # MI_DEVOP_CAPACITY

_vp = ctypes.c_void_p
_i = ctypes.c_int


class PanelSparse(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in ("sparse", "dense", "panels", "width")] +
                [(n, ctypes.c_int64) for n in ("kept", "bytes_down")])


class Geometry(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("tile_columns", "offsets_step_tiles")]


class SparsePanelApi(ctypes.Structure):
    _fields_ = devop_panel.PanelApi._fields_ + [
        ("column_dots_panel_sparse", ctypes.CFUNCTYPE(_i, _vp, _vp, _i, ctypes.c_double, _vp, _vp,
                                                      _vp, _vp, ctypes.c_int64)),
        ("last_panel_sparse", ctypes.CFUNCTYPE(_i, _vp, ctypes.POINTER(PanelSparse))),
        ("panel_sparse_geometry", ctypes.CFUNCTYPE(_i, ctypes.POINTER(Geometry))),
    ]


_api = None


def api():
    global _api
    if _api is None:
        _api = SparsePanelApi.in_dll(engine.lib(), "mi_devop_table")
    return _api


def geometry():
    g = Geometry()
    assert api().panel_sparse_geometry(ctypes.byref(g)) == 0
    return {"tile_columns": g.tile_columns, "offsets_step_tiles": g.offsets_step_tiles}


class CapacityError(RuntimeError):
    """The result has more entries than the buffers hold: no device error."""


class SparsePanelDevOp(devop_panel.PanelDevOp):
    def column_dots_panel_sparse(self, Y, drop_tolerance, keep=None, capacity=None,
                                 row_starts=None, cols=None, vals=None):
        """Y: (k, m); keep: bool[N] or None (all columns). Returns (row_starts
        [k + 1], cols, vals) cut to the result; the buffers, when given, receive
        it in place (capacity defaults to their length, or to k * N)."""
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        assert Y.ndim == 2 and Y.shape[1] == self.m
        k = Y.shape[0]
        if capacity is None:
            capacity = k * self.N if cols is None else len(cols)
        if row_starts is None:
            row_starts = np.zeros(k + 1, np.int64)
        if cols is None:
            cols = np.zeros(max(1, capacity), np.int32)
        if vals is None:
            vals = np.zeros(max(1, capacity), np.float64)
        assert row_starts.dtype == np.int64 and len(row_starts) >= k + 1
        assert cols.dtype == np.int32 and vals.dtype == np.float64
        assert len(cols) >= capacity and len(vals) >= capacity
        words = None if keep is None else devop.mask_words(keep)
        assert words is None or len(words) == (self.N + 63) // 64
        rc = api().column_dots_panel_sparse(
            self.h, Y.ctypes.data_as(_vp), k, drop_tolerance,
            None if words is None else words.ctypes.data_as(_vp), row_starts.ctypes.data_as(_vp),
            cols.ctypes.data_as(_vp), vals.ctypes.data_as(_vp), capacity)
        if rc == CAPACITY:
            raise CapacityError(self._a.last_error(self.h).decode())
        self._check(rc)
        kept = int(row_starts[k])
        return row_starts[:k + 1], cols[:kept], vals[:kept]

    def last_panel_sparse(self):
        p = PanelSparse()
        self._check(api().last_panel_sparse(self.h, ctypes.byref(p)))
        return {"sparse": devop_panel.PANEL_SPARSE[p.sparse], "dense": bool(p.dense),
                "panels": p.panels, "width": p.width, "kept": p.kept,
                "bytes_down": p.bytes_down}
