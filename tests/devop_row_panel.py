"""The probe entries appended after last_flips (include/mi_lp_devop.h):
row_sums_panel, row_sums_panel_from, last_row_panel, row_panel_geometry.

TEST INFRASTRUCTURE ONLY. RowPanelDevOp is devop_solveops.SolveDevOp (every
older entry goes through the older bindings of the table's prefix) plus these
calls, bound here through the longer struct.
"""
import ctypes

import numpy as np

import devop_solveops
from mi_glop import engine

ROW_PANEL_KERNELS = ("none", "direct")  # MI_DEVOP_ROW_PANEL_*

_vp = ctypes.c_void_p
_i = ctypes.c_int


class RowPanel(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in ("panels", "width", "kernel", "reserved")] +
                [("overrides_up_bytes", ctypes.c_int64)])


class Geometry(ctypes.Structure):
    _fields_ = [("rows_per_workgroup", ctypes.c_int32 * 3), ("chunk", ctypes.c_int32)]


class RowPanelApi(ctypes.Structure):
    _fields_ = devop_solveops.SolveOpsApi._fields_ + [
        ("row_sums_panel", ctypes.CFUNCTYPE(_i, _vp, _vp, _i, _vp)),
        ("row_sums_panel_from", ctypes.CFUNCTYPE(_i, _vp, _vp, _i, _vp, _vp, _vp, _vp)),
        ("last_row_panel", ctypes.CFUNCTYPE(_i, _vp, ctypes.POINTER(RowPanel))),
        ("row_panel_geometry", ctypes.CFUNCTYPE(_i, ctypes.POINTER(Geometry))),
    ]


_api = None


def api():
    global _api
    if _api is None:
        _api = RowPanelApi.in_dll(engine.lib(), "mi_devop_table")
    return _api


def geometry():
    """Rows per workgroup at the widths 1, 4 and 16, and the staging chunk
    length (0: the kernel does not stage)."""
    g = Geometry()
    assert api().row_panel_geometry(ctypes.byref(g)) == 0
    return {"rows_per_workgroup": dict(zip((1, 4, 16), g.rows_per_workgroup)), "chunk": g.chunk}


def _p(a):
    return a.ctypes.data_as(_vp)


class RowPanelDevOp(devop_solveops.SolveDevOp):
    def _out(self, k, out):
        if out is None:
            return np.zeros(k * self.m, np.float64)
        assert out.dtype == np.float64 and out.flags.c_contiguous and out.size >= k * self.m
        return out

    def row_sums_panel(self, X, out=None):
        """X: (k, N). Returns (k, m); `out` (flat, at least k * m) receives it
        in place."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        assert X.ndim == 2 and X.shape[1] == self.N
        k = X.shape[0]
        out = self._out(k, out)
        self._check(api().row_sums_panel(self.h, _p(X), k, _p(out)))
        return out[:k * self.m].reshape(k, self.m)

    def row_sums_panel_from(self, base, starts, cols, vals, out=None):
        """base: N; starts (k + 1), cols, vals as row_panel_cases.flatten."""
        base = np.ascontiguousarray(base, dtype=np.float64)
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        assert len(base) == self.N and len(cols) == len(vals) == starts[-1]
        k = len(starts) - 1
        out = self._out(k, out)
        self._check(api().row_sums_panel_from(
            self.h, _p(base), k, _p(starts), _p(cols) if len(cols) else None,
            _p(vals) if len(vals) else None, _p(out)))
        return out[:k * self.m].reshape(k, self.m)

    def last_row_panel(self):
        p = RowPanel()
        self._check(api().last_row_panel(self.h, ctypes.byref(p)))
        return {"panels": p.panels, "width": p.width, "kernel": ROW_PANEL_KERNELS[p.kernel],
                "overrides_up_bytes": p.overrides_up_bytes}
