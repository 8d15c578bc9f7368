"""The probe entries appended after last_paths (include/mi_lp_devop.h):
column_dots_panel, last_panel, take_kernel_ms.

TEST INFRASTRUCTURE ONLY. PanelDevOp is devop.DevOp (every older entry goes
through devop's own binding of the table's prefix) plus the panel calls,
bound here through the longer struct.
"""
import ctypes

import numpy as np

import devop
from mi_glop import engine

PANEL_SPARSE = ("none", "short_columns", "long_columns")

_vp = ctypes.c_void_p
_i = ctypes.c_int
_dp = ctypes.POINTER(ctypes.c_double)


class Panel(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("sparse", "dense", "panels", "width")]


class PanelApi(ctypes.Structure):
    _fields_ = devop.Api._fields_ + [
        ("column_dots_panel", ctypes.CFUNCTYPE(_i, _vp, _vp, _i, _vp)),
        ("last_panel", ctypes.CFUNCTYPE(_i, _vp, ctypes.POINTER(Panel))),
        ("take_kernel_ms", ctypes.CFUNCTYPE(_i, _vp, _dp, _dp)),
    ]


_api = None


def api():
    global _api
    if _api is None:
        _api = PanelApi.in_dll(engine.lib(), "mi_devop_table")
    return _api


class PanelDevOp(devop.DevOp):
    def column_dots_panel(self, Y, out=None):
        """Y: (k, m). Returns (k, N); `out` (at least k x N doubles, C order)
        receives the result in place when given."""
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        assert Y.ndim == 2 and Y.shape[1] == self.m
        k = Y.shape[0]
        if out is None:
            out = np.zeros((k, self.N), np.float64)
        assert out.flags.c_contiguous and out.dtype == np.float64 and out.size >= k * self.N
        self._check(api().column_dots_panel(self.h, Y.ctypes.data_as(_vp), k,
                                            out.ctypes.data_as(_vp)))
        return out

    def last_panel(self):
        p = Panel()
        self._check(api().last_panel(self.h, ctypes.byref(p)))
        return {"sparse": PANEL_SPARSE[p.sparse], "dense": bool(p.dense), "panels": p.panels,
                "width": p.width}

    def take_kernel_ms(self):
        """(panel kernels, list_dots kernels) device-event ms since the last call."""
        a, b = ctypes.c_double(), ctypes.c_double()
        self._check(api().take_kernel_ms(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value
