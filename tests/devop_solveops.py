"""The probe entries appended after panel_sparse_geometry
(include/mi_lp_devop.h): pricing, column_squared_norms, row_sums,
dual_boxed_flips, dual_boxed_flips_early, dual_take_priced_reduced_costs,
dual_set_reduced_cost, last_column_dots, last_flips.

TEST INFRASTRUCTURE ONLY. SolveDevOp is devop_panel_sparse.SparsePanelDevOp
(every older entry goes through the older bindings of the table's prefix)
plus these calls, bound here through the longer struct.
"""
import ctypes

import numpy as np

import devop_panel_sparse
from mi_glop import engine

MASK_BASIC = 1
# DotMode of simplex_kernels.hip.
DOT_MODES = ("update_row_column_wise", "pricing", "list_dots", "full_update_row",
             "update_row_with_dots", "pricing_with_dots")

_vp = ctypes.c_void_p
_i = ctypes.c_int
_d = ctypes.c_double
_ip = ctypes.POINTER(ctypes.c_int)


class ColumnDots(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("mode", "wave_per_col", "dense", "dense_unroll")]


class Flips(ctypes.Structure):
    _fields_ = [("early_taken", ctypes.c_int32)]


class SolveOpsApi(ctypes.Structure):
    _fields_ = devop_panel_sparse.SparsePanelApi._fields_ + [
        ("pricing", ctypes.CFUNCTYPE(_i, _vp, _vp, _vp, _vp, _vp, _vp, _ip)),
        ("column_squared_norms", ctypes.CFUNCTYPE(_i, _vp, _vp)),
        ("row_sums", ctypes.CFUNCTYPE(_i, _vp, _vp, _i, _d, _vp)),
        ("dual_boxed_flips", ctypes.CFUNCTYPE(_i, _vp, _vp, _i, _d, _vp)),
        ("dual_boxed_flips_early", ctypes.CFUNCTYPE(_i, _vp, _vp, _i, _d)),
        ("dual_take_priced_reduced_costs", ctypes.CFUNCTYPE(_i, _vp)),
        ("dual_set_reduced_cost", ctypes.CFUNCTYPE(_i, _vp, _i, _d)),
        ("last_column_dots", ctypes.CFUNCTYPE(_i, _vp, ctypes.POINTER(ColumnDots))),
        ("last_flips", ctypes.CFUNCTYPE(_i, _vp, ctypes.POINTER(Flips))),
    ]


_api = None


def api():
    global _api
    if _api is None:
        _api = SolveOpsApi.in_dll(engine.lib(), "mi_devop_table")
    return _api


def _p(a):
    return a.ctypes.data_as(_vp)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class SolveDevOp(devop_panel_sparse.SparsePanelDevOp):
    def pricing(self, c, y, w=None):
        """rc[N]; with w also the dots over the last update row's list, in list
        order: (rc, list_dots). fetch_update_row comes first."""
        c, y = _f64(c), _f64(y)
        assert len(c) == self.N and len(y) == self.m
        wv = None if w is None else _f64(w)
        assert wv is None or len(wv) == self.m
        rc = np.zeros(self.N, np.float64)
        dots = np.zeros(self.N, np.float64)
        cnt = ctypes.c_int(-1)
        self._check(api().pricing(self.h, _p(c), _p(y), None if wv is None else _p(wv), _p(rc),
                                  _p(dots), ctypes.byref(cnt)))
        if w is None:
            assert cnt.value == 0
            return rc
        return rc, dots[:cnt.value].copy()

    def column_squared_norms(self):
        out = np.zeros(self.N, np.float64)
        self._check(api().column_squared_norms(self.h, _p(out)))
        return out

    def row_sums(self, x, skip_basic, sign):
        x = _f64(x)
        assert len(x) == self.N
        out = np.zeros(self.m, np.float64)
        self._check(api().row_sums(self.h, _p(x), int(bool(skip_basic)), float(sign), _p(out)))
        return out

    def dual_boxed_flips(self, cols, threshold):
        """uint8 flags: one per listed column, or one per column (cols None)."""
        if cols is None:
            flags = np.full(self.N, 0xEE, np.uint8)
            self._check(api().dual_boxed_flips(self.h, None, 0, float(threshold), _p(flags)))
            return flags
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        flags = np.full(max(1, len(cols)), 0xEE, np.uint8)
        self._check(api().dual_boxed_flips(self.h, _p(cols), len(cols), float(threshold),
                                           _p(flags)))
        return flags[:len(cols)].copy()

    def dual_boxed_flips_early(self, cols, threshold):
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        self._check(api().dual_boxed_flips_early(self.h, _p(cols), len(cols), float(threshold)))

    def dual_take_priced_reduced_costs(self):
        self._check(api().dual_take_priced_reduced_costs(self.h))

    def dual_set_reduced_cost(self, col, value):
        assert 0 <= col < self.N
        self._check(api().dual_set_reduced_cost(self.h, int(col), float(value)))

    def last_column_dots(self):
        p = ColumnDots()
        self._check(api().last_column_dots(self.h, ctypes.byref(p)))
        return {"mode": DOT_MODES[p.mode] if 0 <= p.mode < len(DOT_MODES) else "none",
                "wave_per_col": bool(p.wave_per_col), "dense": bool(p.dense),
                "dense_unroll": p.dense_unroll}

    def last_flips(self):
        p = Flips()
        self._check(api().last_flips(self.h, ctypes.byref(p)))
        return {"early_taken": bool(p.early_taken)}

    def set_basic_mask(self, bits):
        self.set_mask(bits, which=MASK_BASIC)
