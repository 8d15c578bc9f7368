"""The probe's matrix entries (include/mi_lp_devop.h mi_devop_matrix_table):
append_rows, fetch_matrix and last_append.

TEST INFRASTRUCTURE ONLY. MatrixDevOp is devop_cuts.CutsDevOp (every older
entry goes through the bindings of mi_devop_table) plus these calls, bound
here through the second table. A library without that table is an error,
never a skip.
"""
import ctypes

import numpy as np

import devop_cuts
from mi_glop import engine

MOVE_COLUMN_PER_THREAD = 1
MOVE_COLUMN_PER_WORKGROUP = 2

_vp = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64


class Append(ctypes.Structure):
    _fields_ = [("path", ctypes.c_int32), ("rows", ctypes.c_int32), ("entries", ctypes.c_int64),
                ("bytes_up", ctypes.c_int64), ("move_shapes", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("device_ms", ctypes.c_double)]


class MatrixApi(ctypes.Structure):
    _fields_ = [
        ("append_rows", ctypes.CFUNCTYPE(_i, _vp, _i, _vp, _vp, _vp)),
        ("fetch_matrix", ctypes.CFUNCTYPE(_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                          ctypes.POINTER(ctypes.c_int32), _vp, _vp, _i64)),
        ("last_append", ctypes.CFUNCTYPE(_i, _vp, ctypes.POINTER(Append))),
    ]


_api = None


def api():
    global _api
    if _api is None:
        try:
            _api = MatrixApi.in_dll(engine.lib(), "mi_devop_matrix_table")
        except ValueError as e:
            raise AssertionError("the library has no append-rows probe "
                                 "(mi_devop_matrix_table)") from e
    return _api


def _p(a):
    return a.ctypes.data_as(_vp) if len(a) else None


class MatrixDevOp(devop_cuts.CutsDevOp):
    def __init__(self, m, n, col_starts, row_idx, vals, device=0):
        api()
        super().__init__(m, n, col_starts, row_idx, vals, device)
        self.nnz = int(np.asarray(col_starts)[-1]) + m  # of [A | I]

    def append_rows(self, row_starts, cols, vals):
        rs = np.ascontiguousarray(row_starts, dtype=np.int64)
        c = np.ascontiguousarray(cols, dtype=np.int32)
        v = np.ascontiguousarray(vals, dtype=np.float64)
        k = len(rs) - 1
        assert k >= 0 and len(c) == len(v) == rs[-1]
        self._check(api().append_rows(self.h, k, _p(rs), _p(c), _p(v)))
        self.m += k
        self.N += k
        self.nnz += int(rs[-1]) + k

    def fetch_matrix(self):
        """dict of the device's arrays: starts / rows / vals (CSC of [A | I]),
        t_starts / t_cols / t_vals (CSR), dense_cols and dense_block."""
        out = {"starts": np.zeros(self.N + 1, np.int64), "rows": np.zeros(self.nnz, np.int32),
               "vals": np.zeros(self.nnz, np.float64), "t_starts": np.zeros(self.m + 1, np.int64),
               "t_cols": np.zeros(self.nnz, np.int32), "t_vals": np.zeros(self.nnz, np.float64)}
        dense_cols = np.zeros(max(1, self.n), np.int32)
        capacity = max(1, self.n * self.m)
        block = np.zeros(capacity, np.float64)
        nd = ctypes.c_int32(-1)
        self._check(api().fetch_matrix(
            self.h, *[_p(out[key]) for key in ("starts", "rows", "vals", "t_starts", "t_cols",
                                               "t_vals")],
            ctypes.byref(nd), _p(dense_cols), _p(block), capacity))
        out["dense_cols"] = dense_cols[:nd.value].copy()
        out["dense_block"] = block[:nd.value * self.m].copy()
        return out

    def last_append(self):
        p = Append()
        self._check(api().last_append(self.h, ctypes.byref(p)))
        return {"path": p.path, "rows": p.rows, "entries": p.entries, "bytes_up": p.bytes_up,
                "move_shapes": p.move_shapes, "device_ms": p.device_ms}
