"""The probe's row-deletion entries (include/mi_lp_devop.h
mi_devop_matrix_delete_table): delete_rows and last_delete.

TEST INFRASTRUCTURE ONLY. DeleteDevOp is devop_matrix.MatrixDevOp (append_rows
and fetch_matrix are its own) plus these calls, bound here through the third
table. A library without that table is an error, never a skip.
"""
import ctypes

import numpy as np

import devop_matrix
from mi_glop import engine

MOVE_PER_THREAD = devop_matrix.MOVE_COLUMN_PER_THREAD
MOVE_PER_WORKGROUP = devop_matrix.MOVE_COLUMN_PER_WORKGROUP

_vp = ctypes.c_void_p
_i = ctypes.c_int


class Delete(ctypes.Structure):
    _fields_ = [("path", ctypes.c_int32), ("rows", ctypes.c_int32), ("entries", ctypes.c_int64),
                ("bytes_up", ctypes.c_int64), ("column_shapes", ctypes.c_int32),
                ("row_shapes", ctypes.c_int32), ("device_ms", ctypes.c_double)]


class DeleteApi(ctypes.Structure):
    _fields_ = [
        ("delete_rows", ctypes.CFUNCTYPE(_i, _vp, _vp)),
        ("last_delete", ctypes.CFUNCTYPE(_i, _vp, ctypes.POINTER(Delete))),
    ]


_api = None


def api():
    global _api
    if _api is None:
        try:
            _api = DeleteApi.in_dll(engine.lib(), "mi_devop_matrix_delete_table")
        except ValueError as e:
            raise AssertionError("the library has no delete-rows probe "
                                 "(mi_devop_matrix_delete_table)") from e
    return _api


class DeleteDevOp(devop_matrix.MatrixDevOp):
    def __init__(self, m, n, col_starts, row_idx, vals, device=0):
        api()
        super().__init__(m, n, col_starts, row_idx, vals, device)

    def delete_rows(self, mask, entries):
        """mask: m booleans, True deletes; entries: the structural entries of
        the deleted rows (the caller's own count, which sizes fetch_matrix)."""
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        assert mask.shape == (self.m,)
        self._check(api().delete_rows(self.h, mask.ctypes.data_as(_vp) if self.m else None))
        d = int(np.count_nonzero(mask))
        self.m -= d
        self.N -= d
        self.nnz -= int(entries) + d

    def fetch_matrix(self, dense_columns=None):
        """MatrixDevOp.fetch_matrix; with dense_columns, the caller's bound on
        the dense columns, the block's buffer has room for that many only
        (the default, n * m values, is too much where both are large)."""
        if dense_columns is None:
            return super().fetch_matrix()
        out = {"starts": np.zeros(self.N + 1, np.int64), "rows": np.zeros(self.nnz, np.int32),
               "vals": np.zeros(self.nnz, np.float64), "t_starts": np.zeros(self.m + 1, np.int64),
               "t_cols": np.zeros(self.nnz, np.int32), "t_vals": np.zeros(self.nnz, np.float64)}
        dense_cols = np.zeros(max(1, self.n), np.int32)
        capacity = max(1, dense_columns * self.m)
        block = np.zeros(capacity, np.float64)
        nd = ctypes.c_int32(-1)
        p = devop_matrix._p
        self._check(devop_matrix.api().fetch_matrix(
            self.h, *[p(out[key]) for key in ("starts", "rows", "vals", "t_starts", "t_cols",
                                              "t_vals")],
            ctypes.byref(nd), p(dense_cols), p(block), capacity))
        out["dense_cols"] = dense_cols[:nd.value].copy()
        out["dense_block"] = block[:nd.value * self.m].copy()
        return out

    def last_delete(self):
        p = Delete()
        self._check(api().last_delete(self.h, ctypes.byref(p)))
        return {"path": p.path, "rows": p.rows, "entries": p.entries, "bytes_up": p.bytes_up,
                "column_shapes": p.column_shapes, "row_shapes": p.row_shapes,
                "device_ms": p.device_ms}
