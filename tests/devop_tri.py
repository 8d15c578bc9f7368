"""The probe entries appended after last_cuts (include/mi_lp_devop.h): the
device triangular solves on a matrix of the test's own -- tri_set_matrix,
tri_solve, tri_solve_pair, tri_async_begin / finish / drop, tri_host_solve,
last_tri and last_tri_level_widths.

TEST INFRASTRUCTURE ONLY. TriDevOp is devop_cuts.CutsDevOp (every older entry
goes through the older bindings of the table's prefix) plus these calls, bound
here through the longer struct. A library without the entries is an error,
never a skip: api() refuses a library whose mi_devop_table is shorter than the
struct bound here.
"""
import ctypes
import re
import subprocess

import numpy as np

import devop_cuts
from mi_glop import engine

KINDS = ("upper_t", "lower", "upper_t_up", "lower_t", "unit_row", "upper")
PLANS = ("none", "trivial", "sync_free", "persistent", "levels", "dense_tail")

_vp = ctypes.c_void_p
_i = ctypes.c_int
_u64 = ctypes.c_uint64
_ip = ctypes.POINTER(ctypes.c_int)


class Tri(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in
                 ("plan", "kind", "rows", "first_col", "top", "work", "pos", "levels",
                  "chain_levels", "level0_end", "wide_runs", "chain_runs", "chip_launches",
                  "cu_runs", "fused0", "vectors", "max_wide_run", "max_entries")] +
                [("rows_over", ctypes.c_int32 * 3)] +
                [(n, ctypes.c_int32) for n in ("t", "tail_cols", "blocks")] +
                [("entries", ctypes.c_int64)])


class TriApi(ctypes.Structure):
    _fields_ = devop_cuts.CutsApi._fields_ + [
        ("tri_set_matrix", ctypes.CFUNCTYPE(_i, _vp, _i, _vp, _vp, _vp, _vp)),
        ("tri_solve", ctypes.CFUNCTYPE(_i, _vp, _i, _u64, _i, _vp, _ip)),
        ("tri_solve_pair", ctypes.CFUNCTYPE(_i, _vp, _i, _u64, _vp, _vp, _ip)),
        ("tri_async_begin", ctypes.CFUNCTYPE(_i, _vp, _u64, _vp, _ip)),
        ("tri_async_finish", ctypes.CFUNCTYPE(_i, _vp, _vp)),
        ("tri_async_drop", ctypes.CFUNCTYPE(_i, _vp)),
        ("tri_host_solve", ctypes.CFUNCTYPE(_i, _vp, _i, _i, _vp)),
        ("last_tri", ctypes.CFUNCTYPE(_i, _vp, ctypes.POINTER(Tri))),
        ("last_tri_level_widths", ctypes.CFUNCTYPE(_i, _vp, _vp, _i, _ip)),
    ]


_api = None


def api():
    global _api
    if _api is None:
        lib = engine.lib()
        # The table's size as the dynamic symbol table states it.
        out = subprocess.run(["nm", "-D", "-S", "--defined-only", engine.LIB_PATH],
                             capture_output=True, text=True, check=True).stdout
        size = re.search(r"^[0-9a-f]+ ([0-9a-f]+) \w mi_devop_table$", out, re.M)
        assert size is not None and int(size.group(1), 16) >= ctypes.sizeof(TriApi), \
            "the library has no triangular-solve probe (mi_devop_table ends before it)"
        _api = TriApi.in_dll(lib, "mi_devop_table")
    return _api


def _p(a):
    return a.ctypes.data_as(_vp)


class TriDevOp(devop_cuts.CutsDevOp):
    """A handle over a 1 x 1 [A | I]: only the triangular entries are used."""

    def __init__(self, device=0):
        super().__init__(1, 1, np.array([0, 1]), np.array([0]), np.array([1.0]), device)
        api()
        self.tri_n = 0

    def tri_set_matrix(self, t):
        """t: tri_ref.Tri (or anything with n, starts, rows, vals, diag)."""
        starts = np.ascontiguousarray(t.starts, dtype=np.int64)
        rows = np.ascontiguousarray(t.rows, dtype=np.int32)
        vals = np.ascontiguousarray(t.vals, dtype=np.float64)
        diag = np.ascontiguousarray(t.diag, dtype=np.float64)
        assert len(starts) == t.n + 1 and len(diag) == t.n and len(rows) == len(vals) == starts[-1]
        if len(rows) == 0:
            rows, vals = np.zeros(1, np.int32), np.zeros(1, np.float64)
        self._check(api().tri_set_matrix(self.h, int(t.n), _p(starts), _p(rows), _p(vals),
                                         _p(diag)))
        self.tri_n = int(t.n)

    def _x(self, x):
        x = np.array(x, dtype=np.float64)
        assert x.shape == (self.tri_n,)
        return x

    def tri_solve(self, kind, key, x, start=0):
        """(on_device, x): x is a copy, the input's bits when not on device."""
        x = self._x(x)
        on = ctypes.c_int(-1)
        self._check(api().tri_solve(self.h, int(kind), int(key), int(start), _p(x),
                                    ctypes.byref(on)))
        return bool(on.value), x

    def tri_solve_pair(self, kind, key, x0, x1):
        x0, x1 = self._x(x0), self._x(x1)
        on = ctypes.c_int(-1)
        self._check(api().tri_solve_pair(self.h, int(kind), int(key), _p(x0), _p(x1),
                                         ctypes.byref(on)))
        return bool(on.value), x0, x1

    def tri_async_begin(self, key, x):
        x = self._x(x)
        started = ctypes.c_int(-1)
        self._check(api().tri_async_begin(self.h, int(key), _p(x), ctypes.byref(started)))
        return bool(started.value)

    def tri_async_finish(self, x):
        x = self._x(x)
        self._check(api().tri_async_finish(self.h, _p(x)))
        return x

    def tri_async_drop(self):
        self._check(api().tri_async_drop(self.h))

    def tri_host_solve(self, kind, x, start=0):
        x = self._x(x)
        self._check(api().tri_host_solve(self.h, int(kind), int(start), _p(x)))
        return x

    def last_tri(self):
        p = Tri()
        self._check(api().last_tri(self.h, ctypes.byref(p)))
        d = {n: getattr(p, n) for n, _ in Tri._fields_ if n not in ("plan", "kind", "rows_over")}
        d.update(plan=PLANS[p.plan], kind=KINDS[p.kind], rows_over=list(p.rows_over),
                 fused0=bool(p.fused0))
        return d

    def last_tri_level_widths(self):
        count = ctypes.c_int(0)
        self._check(api().last_tri_level_widths(self.h, None, 0, ctypes.byref(count)))
        w = np.zeros(max(1, count.value), np.int32)
        self._check(api().last_tri_level_widths(self.h, _p(w), len(w), ctypes.byref(count)))
        return w[:count.value].tolist()
