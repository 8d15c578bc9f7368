"""ctypes binding of the device-operation probe (include/mi_lp_devop.h).

TEST INFRASTRUCTURE ONLY: one DeviceLp operation per call, with inputs the
test chooses. Not part of the mi_glop package. DevOp() reads the MILP_*
environment switches at creation, so set the environment first.
"""
import ctypes

import numpy as np

from mi_glop import engine

ROW_PATHS = ("none", "small_serial", "small_serial_256", "small_by_column", "medium_direct",
             "medium_batched", "list", "full_rows", "chunk", "by_column", "column_wise_small",
             "column_wise_general")
COMPACT_PATHS = ("none", "small", "chip_wide")
RATIO_PATHS = ("none", "one_workgroup", "two_kernels")

MASK_RELEVANT = 0

_vp = ctypes.c_void_p
_i = ctypes.c_int
_d = ctypes.c_double
_ip = ctypes.POINTER(ctypes.c_int)


class Paths(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ("update_row", "compact", "ratio", "ratio_tightened", "list_mapped")]


def _fn(res, *args):
    return ctypes.CFUNCTYPE(res, *args)


class Api(ctypes.Structure):
    _fields_ = [
        ("create", _fn(_vp, _i, _i, _i, _vp, _vp, _vp)),
        ("destroy", _fn(None, _vp)),
        ("last_error", _fn(ctypes.c_char_p, _vp)),
        ("set_mask", _fn(_i, _vp, _i, _vp, _i)),
        ("set_list_mirror", _fn(_i, _vp, _i)),
        ("set_small_batch", _fn(_i, _vp, _i)),
        ("update_row_row_wise", _fn(_i, _vp, _vp, _i, _vp, _i, _d)),
        ("update_row_column_wise", _fn(_i, _vp, _vp, _d, _vp)),
        ("fetch_update_row", _fn(_i, _vp, _vp, _vp, _ip)),
        ("read_coefficient", _fn(_i, _vp, _i, ctypes.POINTER(_d))),
        ("download_coefficients", _fn(_i, _vp, _vp)),
        ("list_dots_over_update_row", _fn(_i, _vp, _vp, _vp, _ip)),
        ("list_dots", _fn(_i, _vp, _vp, _i, _vp, _vp)),
        ("dual_begin", _fn(_i, _vp, _vp, _vp, _vp)),
        ("dual_set_col_bits", _fn(_i, _vp, _vp, _vp, _i)),
        ("dual_ratio_candidates", _fn(_i, _vp, _d, _d, _d, _d, _d, _vp, _vp, _vp, _ip, _ip)),
        ("dual_update_reduced_costs", _fn(_i, _vp, _d, _i, _d, _i)),
        ("dual_download_reduced_costs", _fn(_i, _vp, _vp)),
        ("last_paths", _fn(_i, _vp, ctypes.POINTER(Paths))),
    ]


_api = None


def api():
    global _api
    if _api is None:
        _api = Api.in_dll(engine.lib(), "mi_devop_table")
    return _api


class DevOpError(RuntimeError):
    pass


# Set by any failed call. No test provokes a device error, so one means
# trouble on the device: the GPU tests start nothing more after it.
device_error = None


def _p(a):
    return a.ctypes.data_as(_vp)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def mask_words(bits):
    """bool[N] -> the uint64 words of a column bit mask."""
    bits = np.asarray(bits, dtype=bool)
    pad = (-len(bits)) % 64
    b = np.concatenate([bits, np.zeros(pad, bool)]).reshape(-1, 64)
    return (b.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


class DevOp:
    """One DeviceLp over [A | I]; A (m x n) given in CSC."""

    def __init__(self, m, n, col_starts, row_idx, vals, device=0):
        self._a = api()
        self.m, self.n, self.N = m, n, n + m
        cs = np.ascontiguousarray(col_starts, dtype=np.int64)
        ri, v = _i32(row_idx), _f64(vals)
        self.h = self._a.create(device, m, n, _p(cs), _p(ri), _p(v))
        if not self.h:
            raise DevOpError(self._a.last_error(None).decode())

    def close(self):
        if getattr(self, "h", None):
            self._a.destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        global device_error
        if rc != 0:
            device_error = self._a.last_error(self.h).decode()
            raise DevOpError(device_error)

    def set_mask(self, bits, which=MASK_RELEVANT):
        w = mask_words(bits)
        self._check(self._a.set_mask(self.h, which, _p(w), len(w)))

    def set_list_mirror(self, on):
        self._check(self._a.set_list_mirror(self.h, int(on)))

    def set_small_batch(self, on):
        self._check(self._a.set_small_batch(self.h, int(on)))

    def update_row_row_wise(self, rows, rho, algorithm, drop):
        rows, rho = _i32(rows), _f64(rho)
        assert len(rho) == self.m
        self._check(self._a.update_row_row_wise(self.h, _p(rows), len(rows), _p(rho),
                                                algorithm, drop))

    def update_row_column_wise(self, rho, drop, w=None):
        rho = _f64(rho)
        assert len(rho) == self.m
        wv = None if w is None else _f64(w)
        self._check(self._a.update_row_column_wise(self.h, _p(rho), drop,
                                                   None if wv is None else _p(wv)))

    def fetch_update_row(self):
        pos = np.zeros(self.N, np.int32)
        val = np.zeros(self.N, np.float64)
        cnt = ctypes.c_int()
        self._check(self._a.fetch_update_row(self.h, _p(pos), _p(val), ctypes.byref(cnt)))
        return pos[:cnt.value].copy(), val[:cnt.value].copy()

    def read_coefficient(self, col):
        out = _d()
        self._check(self._a.read_coefficient(self.h, int(col), ctypes.byref(out)))
        return np.float64(out.value)

    def download_coefficients(self):
        out = np.zeros(self.N, np.float64)
        self._check(self._a.download_coefficients(self.h, _p(out)))
        return out

    def list_dots_over_update_row(self, v):
        v = _f64(v)
        assert len(v) == self.m
        out = np.zeros(self.N, np.float64)
        cnt = ctypes.c_int()
        self._check(self._a.list_dots_over_update_row(self.h, _p(v), _p(out), ctypes.byref(cnt)))
        return out[:cnt.value].copy()

    def list_dots(self, cols, v):
        cols, v = _i32(cols), _f64(v)
        assert len(v) == self.m
        out = np.zeros(max(1, len(cols)), np.float64)
        self._check(self._a.list_dots(self.h, _p(cols), len(cols), _p(v), _p(out)))
        return out[:len(cols)].copy()

    def dual_begin(self, rc, colbits, bound_diff):
        rc, bd = _f64(rc), _f64(bound_diff)
        cb = np.ascontiguousarray(colbits, dtype=np.uint8)
        assert len(rc) == len(cb) == len(bd) == self.N
        self._check(self._a.dual_begin(self.h, _p(rc), _p(cb), _p(bd)))

    def dual_set_col_bits(self, cols, bits):
        cols = _i32(cols)
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        self._check(self._a.dual_set_col_bits(self.h, _p(cols), _p(bits), len(cols)))

    def dual_ratio_candidates(self, sign, threshold, harris_tolerance, minimum_delta,
                              variation_magnitude):
        """(col, coeff, rc, list_count) of the kept candidates, in list order."""
        col = np.zeros(self.N, np.int32)
        coeff = np.zeros(self.N, np.float64)
        rc = np.zeros(self.N, np.float64)
        cnt, lc = ctypes.c_int(), ctypes.c_int()
        self._check(self._a.dual_ratio_candidates(
            self.h, sign, threshold, harris_tolerance, minimum_delta, variation_magnitude,
            _p(col), _p(coeff), _p(rc), ctypes.byref(cnt), ctypes.byref(lc)))
        k = cnt.value
        return col[:k].copy(), coeff[:k].copy(), rc[:k].copy(), lc.value

    def dual_update_reduced_costs(self, mult, leaving_col, leaving_value, entering_col):
        self._check(self._a.dual_update_reduced_costs(self.h, mult, int(leaving_col),
                                                      leaving_value, int(entering_col)))

    def dual_download_reduced_costs(self):
        out = np.zeros(self.N, np.float64)
        self._check(self._a.dual_download_reduced_costs(self.h, _p(out)))
        return out

    def paths(self):
        """dict: update_row / compact / ratio (names), ratio_tightened, list_mapped."""
        p = Paths()
        self._check(self._a.last_paths(self.h, ctypes.byref(p)))
        return {"update_row": ROW_PATHS[p.update_row], "compact": COMPACT_PATHS[p.compact],
                "ratio": RATIO_PATHS[p.ratio], "ratio_tightened": bool(p.ratio_tightened),
                "list_mapped": bool(p.list_mapped)}
