"""ctypes binding of the MI355X engine (or-tools_amd/lib/libmi_lp.so).

This is the product path: every solve runs the HIP kernels. There is no CPU
fallback: if the library or a GPU is missing, creating a handle raises.
"""
import ctypes
import os
import subprocess

import numpy as np

from . import abi

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("MI_LP_LIB") or os.path.join(PKG_DIR, "lib", "libmi_lp.so")

_lib = None


class EngineUnavailable(RuntimeError):
    pass


# mi_lp_allgather_fn (include/mi_lp.h): ctx, send, send_bytes, recv, recv_bytes.
ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64))
# include/mi_lp.h mi_lp_simplex_fn: the LPSolver's simplex, supplied by the caller.
SIMPLEX_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                              *([ctypes.c_void_p] * 8), ctypes.c_double, ctypes.c_double,
                              ctypes.c_int32, ctypes.c_void_p, *([ctypes.c_void_p] * 4))
# include/mi_lp.h mi_lp_point_violations: one summary per point.
POINT_VIOLATIONS = np.dtype([("count", np.int64), ("worst", np.float64),
                             ("worst_row", np.int32), ("reserved", np.int32)])
assert POINT_VIOLATIONS.itemsize == 24
# include/mi_lp.h mi_lp_branch_penalty: one record per tableau row.
BRANCH_PENALTY = np.dtype([("down", np.float64), ("up", np.float64), ("down_col", np.int32),
                           ("up_col", np.int32), ("down_count", np.int32),
                           ("up_count", np.int32)])
assert BRANCH_PENALTY.itemsize == 32
# include/mi_lp.h mi_lp_cut_summary: one record per Gomory cut.
CUT_SUMMARY = np.dtype([("max_abs", np.float64), ("min_abs", np.float64), ("count", np.int32),
                        ("bad_count", np.int32), ("max_col", np.int32), ("min_col", np.int32)])
assert CUT_SUMMARY.itemsize == 32
# mi_lp_propagation (include/mi_lp.h) as a numpy record.
PROPAGATION = np.dtype([("status", np.int32), ("rounds", np.int32), ("moves", np.int64),
                        ("worst", np.float64), ("worst_col", np.int32), ("kept", np.int32)])
assert PROPAGATION.itemsize == 32
PROPAGATE_ROUND_LIMIT, PROPAGATE_FIXPOINT, PROPAGATE_INFEASIBLE = 0, 1, 2


def build(jobs=8):
    """Compiles the engine for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-s", f"-j{jobs}", "-C", PKG_DIR], check=True)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineUnavailable(
            f"{LIB_PATH} is missing: run `make -C or-tools_amd` (no CPU fallback)")
    L = ctypes.CDLL(LIB_PATH)
    vp = ctypes.c_void_p
    L.mi_glop_params_default.argtypes = [ctypes.POINTER(abi.MiGlopParams)]
    L.mi_lp_device_count.restype = ctypes.c_int
    L.mi_lp_shutdown.restype = ctypes.c_int
    # Drain the engine's resident grids and join its service threads while
    # the HIP runtime is still up: Python's atexit runs before the C exit
    # handlers (the runtime's and a profiler's own teardown).
    import atexit
    atexit.register(_shutdown, L)
    # RCCL bound sharing (engine/comm.hip).
    L.mi_lp_comm_get_unique_id.argtypes = [vp]
    L.mi_lp_comm_create.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                    ctypes.POINTER(vp)]
    L.mi_lp_comm_rank.argtypes = [vp]
    L.mi_lp_comm_size.argtypes = [vp]
    L.mi_lp_share_bound.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.c_int32]
    L.mi_lp_comm_allreduce_device.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int32]
    L.mi_lp_comm_allgather_device.argtypes = [vp, vp, vp, ctypes.c_int64]
    L.mi_lp_comm_last_error.argtypes = [vp]
    L.mi_lp_comm_last_error.restype = ctypes.c_char_p
    L.mi_lp_comm_destroy.argtypes = [vp]
    L.mi_lp_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.mi_lp_destroy.argtypes = [vp]
    L.mi_lp_last_error.argtypes = [vp]
    L.mi_lp_last_error.restype = ctypes.c_char_p
    L.mi_lp_set_params.argtypes = [vp, ctypes.POINTER(abi.MiGlopParams)]
    L.mi_lp_load.argtypes = [vp, ctypes.c_int32, ctypes.c_int32] + [vp] * 8 + \
        [ctypes.c_double, ctypes.c_double, ctypes.c_int32]
    L.mi_lp_add_rows.argtypes = [vp, ctypes.c_int32, vp, vp, vp, vp, vp,
                                 ctypes.POINTER(abi.MiLpAppendInfo)]
    L.mi_lp_delete_rows.argtypes = [vp, vp, ctypes.POINTER(abi.MiLpDeleteInfo)]
    L.mi_lp_load_basis_state.argtypes = [vp, vp, ctypes.c_int32]
    L.mi_lp_clear_basis_state.argtypes = [vp]
    L.mi_lp_notify_matrix_unchanged.argtypes = [vp]
    L.mi_lp_solve.argtypes = [vp, vp, ctypes.POINTER(abi.MiLpResult)]
    for name in ["mi_lp_get_primal", "mi_lp_get_reduced_costs", "mi_lp_get_duals",
                 "mi_lp_get_activities", "mi_lp_get_basis", "mi_lp_get_state",
                 "mi_lp_get_primal_ray", "mi_lp_get_dual_ray",
                 "mi_lp_get_dual_ray_row_combination"]:
        getattr(L, name).argtypes = [vp, vp]
    L.mi_lp_get_statuses.argtypes = [vp, vp, vp]
    L.mi_lp_begin.argtypes = [vp, ctypes.c_int64]
    L.mi_lp_run_until.argtypes = [vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32),
                                  ctypes.POINTER(ctypes.c_int64)]
    L.mi_lp_finish.argtypes = [vp, ctypes.POINTER(abi.MiLpResult)]
    L.mi_lp_stop.argtypes = [vp]
    L.mi_lp_get_kernel_stats.argtypes = [vp, ctypes.POINTER(abi.MiLpKernelStats)]
    L.mi_lp_reset_kernel_stats.argtypes = [vp]
    L.mi_lp_set_kernel_timing.argtypes = [vp, ctypes.c_int32]
    L.mi_lp_set_kernel_timing_ids.argtypes = [vp, ctypes.c_uint32]
    L.mi_lp_batch_solve.argtypes = [vp, ctypes.c_int32, ctypes.c_int32,
                                    ctypes.POINTER(abi.MiLpResult)]
    L.mi_lp_set_variable_bounds.argtypes = [vp, vp, vp]
    L.mi_lp_batch_solve_gpus.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                         ctypes.POINTER(abi.MiLpResult)]
    L.mi_lp_batch_solve_bounds.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, vp, vp, vp,
                                           ctypes.c_int32, ctypes.POINTER(abi.MiLpResult)]
    L.mi_lp_notify_matrix_changed.argtypes = [vp]
    L.mi_lp_set_starting_variable_values.argtypes = [vp, vp, ctypes.c_int32]
    L.mi_lp_set_integrality_scale.argtypes = [vp, ctypes.c_int32, ctypes.c_double]
    L.mi_lp_clear_integrality_scales.argtypes = [vp]
    L.mi_lp_record_iteration_times.argtypes = [vp, ctypes.c_int32]
    L.mi_lp_get_iteration_times.argtypes = [vp, vp, ctypes.c_int64]
    L.mi_lp_get_iteration_times.restype = ctypes.c_int64
    L.mi_lp_get_run_counters.argtypes = [vp, ctypes.POINTER(abi.MiLpRunCounters)]
    L.mi_lp_set_exchange.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, vp, ALLGATHER_FN]
    L.mi_exchange_open.argtypes = [ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32,
                                   ctypes.c_int64, ctypes.POINTER(vp)]
    L.mi_exchange_allgather.argtypes = [vp, vp, ctypes.c_int64, vp, ctypes.POINTER(ctypes.c_int64)]
    L.mi_exchange_close.argtypes = [vp]
    L.mi_lp_objective_limit_reached.argtypes = [vp, vp]
    L.mi_lp_get_unit_row_left_inverse.argtypes = [vp, ctypes.c_int32, vp, vp, vp]
    L.mi_lp_compute_dictionary.argtypes = [vp, vp, ctypes.c_int32, vp]
    L.mi_lp_get_dictionary.argtypes = [vp, vp, vp, vp]
    L.mi_lp_row_combinations.argtypes = [vp, vp, ctypes.c_int32, vp]
    L.mi_lp_get_tableau_rows.argtypes = [vp, vp, ctypes.c_int32, vp, vp]
    L.mi_lp_row_combinations_sparse.argtypes = [vp, vp, ctypes.c_int32, ctypes.c_double,
                                                ctypes.c_uint32, vp]
    L.mi_lp_get_tableau_rows_sparse.argtypes = [vp, vp, ctypes.c_int32, ctypes.c_double,
                                                ctypes.c_uint32, vp, vp]
    L.mi_lp_get_sparse_rows.argtypes = [vp, vp, vp]
    L.mi_lp_row_penalties.argtypes = [vp, vp, ctypes.c_int32, vp, vp, vp, vp, vp,
                                      ctypes.c_double, vp]
    L.mi_lp_branching_penalties.argtypes = [vp, vp, ctypes.c_int32, vp, vp, vp, ctypes.c_double,
                                            vp, vp]
    L.mi_lp_row_gomory_cuts.argtypes = [vp, vp, ctypes.c_int32, vp, vp, vp, vp, ctypes.c_double,
                                        ctypes.c_double, vp, vp]
    L.mi_lp_gomory_cuts.argtypes = [vp, vp, ctypes.c_int32, vp, ctypes.c_double, ctypes.c_double,
                                    vp, vp, vp]
    L.mi_lp_get_cut_rows.argtypes = [vp, vp, vp]
    L.mi_lp_column_combinations.argtypes = [vp, vp, ctypes.c_int32, vp]
    L.mi_lp_column_combinations_from.argtypes = [vp, vp, ctypes.c_int32, vp, vp, vp, vp]
    L.mi_lp_column_combinations_violations.argtypes = [vp, vp, ctypes.c_int32, vp, vp,
                                                       ctypes.c_double, vp, vp]
    L.mi_lp_column_combinations_from_violations.argtypes = [vp, vp, ctypes.c_int32, vp, vp, vp,
                                                            vp, vp, ctypes.c_double, vp, vp]
    L.mi_lp_get_violated_rows.argtypes = [vp, vp, vp]
    L.mi_lp_bound_activity_ranges.argtypes = [vp, vp, vp, ctypes.c_int32, vp, vp, vp]
    L.mi_lp_bound_activity_ranges_from.argtypes = [vp, vp, vp, ctypes.c_int32] + [vp] * 7
    L.mi_lp_bound_infeasible_rows.argtypes = [vp, vp, vp, ctypes.c_int32, vp, vp,
                                              ctypes.c_double, vp, vp]
    L.mi_lp_bound_infeasible_rows_from.argtypes = [vp, vp, vp, ctypes.c_int32] + [vp] * 6 + [
        ctypes.c_double, vp, vp]
    L.mi_lp_get_infeasible_rows.argtypes = [vp, vp, vp]
    L.mi_lp_bound_implied_bounds.argtypes = [vp, vp, vp, ctypes.c_int32, vp, vp, vp, vp]
    L.mi_lp_bound_implied_bounds_from.argtypes = [vp, vp, vp, ctypes.c_int32] + [vp] * 8
    L.mi_lp_bound_tightened_columns.argtypes = [vp, vp, vp, ctypes.c_int32, vp, vp,
                                                ctypes.c_double, vp, vp]
    L.mi_lp_bound_tightened_columns_from.argtypes = [vp, vp, vp, ctypes.c_int32] + [vp] * 6 + [
        ctypes.c_double, vp, vp]
    L.mi_lp_get_tightened_columns.argtypes = [vp, vp, vp, vp]
    _rounds = [ctypes.c_double, ctypes.c_double, ctypes.c_int32]
    L.mi_lp_bound_propagate.argtypes = [vp, vp, vp, ctypes.c_int32, vp, vp, vp] + _rounds + [
        vp, vp, vp]
    L.mi_lp_bound_propagate_from.argtypes = [vp, vp, vp, ctypes.c_int32] + [vp] * 7 + _rounds + [
        vp, vp, vp]
    L.mi_lp_bound_propagated_columns_from.argtypes = [vp, vp, vp, ctypes.c_int32] + [vp] * 7 + \
        _rounds + [vp, vp]
    L.mi_lp_get_propagated_columns.argtypes = [vp, vp, vp, vp]
    L.mi_lp_solver_params_default.argtypes = [ctypes.POINTER(abi.MiLpSolverParams)]
    L.mi_lp_scale.argtypes = [ctypes.POINTER(abi.MiLpSolverParams), ctypes.c_int32,
                              ctypes.c_int32] + [vp] * 14
    L.mi_lp_solver_solve.argtypes = [vp, ctypes.POINTER(abi.MiLpSolverParams), ctypes.c_int32,
                                     ctypes.c_int32] + [vp] * 8 + [
        ctypes.c_double, ctypes.c_double, ctypes.c_int32, vp,
        ctypes.POINTER(abi.MiLpResult)] + [vp] * 6
    L.mi_lp_solver_solve_with.argtypes = [SIMPLEX_FN, vp, ctypes.POINTER(abi.MiLpSolverParams),
                                          ctypes.c_int32, ctypes.c_int32] + [vp] * 8 + [
        ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.POINTER(abi.MiLpResult)] + \
        [vp] * 6
    L.mi_presolve_create.restype = vp
    L.mi_presolve_destroy.argtypes = [vp]
    L.mi_presolve_run.argtypes = [vp, ctypes.POINTER(abi.MiLpSolverParams), ctypes.c_int32,
                                  ctypes.c_int32] + [vp] * 8 + [
        ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
    L.mi_presolve_dims.argtypes = [vp] + [vp] * 4
    L.mi_presolve_get.argtypes = [vp] + [vp] * 10
    L.mi_presolve_recover.argtypes = [vp, ctypes.POINTER(ctypes.c_int32)] + [vp] * 8
    L.mi_presolve_num_passes.argtypes = [vp]
    L.mi_presolve_num_passes.restype = ctypes.c_int32
    L.mi_presolve_pass_name.argtypes = [vp, ctypes.c_int32]
    L.mi_presolve_pass_name.restype = ctypes.c_char_p
    _lib = L
    return L


_open_handles = None  # weakref.WeakSet of LpHandle, created with the first


def _shutdown(L):
    """Python exit: destroy the handles still open (their streams and device
    memory) and then the engine's shared device objects, before the HIP
    runtime and any profiler attached to it tear down."""
    if _open_handles is not None:
        for h in list(_open_handles):
            try:
                h.close()
            except Exception:  # noqa: BLE001 (exit path)
                pass
    L.mi_lp_shutdown()


def device_count():
    return lib().mi_lp_device_count()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def allgather_callback(world, allgather):
    """A mi_lp_allgather_fn over a Python `allgather(data, sizes) -> bytes`.
    Failures return 1 (no exception may cross the C ABI; the engine then
    raises a DeviceError for the solve)."""
    def cb(_ctx, send, send_bytes, recv, recv_bytes):
        try:
            sizes = [int(recv_bytes[r]) for r in range(world)]
            data = ctypes.string_at(send, send_bytes) if send_bytes > 0 else b""
            out = allgather(data, sizes)
            if len(out) != sum(sizes):
                return 1
            if out:
                ctypes.memmove(recv, out, len(out))
            return 0
        except Exception:  # noqa: BLE001
            return 1
    return ALLGATHER_FN(cb)


class ShmExchange:
    """Same-node all-gather of host bytes in C++ (mi_exchange_open, engine/
    exchange.cc): the split's joins run without Python. Rank 0 creates the
    segment `name`, the other ranks attach (the call returns once all
    `world` ranks are attached). Needs no GPU."""

    def __init__(self, name, rank, world, slot_bytes=8 << 20):
        self._L = lib()
        x = ctypes.c_void_p()
        rc = self._L.mi_exchange_open(name.encode(), int(rank), int(world), int(slot_bytes),
                                      ctypes.byref(x))
        if rc != 0:
            raise RuntimeError(f"mi_exchange_open({name!r}, rank {rank}/{world}) failed with {rc}")
        self.x = x
        self.rank, self.world = int(rank), int(world)

    def allgather(self, data, sizes):
        """Every rank's bytes in rank order (sizes[r] from rank r)."""
        send = ctypes.create_string_buffer(bytes(data), max(1, len(data)))
        recv = ctypes.create_string_buffer(max(1, sum(sizes)))
        arr = (ctypes.c_int64 * self.world)(*sizes)
        rc = self._L.mi_exchange_allgather(self.x, send, len(data), recv, arr)
        if rc != 0:
            raise RuntimeError(f"mi_exchange_allgather failed with {rc}")
        return recv.raw[:sum(sizes)]

    def function(self):
        """(ctx, mi_lp_allgather_fn) for mi_lp_set_exchange: the C function."""
        addr = ctypes.cast(self._L.mi_exchange_allgather, ctypes.c_void_p).value
        return self.x, ALLGATHER_FN(addr)

    def close(self):
        if getattr(self, "x", None):
            self._L.mi_exchange_close(self.x)
            self.x = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LpHandle:
    """One RevisedSimplex on one GPU (include/mi_lp.h)."""

    def __init__(self, params=None, device=0):
        self._L = lib()
        h = ctypes.c_void_p()
        rc = self._L.mi_lp_create(int(device), ctypes.byref(h))
        if rc != 0:
            raise EngineUnavailable(f"mi_lp_create(device={device}) failed with {rc}: "
                                    "no usable MI355X (there is no CPU fallback)")
        self.h = h
        self.params = params or abi.default_params()
        self.lp = None
        global _open_handles
        if _open_handles is None:
            import weakref
            _open_handles = weakref.WeakSet()
        _open_handles.add(self)

    def close(self):
        if getattr(self, "h", None):
            self._L.mi_lp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        msg = self._L.mi_lp_last_error(self.h)
        return msg.decode() if msg else ""

    def _check(self, rc, what):
        if rc != 0:
            msg = self._L.mi_lp_last_error(self.h)
            raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def set_params(self, params):
        self.params = params

    def load(self, lp):
        self.lp = lp
        self._keep = [np.ascontiguousarray(x, dtype=t) for x, t in (
            (lp.col_starts, np.int64), (lp.row_idx, np.int32), (lp.vals, np.float64),
            (lp.col_lb, np.float64), (lp.col_ub, np.float64), (lp.row_lb, np.float64),
            (lp.row_ub, np.float64), (lp.obj, np.float64))]
        cs, ri, v, clb, cub, rlb, rub, ob = self._keep
        self._check(self._L.mi_lp_load(self.h, lp.m, lp.n, _p(cs), _p(ri), _p(v),
                                       _p(clb), _p(cub), _p(rlb), _p(rub), _p(ob),
                                       lp.obj_offset, lp.obj_scale, int(lp.maximize)),
                    "mi_lp_load")

    def add_rows(self, row_starts, cols, vals, row_lb, row_ub):
        """Appends k rows given as lists to the loaded LP (include/mi_lp.h
        mi_lp_add_rows): in every later result it is load(lp.with_rows(...)),
        but only the new rows go to the device, where they are merged into the
        resident matrix. Returns {"path", "rows", "entries", "bytes_up"};
        self.lp becomes the extended LP."""
        rs = np.ascontiguousarray(row_starts, dtype=np.int64)
        c = np.ascontiguousarray(cols, dtype=np.int32)
        v = np.ascontiguousarray(vals, dtype=np.float64)
        lb = np.ascontiguousarray(row_lb, dtype=np.float64)
        ub = np.ascontiguousarray(row_ub, dtype=np.float64)
        k = len(rs) - 1
        if k < 0 or len(lb) != k or len(ub) != k or len(c) != len(v) or rs[-1] != len(c):
            raise ValueError("row_starts, cols / vals and the bounds do not describe k rows")
        info = abi.MiLpAppendInfo()
        self._check(self._L.mi_lp_add_rows(
            self.h, k, _p(rs), _p(c) if len(c) else None, _p(v) if len(v) else None,
            _p(lb) if k else None, _p(ub) if k else None, ctypes.byref(info)), "mi_lp_add_rows")
        if self.lp is not None:
            self.lp = self.lp.with_rows(rs, c, v, lb, ub)
        return {"path": info.path, "rows": info.rows, "entries": info.entries,
                "bytes_up": info.bytes_up}

    def delete_rows(self, rows):
        """Deletes rows from the loaded LP (include/mi_lp.h mi_lp_delete_rows):
        `rows` is a boolean mask of length m or an array of row indices (out of
        range or repeated: ValueError). In every later result it is
        load(lp.without_rows(mask)) followed by load_basis_state of the state
        without the deleted rows' slacks, but only the mask goes to the
        device, where the resident matrix is compacted. Returns {"path",
        "rows", "entries", "bytes_up"}; self.lp becomes the reduced LP."""
        m = self.lp.m
        r = np.asarray(rows)
        if r.dtype == np.bool_:
            if r.shape != (m,):
                raise ValueError("a row mask has one entry per row")
            mask = r
        else:
            if r.size and not np.issubdtype(r.dtype, np.integer):
                raise ValueError("row indices are integers (or pass a boolean mask)")
            idx = r.astype(np.int64).reshape(-1)
            if len(idx) and (idx.min() < 0 or idx.max() >= m):
                raise ValueError("a row index is out of range")
            if len(np.unique(idx)) != len(idx):
                raise ValueError("a row index is repeated")
            mask = np.zeros(m, bool)
            mask[idx] = True
        bytes_ = np.ascontiguousarray(mask, dtype=np.uint8)
        info = abi.MiLpDeleteInfo()
        self._check(self._L.mi_lp_delete_rows(self.h, _p(bytes_) if m else None,
                                              ctypes.byref(info)), "mi_lp_delete_rows")
        self.lp = self.lp.without_rows(mask)
        return {"path": info.path, "rows": info.rows, "entries": info.entries,
                "bytes_up": info.bytes_up}

    def solve_lp(self, lp, solver_params=None, interrupt=None):
        """glop::LPSolver::SolveWithTimeLimit on this handle (mi_lp_solver_solve):
        scaling preprocessor, engine solve, RecoverSolution, solution values of
        the unscaled LP. Returns (result, dict of unscaled solution arrays)."""
        sp = solver_params or abi.default_solver_params()
        keep = [np.ascontiguousarray(x, dtype=t) for x, t in (
            (lp.col_starts, np.int64), (lp.row_idx, np.int32), (lp.vals, np.float64),
            (lp.col_lb, np.float64), (lp.col_ub, np.float64), (lp.row_lb, np.float64),
            (lp.row_ub, np.float64), (lp.obj, np.float64))]
        out = {"x": np.zeros(lp.n), "y": np.zeros(lp.m), "rc": np.zeros(lp.n),
               "act": np.zeros(lp.m), "vstat": np.zeros(lp.n, np.int8),
               "cstat": np.zeros(lp.m, np.int8)}
        r = abi.MiLpResult()
        flag = None if interrupt is None else _p(interrupt)
        self._push_params()
        rc = self._L.mi_lp_solver_solve(
            self.h, ctypes.byref(sp), lp.m, lp.n, *[_p(a) for a in keep], lp.obj_offset,
            lp.obj_scale, int(lp.maximize), flag, ctypes.byref(r),
            *[_p(out[k]) for k in ("x", "y", "rc", "act", "vstat", "cstat")])
        self._check(rc, "mi_lp_solver_solve")
        self.lp = None  # the handle now holds the scaled LP
        return r, out

    def set_variable_bounds(self, col_lb, col_ub):
        lb = np.ascontiguousarray(col_lb, dtype=np.float64)
        ub = np.ascontiguousarray(col_ub, dtype=np.float64)
        self._check(self._L.mi_lp_set_variable_bounds(self.h, _p(lb), _p(ub)),
                    "mi_lp_set_variable_bounds")

    def load_basis_state(self, state):
        st = np.ascontiguousarray(state, dtype=np.int8)
        self._check(self._L.mi_lp_load_basis_state(self.h, _p(st), len(st)),
                    "mi_lp_load_basis_state")

    def clear_basis_state(self):
        self._L.mi_lp_clear_basis_state(self.h)

    def notify_matrix_unchanged(self):
        self._L.mi_lp_notify_matrix_unchanged(self.h)

    def _push_params(self):
        self._check(self._L.mi_lp_set_params(self.h, ctypes.byref(self.params)),
                    "mi_lp_set_params")

    def solve(self):
        self._push_params()
        r = abi.MiLpResult()
        self._L.mi_lp_solve(self.h, None, ctypes.byref(r))
        if r.error_code == 100:
            raise EngineUnavailable(self._L.mi_lp_last_error(self.h).decode())
        return r

    # benchmark slicing
    def begin(self, pause_at):
        self._push_params()
        self._check(self._L.mi_lp_begin(self.h, int(pause_at)), "mi_lp_begin")

    def run_until(self, pause_at):
        fin = ctypes.c_int32()
        it = ctypes.c_int64()
        self._check(self._L.mi_lp_run_until(self.h, int(pause_at), ctypes.byref(fin),
                                            ctypes.byref(it)), "mi_lp_run_until")
        return bool(fin.value), int(it.value)

    def stop(self):
        self._check(self._L.mi_lp_stop(self.h), "mi_lp_stop")

    def finish(self):
        r = abi.MiLpResult()
        self._L.mi_lp_finish(self.h, ctypes.byref(r))
        return r

    def kernel_stats(self):
        s = abi.MiLpKernelStats()
        self._L.mi_lp_get_kernel_stats(self.h, ctypes.byref(s))
        return {name: dict(launches=s.launches[i], bytes=s.algorithmic_bytes[i],
                           device_ms=s.device_ms[i], call_ms=s.call_ms[i])
                for i, name in enumerate(abi.KERNEL_NAMES)}

    def set_exchange(self, rank, world, allgather):
        """Cross-process column split (mi_lp_set_exchange): `allgather(data:
        bytes, sizes: list[int]) -> bytes` returns every rank's bytes in rank
        order. Call before load()."""
        self._exchange_cb = allgather_callback(world, allgather)  # kept alive with the handle
        self._check(self._L.mi_lp_set_exchange(self.h, int(rank), int(world), None,
                                               self._exchange_cb), "mi_lp_set_exchange")

    def set_exchange_native(self, rank, world, exchange):
        """Cross-process split with a C++ exchange (ShmExchange): the engine
        calls mi_exchange_allgather directly. Call before load()."""
        ctx, fn = exchange.function()
        self._exchange_keep = (exchange, fn)
        self._check(self._L.mi_lp_set_exchange(self.h, int(rank), int(world), ctx, fn),
                    "mi_lp_set_exchange")

    def record_iteration_times(self, on=True):
        self._check(self._L.mi_lp_record_iteration_times(self.h, int(on)),
                    "mi_lp_record_iteration_times")

    def iteration_times(self):
        """Seconds since Solve() started at the end of every iteration."""
        n = self._L.mi_lp_get_iteration_times(self.h, None, 0)
        if n < 0:
            raise RuntimeError(f"mi_lp_get_iteration_times failed ({-n})")
        out = np.zeros(n)
        self._L.mi_lp_get_iteration_times(self.h, _p(out), n)
        return out

    def run_counters(self):
        c = abi.MiLpRunCounters()
        self._check(self._L.mi_lp_get_run_counters(self.h, ctypes.byref(c)),
                    "mi_lp_get_run_counters")
        return {"factorizations": int(c.factorizations),
                "factorization_seconds": float(c.factorization_seconds),
                "iterations": int(c.iterations), "u_levels": int(c.u_levels),
                "u_outputs": int(c.u_outputs), "u_entries": int(c.u_entries),
                "sdual_segments": int(c.sdual_segments),
                "sdual_iterations": int(c.sdual_iterations)}

    def reset_kernel_stats(self):
        self._L.mi_lp_reset_kernel_stats(self.h)

    def set_kernel_timing(self, on=True, kernels=None):
        """HIP-event timing of the kernel ids in `kernels` (names of
        abi.KERNEL_NAMES; None: all) while on."""
        if kernels is None:
            self._L.mi_lp_set_kernel_timing(self.h, int(on))
            return
        mask = 0
        for k in kernels:
            mask |= 1 << abi.KERNEL_NAMES.index(k)
        self._L.mi_lp_set_kernel_timing_ids(self.h, mask if on else 0)

    def _get(self, fn, n, dtype):
        out = np.zeros(n, dtype=dtype)
        self._check(getattr(self._L, fn)(self.h, _p(out)), fn)
        return out

    def primal(self):
        return self._get("mi_lp_get_primal", self.lp.n, np.float64)

    def reduced_costs(self):
        return self._get("mi_lp_get_reduced_costs", self.lp.n, np.float64)

    def duals(self):
        return self._get("mi_lp_get_duals", self.lp.m, np.float64)

    def activities(self):
        return self._get("mi_lp_get_activities", self.lp.m, np.float64)

    def basis(self):
        return self._get("mi_lp_get_basis", self.lp.m, np.int32)

    def state(self):
        return self._get("mi_lp_get_state", self.lp.n + self.lp.m, np.int8)

    def statuses(self):
        var = np.zeros(self.lp.n, np.int8)
        cons = np.zeros(self.lp.m, np.int8)
        self._check(self._L.mi_lp_get_statuses(self.h, _p(var), _p(cons)),
                    "mi_lp_get_statuses")
        return var, cons

    def primal_ray(self):
        return self._get("mi_lp_get_primal_ray", self.lp.n + self.lp.m, np.float64)

    def dual_ray(self):
        return self._get("mi_lp_get_dual_ray", self.lp.m, np.float64)

    def _call(self, name, *args):
        self._check(getattr(self._L, "mi_lp_" + name)(self.h, *args), "mi_lp_" + name)

    # --- CP-SAT boundary (include/mi_lp.h) ---------------------------------
    def notify_matrix_changed(self):
        self._call("notify_matrix_changed")

    def set_starting_variable_values(self, values):
        self._start_values = np.ascontiguousarray(values, dtype=np.float64)
        self._call("set_starting_variable_values", _p(self._start_values),
                   len(self._start_values))

    def set_integrality_scale(self, col, scale):
        self._call("set_integrality_scale", int(col), ctypes.c_double(scale))

    def clear_integrality_scales(self):
        self._call("clear_integrality_scales")

    def objective_limit_reached(self):
        r = ctypes.c_int32()
        self._call("objective_limit_reached", ctypes.byref(r))
        return bool(r.value)

    def unit_row_left_inverse(self, row):
        """(dense values[m], non-zero rows) of e_row^T B^-1."""
        vals = np.zeros(self.lp.m, np.float64)
        nz = np.zeros(self.lp.m, np.int32)
        cnt = ctypes.c_int32()
        self._call("get_unit_row_left_inverse", int(row), _p(vals), _p(nz), ctypes.byref(cnt))
        return vals, nz[:cnt.value].copy()

    def dictionary(self, column_scales=None):
        """B^-1 A as (row_starts[m+1], cols, values), rows in basis order."""
        nnz = ctypes.c_int64()
        if column_scales is None:
            self._call("compute_dictionary", None, 0, ctypes.byref(nnz))
        else:
            sc = np.ascontiguousarray(column_scales, dtype=np.float64)
            self._call("compute_dictionary", _p(sc), len(sc), ctypes.byref(nnz))
        starts = np.zeros(self.lp.m + 1, np.int64)
        cols = np.zeros(max(1, nnz.value), np.int32)
        vals = np.zeros(max(1, nnz.value), np.float64)
        self._call("get_dictionary", _p(starts), _p(cols), _p(vals))
        return starts, cols[:nnz.value], vals[:nnz.value]

    def row_combinations(self, Y):
        """Y: (k, m), or (m,) for k = 1. Returns the (k, n+m) array of
        Y[j] . a_col for every column of [A | I] (ColumnScalarProduct's order),
        computed on the GPU with A read once per 16 vectors."""
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        if Y.ndim == 1:
            Y = Y[None, :]
        if Y.ndim != 2 or Y.shape[1] != self.lp.m:
            raise ValueError(f"Y must be (k, {self.lp.m}), got {Y.shape}")
        k = Y.shape[0]
        if k == 0:  # still a call (its state checks), with non-empty buffers behind it
            Y = np.zeros((1, self.lp.m), np.float64)
        out = np.zeros((max(k, 1), self.lp.n + self.lp.m), np.float64)
        self._call("row_combinations", _p(Y), k, _p(out))
        return out[:k]

    def tableau_rows(self, rows, with_left_inverses=False):
        """Rows `rows` of B^-1 [A | I] as a (k, n+m) array: row j is
        unit_row_left_inverse(rows[j]) times every column. With
        with_left_inverses also returns those (k, m) left inverses."""
        rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        k = len(rows)
        if k == 0:  # still a call (its state checks), with non-empty buffers behind it
            rows = np.zeros(1, np.int32)
        out = np.zeros((max(k, 1), self.lp.n + self.lp.m), np.float64)
        left = np.zeros((max(k, 1), self.lp.m), np.float64) if with_left_inverses else None
        self._call("get_tableau_rows", _p(rows), k, _p(out),
                   None if left is None else _p(left))
        return (out[:k], left[:k]) if with_left_inverses else out[:k]

    def _sparse_rows(self, starts, k):
        """The stored result of the last sparse call as (row_starts, cols, vals)."""
        kept = int(starts[k])
        cols = np.zeros(max(1, kept), np.int32)
        vals = np.zeros(max(1, kept), np.float64)
        self._call("get_sparse_rows", _p(cols), _p(vals))
        return starts[:k + 1], cols[:kept], vals[:kept]

    def row_combinations_sparse(self, Y, drop_tolerance=0.0, columns="all"):
        """row_combinations(Y) as sparse rows, filtered and packed on the GPU:
        (row_starts[k+1] int64, cols int32, vals float64). Row j keeps, columns
        ascending, the columns selected by `columns` ("all", "structural",
        "non_basic", "structural_non_basic") with |value| > drop_tolerance."""
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        if Y.ndim == 1:
            Y = Y[None, :]
        if Y.ndim != 2 or Y.shape[1] != self.lp.m:
            raise ValueError(f"Y must be (k, {self.lp.m}), got {Y.shape}")
        k = Y.shape[0]
        if k == 0:  # still a call (its state checks), with non-empty buffers behind it
            Y = np.zeros((1, self.lp.m), np.float64)
        starts = np.zeros(max(k, 1) + 1, np.int64)
        self._call("row_combinations_sparse", _p(Y), k, ctypes.c_double(drop_tolerance),
                   abi.COLUMN_FILTERS[columns], _p(starts))
        return self._sparse_rows(starts, k)

    def tableau_rows_sparse(self, rows, drop_tolerance=0.0, columns="all",
                            with_left_inverses=False):
        """tableau_rows(rows) as sparse rows (see row_combinations_sparse). With
        with_left_inverses also returns the (k, m) left inverses, last."""
        rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        k = len(rows)
        if k == 0:  # still a call (its state checks), with non-empty buffers behind it
            rows = np.zeros(1, np.int32)
        starts = np.zeros(max(k, 1) + 1, np.int64)
        left = np.zeros((max(k, 1), self.lp.m), np.float64) if with_left_inverses else None
        self._call("get_tableau_rows_sparse", _p(rows), k, ctypes.c_double(drop_tolerance),
                   abi.COLUMN_FILTERS[columns], _p(starts),
                   None if left is None else _p(left))
        out = self._sparse_rows(starts, k)
        return out + (left[:k],) if with_left_inverses else out

    def row_penalties(self, Y, d, status, down_dist, up_dist, unit=None, pivot_tolerance=0.0):
        """One branching penalty record (BRANCH_PENALTY: down, up, down_col,
        up_col, down_count, up_count) per row of row_combinations(Y), reduced
        on the GPU (include/mi_lp.h mi_lp_row_penalties has the rule). d,
        status and unit cover the n+m columns, the distances the k vectors;
        unit None means all 0."""
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        if Y.ndim == 1:
            Y = Y[None, :]
        total = self.lp.n + self.lp.m
        if Y.ndim != 2 or Y.shape[1] != self.lp.m:
            raise ValueError(f"Y must be (k, {self.lp.m}), got {Y.shape}")
        k = Y.shape[0]
        d = np.ascontiguousarray(d, dtype=np.float64)
        status = np.ascontiguousarray(status, dtype=np.int8)
        down = np.ascontiguousarray(down_dist, dtype=np.float64).reshape(-1)
        up = np.ascontiguousarray(up_dist, dtype=np.float64).reshape(-1)
        if unit is not None:
            unit = np.ascontiguousarray(unit, dtype=np.float64)
        if d.shape != (total,) or status.shape != (total,) or \
                (unit is not None and unit.shape != (total,)):
            raise ValueError(f"d, status and unit must have {total} entries")
        if len(down) != k or len(up) != k:
            raise ValueError(f"the distances must have {k} entries")
        if k == 0:  # still a call (its state checks), with non-empty buffers behind it
            Y = np.zeros((1, self.lp.m), np.float64)
            down = up = np.zeros(1, np.float64)
        out = np.zeros(max(k, 1), BRANCH_PENALTY)
        self._call("row_penalties", _p(Y), k, _p(d), _p(status),
                   None if unit is None else _p(unit), _p(down), _p(up),
                   ctypes.c_double(pivot_tolerance), _p(out))
        return out[:k]

    def branching_penalties(self, cols, down_dist=None, up_dist=None, unit=None,
                            pivot_tolerance=0.0, with_left_inverses=False):
        """The records of the k BASIC columns `cols` of the current basis
        (include/mi_lp.h mi_lp_branching_penalties): tableau rows, statuses and
        reduced costs are the solver's. Distances None: the fractional parts of
        the columns' values. unit: n entries, or None. With with_left_inverses
        also returns the (k, m) left inverses."""
        cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        k = len(cols)
        dists = []
        for dist in (down_dist, up_dist):
            if dist is not None:
                dist = np.ascontiguousarray(dist, dtype=np.float64).reshape(-1)
                if len(dist) != k:
                    raise ValueError(f"the distances must have {k} entries")
                if k == 0:
                    dist = np.zeros(1, np.float64)
            dists.append(dist)
        if unit is not None:
            unit = np.ascontiguousarray(unit, dtype=np.float64)
            if unit.shape != (self.lp.n,):
                raise ValueError(f"unit must have {self.lp.n} entries")
        if k == 0:  # still a call (its state checks), with non-empty buffers behind it
            cols = np.zeros(1, np.int32)
        out = np.zeros(max(k, 1), BRANCH_PENALTY)
        left = np.zeros((max(k, 1), self.lp.m), np.float64) if with_left_inverses else None
        self._call("branching_penalties", _p(cols), k,
                   None if dists[0] is None else _p(dists[0]),
                   None if dists[1] is None else _p(dists[1]),
                   None if unit is None else _p(unit), ctypes.c_double(pivot_tolerance),
                   _p(out), None if left is None else _p(left))
        return (out[:k], left[:k]) if with_left_inverses else out[:k]

    def get_cut_rows(self, kept):
        """The stored lists of the last cut call that built them, `kept`
        entries (its row_starts[k]): (cols int32, vals float64)."""
        cols = np.zeros(max(1, kept), np.int32)
        vals = np.zeros(max(1, kept), np.float64)
        self._call("get_cut_rows", _p(cols), _p(vals))
        return cols[:kept], vals[:kept]

    def _cuts(self, name, k, lists, head, tail=()):
        """The shared tail of the two cut calls: head are the C call's
        arguments before row_starts, tail those after summaries."""
        starts = np.zeros(max(k, 1) + 1, np.int64) if lists else None
        summaries = np.zeros(max(k, 1), CUT_SUMMARY)
        self._call(name, *head, None if starts is None else _p(starts), _p(summaries), *tail)
        if not lists:
            return None, None, None, summaries[:k]
        cols, vals = self.get_cut_rows(int(starts[k]))
        return starts[:k + 1], cols, vals, summaries[:k]

    def row_gomory_cuts(self, Y, status, f0, row_unit, unit=None, zero_tolerance=0.0,
                        drop_tolerance=0.0, lists=True):
        """One Gomory mixed-integer cut sum c_j x_j >= rhs over the structural
        columns per row of row_combinations(Y), built on the GPU (include/
        mi_lp.h mi_lp_row_gomory_cuts has the rule): (row_starts[k+1] int64,
        cols int32, vals float64, summaries). Cut j's kept columns, ascending,
        are cols[row_starts[j]:row_starts[j+1]] with the coefficients in vals;
        summaries is a structured array (CUT_SUMMARY: max_abs, min_abs, count,
        bad_count, max_col, min_col) of k entries. status and unit cover the
        n+m columns (unit None: all 0), f0 and row_unit the k vectors. rhs is
        1 + sum c_j x*_j at the node's LP point and is the caller's to form.
        With lists=False only the summaries come down and the first three are
        None."""
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        if Y.ndim == 1:
            Y = Y[None, :]
        total = self.lp.n + self.lp.m
        if Y.ndim != 2 or Y.shape[1] != self.lp.m:
            raise ValueError(f"Y must be (k, {self.lp.m}), got {Y.shape}")
        k = Y.shape[0]
        status = np.ascontiguousarray(status, dtype=np.int8)
        f0 = np.ascontiguousarray(f0, dtype=np.float64).reshape(-1)
        row_unit = np.ascontiguousarray(row_unit, dtype=np.float64).reshape(-1)
        if unit is not None:
            unit = np.ascontiguousarray(unit, dtype=np.float64)
        if status.shape != (total,) or (unit is not None and unit.shape != (total,)):
            raise ValueError(f"status and unit must have {total} entries")
        if len(f0) != k or len(row_unit) != k:
            raise ValueError(f"f0 and row_unit must have {k} entries")
        if k == 0:  # still a call (its state checks), with non-empty buffers behind it
            Y = np.zeros((1, self.lp.m), np.float64)
            f0 = row_unit = np.full(1, 0.5)
        return self._cuts("row_gomory_cuts", k, lists,
                          (_p(Y), k, _p(status), None if unit is None else _p(unit), _p(f0),
                           _p(row_unit), ctypes.c_double(zero_tolerance),
                           ctypes.c_double(drop_tolerance)))

    def gomory_cuts(self, cols, unit, zero_tolerance=0.0, drop_tolerance=0.0, lists=True,
                    with_left_inverses=False):
        """The cuts of the k BASIC structural columns `cols` of the current
        basis (include/mi_lp.h mi_lp_gomory_cuts): tableau rows, statuses and
        fractional parts are the solver's; unit: n entries, the integer steps
        in LP units (0: continuous), positive on every column of cols. Returns
        what row_gomory_cuts returns; with with_left_inverses also the (k, m)
        left inverses, last."""
        cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        k = len(cols)
        unit = np.ascontiguousarray(unit, dtype=np.float64)
        if unit.shape != (self.lp.n,):
            raise ValueError(f"unit must have {self.lp.n} entries")
        if k == 0:  # still a call (its state checks), with non-empty buffers behind it
            cols = np.zeros(1, np.int32)
        if self.lp.n == 0:
            unit = np.zeros(1, np.float64)
        left = np.zeros((max(k, 1), self.lp.m), np.float64) if with_left_inverses else None
        out = self._cuts("gomory_cuts", k, lists,
                         (_p(cols), k, _p(unit), ctypes.c_double(zero_tolerance),
                          ctypes.c_double(drop_tolerance)),
                         (None if left is None else _p(left),))
        return out + (left[:k],) if with_left_inverses else out

    def _points(self, X, what):
        """X as a contiguous (k, n+m) array: (k, n) gets zero slacks appended,
        a 1-D array is one point."""
        n, total = self.lp.n, self.lp.n + self.lp.m
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X[None, :]
        if X.ndim != 2 or X.shape[1] not in (n, total):
            raise ValueError(f"{what} must be (k, {total}) or (k, {n}), got {X.shape}")
        if X.shape[1] != total:
            X = np.concatenate([X, np.zeros((X.shape[0], total - X.shape[1]))], axis=1)
        return X

    def column_combinations(self, X):
        """X: (k, n+m), or (k, n) (zero slacks are appended), or 1-D for k = 1.
        Returns the (k, m) array of the row sums [A | I] X[j] (entries of a row
        in increasing column order, zero multipliers skipped), computed on the
        GPU with A read once per 16 points."""
        X = self._points(X, "X")
        k = X.shape[0]
        if k == 0:  # still a call (its state checks), with non-empty buffers behind it
            X = np.zeros((1, self.lp.n + self.lp.m), np.float64)
        out = np.zeros((max(k, 1), self.lp.m), np.float64)
        self._call("column_combinations", _p(X), k, _p(out))
        return out[:k]

    def _overrides(self, base, overrides):
        """(base (1, n+m), k, starts, cols, vals) of the override calls."""
        base = self._points(base, "base")
        if base.shape[0] != 1:
            raise ValueError("base must be one point")
        k = len(overrides)
        starts = np.zeros(k + 1, np.int64)
        cols, vals = [np.zeros(0, np.int32)], [np.zeros(0, np.float64)]
        for j, (c, v) in enumerate(overrides):
            c = np.ascontiguousarray(c, dtype=np.int32).reshape(-1)
            v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
            if len(c) != len(v):
                raise ValueError(f"overrides[{j}]: {len(c)} columns, {len(v)} values")
            cols.append(c)
            vals.append(v)
            starts[j + 1] = starts[j] + len(c)
        cols = np.ascontiguousarray(np.concatenate(cols))
        vals = np.ascontiguousarray(np.concatenate(vals))
        return base, k, starts, cols, vals

    def column_combinations_from(self, base, overrides):
        """column_combinations of the points base with X[j][cols] = vals for
        overrides[j] = (cols, vals), built on the GPU: only base (n or n+m
        values) and the override lists go up. No column twice within a point.
        Returns (k, m)."""
        base, k, starts, cols, vals = self._overrides(base, overrides)
        out = np.zeros((max(k, 1), self.lp.m), np.float64)
        self._call("column_combinations_from", _p(base), k, _p(starts),
                   _p(cols) if len(cols) else None, _p(vals) if len(vals) else None, _p(out))
        return out[:k]

    def _row_bounds(self, bounds, what):
        """None (the loaded bounds: NULL in the C call) or m contiguous doubles."""
        if bounds is None:
            return None
        bounds = np.ascontiguousarray(bounds, dtype=np.float64).reshape(-1)
        if len(bounds) != self.lp.m:
            raise ValueError(f"{what} must hold {self.lp.m} values, got {len(bounds)}")
        return bounds

    def _violations(self, name, k, lists, args, row_lb, row_ub, tolerance):
        """The shared tail of the two violations calls: args are the C call's
        leading arguments after the handle."""
        lb, ub = self._row_bounds(row_lb, "row_lb"), self._row_bounds(row_ub, "row_ub")
        starts = np.zeros(max(k, 1) + 1, np.int64) if lists else None
        summaries = np.zeros(max(k, 1), POINT_VIOLATIONS)
        self._call(name, *args, None if lb is None else _p(lb), None if ub is None else _p(ub),
                   ctypes.c_double(tolerance), None if starts is None else _p(starts),
                   _p(summaries))
        if not lists:
            return None, None, None, summaries[:k]
        kept = int(starts[k])
        rows = np.zeros(max(1, kept), np.int32)
        activities = np.zeros(max(1, kept), np.float64)
        self._call("get_violated_rows", _p(rows), _p(activities))
        return starts[:k + 1], rows[:kept], activities[:kept], summaries[:k]

    def column_violations(self, X, row_lb=None, row_ub=None, tolerance=0.0, lists=True):
        """column_combinations(X) filtered on the GPU: per point the rows whose
        activity a has not (a >= row_lb - tolerance) or not (a <= row_ub +
        tolerance), and a summary. X as in column_combinations; row_lb /
        row_ub: m values, None for the loaded bounds. Returns (row_starts[k+1]
        int64, rows int32, activities float64, summaries): point j's violated
        rows, ascending, are rows[row_starts[j]:row_starts[j+1]], and
        summaries is a structured array (POINT_VIOLATIONS: count, worst,
        worst_row, reserved) of k entries. With lists=False only the summaries
        come down and the first three are None."""
        X = self._points(X, "X")
        k = X.shape[0]
        if k == 0:  # still a call (its state checks), with non-empty buffers behind it
            X = np.zeros((1, self.lp.n + self.lp.m), np.float64)
        return self._violations("column_combinations_violations", k, lists, (_p(X), k),
                                row_lb, row_ub, tolerance)

    def column_violations_from(self, base, overrides, row_lb=None, row_ub=None, tolerance=0.0,
                               lists=True):
        """column_violations of the points of column_combinations_from(base,
        overrides), built on the GPU."""
        base, k, starts, cols, vals = self._overrides(base, overrides)
        return self._violations(
            "column_combinations_from_violations", k, lists,
            (_p(base), k, _p(starts), _p(cols) if len(cols) else None,
             _p(vals) if len(vals) else None), row_lb, row_ub, tolerance)

    def _bound_sets(self, lbs, ubs):
        """(lbs, ubs, k): two contiguous (k, n) arrays (1-D for k = 1)."""
        n = self.lp.n
        out = []
        for what, b in (("lbs", lbs), ("ubs", ubs)):
            b = np.ascontiguousarray(b, dtype=np.float64)
            if b.ndim == 1:
                b = b.reshape(1, -1)
            if b.ndim != 2 or b.shape[1] != n:
                raise ValueError(f"{what} must be (k, {n}), got {b.shape}")
            out.append(b)
        if out[0].shape != out[1].shape:
            raise ValueError(f"lbs is {out[0].shape}, ubs {out[1].shape}")
        k = out[0].shape[0]
        if k == 0:  # still a call (its state checks), with non-empty buffers behind it
            out = [np.zeros((1, max(n, 1)), np.float64)] * 2
        return out[0], out[1], k

    def _bound_overrides(self, base_lb, base_ub, overrides):
        """The leading arguments of the override calls after the handle, and k."""
        base_lb, base_ub, one = self._bound_sets(base_lb, base_ub)
        if one != 1:
            raise ValueError("base_lb / base_ub must be one bound set")
        k = len(overrides)
        starts = np.zeros(k + 1, np.int64)
        parts = [[np.zeros(0, np.int32)], [np.zeros(0, np.float64)], [np.zeros(0, np.float64)]]
        for j, (c, lo, hi) in enumerate(overrides):
            c = np.ascontiguousarray(c, dtype=np.int32).reshape(-1)
            lo = np.ascontiguousarray(lo, dtype=np.float64).reshape(-1)
            hi = np.ascontiguousarray(hi, dtype=np.float64).reshape(-1)
            if not len(c) == len(lo) == len(hi):
                raise ValueError(f"overrides[{j}]: {len(c)} columns, {len(lo)} and {len(hi)} bounds")
            for part, a in zip(parts, (c, lo, hi)):
                part.append(a)
            starts[j + 1] = starts[j] + len(c)
        cols, new_lbs, new_ubs = (np.ascontiguousarray(np.concatenate(p)) for p in parts)
        some = len(cols) > 0
        # The arrays are returned too: the pointers must outlive the call.
        keep = (base_lb, base_ub, starts, cols, new_lbs, new_ubs)
        args = (_p(base_lb), _p(base_ub), k, _p(starts), _p(cols) if some else None,
                _p(new_lbs) if some else None, _p(new_ubs) if some else None)
        return args, k, keep

    def _ranges(self, name, k, args):
        m = self.lp.m
        lo = np.zeros((max(k, 1), m), np.float64)
        hi = np.zeros((max(k, 1), m), np.float64)
        counts = np.zeros((max(k, 1), m, 2), np.int32)
        self._call(name, *args, _p(lo), _p(hi), _p(counts))
        return lo[:k], hi[:k], counts[:k, :, 0].copy(), counts[:k, :, 1].copy()

    def bound_activity_ranges(self, lbs, ubs):
        """The activity range of every row of A under each of k bound sets over
        the n structural columns (lbs, ubs: (k, n), as batch_solve_bounds takes
        them), computed on the GPU with A read once per 16 sets. Returns (lo,
        hi, lo_inf, hi_inf), each (k, m): the sums of the finite terms and the
        counts of infinite bounds on each side (include/mi_lp.h
        mi_lp_bound_activity_ranges has the rule). The minimum of row r under
        set j is -inf when lo_inf[j, r] > 0, else lo[j, r]."""
        lbs, ubs, k = self._bound_sets(lbs, ubs)
        return self._ranges("bound_activity_ranges", k, (_p(lbs), _p(ubs), k))

    def bound_activity_ranges_from(self, base_lb, base_ub, overrides):
        """bound_activity_ranges of the sets base with l[cols] = new_lbs,
        u[cols] = new_ubs for overrides[j] = (cols, new_lbs, new_ubs), built on
        the GPU: only the base bounds and the override lists go up. No column
        twice within a set."""
        args, k, _keep = self._bound_overrides(base_lb, base_ub, overrides)
        return self._ranges("bound_activity_ranges_from", k, args)

    def _infeasible(self, name, k, lists, args, row_lb, row_ub, tolerance):
        lb, ub = self._row_bounds(row_lb, "row_lb"), self._row_bounds(row_ub, "row_ub")
        starts = np.zeros(max(k, 1) + 1, np.int64) if lists else None
        summaries = np.zeros(max(k, 1), POINT_VIOLATIONS)
        self._call(name, *args, None if lb is None else _p(lb), None if ub is None else _p(ub),
                   ctypes.c_double(tolerance), None if starts is None else _p(starts),
                   _p(summaries))
        if not lists:
            return None, None, None, summaries[:k]
        kept = int(starts[k])
        rows = np.zeros(max(1, kept), np.int32)
        amounts = np.zeros(max(1, kept), np.float64)
        self._call("get_infeasible_rows", _p(rows), _p(amounts))
        return starts[:k + 1], rows[:kept], amounts[:kept], summaries[:k]

    def infeasible_rows(self, lbs, ubs, row_lb=None, row_ub=None, tolerance=0.0, lists=True):
        """The rows that prove a bound set infeasible, filtered on the GPU: row
        r proves set j when its activity range misses [row_lb[r], row_ub[r]]
        by more than tolerance (g > tolerance, include/mi_lp.h). Conservative:
        a NaN bound or an overflowed sum only ever gives "not proven". Returns
        (row_starts, rows, amounts, summaries) shaped like column_violations;
        with lists=False only the summaries come down."""
        lbs, ubs, k = self._bound_sets(lbs, ubs)
        return self._infeasible("bound_infeasible_rows", k, lists, (_p(lbs), _p(ubs), k), row_lb,
                                row_ub, tolerance)

    def infeasible_rows_from(self, base_lb, base_ub, overrides, row_lb=None, row_ub=None,
                             tolerance=0.0, lists=True):
        """infeasible_rows of the sets of bound_activity_ranges_from(base_lb,
        base_ub, overrides): the children of a node (cpsat.branch_overrides)."""
        args, k, _keep = self._bound_overrides(base_lb, base_ub, overrides)
        return self._infeasible("bound_infeasible_rows_from", k, lists, args, row_lb, row_ub,
                                tolerance)

    def _implied(self, name, k, args, row_lb, row_ub):
        lb, ub = self._row_bounds(row_lb, "row_lb"), self._row_bounds(row_ub, "row_ub")
        n = self.lp.n
        new_lbs = np.zeros((max(k, 1), max(n, 1)), np.float64)
        new_ubs = np.zeros((max(k, 1), max(n, 1)), np.float64)
        self._call(name, *args, None if lb is None else _p(lb), None if ub is None else _p(ub),
                   _p(new_lbs), _p(new_ubs))
        return new_lbs[:k, :n], new_ubs[:k, :n]

    def implied_bounds(self, lbs, ubs, row_lb=None, row_ub=None):
        """One round of bound propagation on the GPU: the implied bounds of
        every structural column under each of k bound sets (lbs, ubs: (k, n)),
        from the activity ranges of bound_activity_ranges and the row bounds
        (None: the loaded ones). Returns (new_lbs, new_ubs), each (k, n), with
        new_lbs >= lbs and new_ubs <= ubs. The rule (include/mi_lp.h
        mi_lp_bound_implied_bounds) is the textbook one in doubles and is not
        outward-rounded."""
        lbs, ubs, k = self._bound_sets(lbs, ubs)
        return self._implied("bound_implied_bounds", k, (_p(lbs), _p(ubs), k), row_lb, row_ub)

    def implied_bounds_from(self, base_lb, base_ub, overrides, row_lb=None, row_ub=None):
        """implied_bounds of the sets of bound_activity_ranges_from(base_lb,
        base_ub, overrides), built on the GPU."""
        args, k, _keep = self._bound_overrides(base_lb, base_ub, overrides)
        return self._implied("bound_implied_bounds_from", k, args, row_lb, row_ub)

    def _tightened(self, name, k, lists, args, row_lb, row_ub, tolerance):
        lb, ub = self._row_bounds(row_lb, "row_lb"), self._row_bounds(row_ub, "row_ub")
        starts = np.zeros(max(k, 1) + 1, np.int64) if lists else None
        summaries = np.zeros(max(k, 1), POINT_VIOLATIONS)
        self._call(name, *args, None if lb is None else _p(lb), None if ub is None else _p(ub),
                   ctypes.c_double(tolerance), None if starts is None else _p(starts),
                   _p(summaries))
        if not lists:
            return None, None, None, None, summaries[:k]
        kept = int(starts[k])
        cols = np.zeros(max(1, kept), np.int32)
        new_lbs = np.zeros(max(1, kept), np.float64)
        new_ubs = np.zeros(max(1, kept), np.float64)
        self._call("get_tightened_columns", _p(cols), _p(new_lbs), _p(new_ubs))
        return starts[:k + 1], cols[:kept], new_lbs[:kept], new_ubs[:kept], summaries[:k]

    def tightened_columns(self, lbs, ubs, row_lb=None, row_ub=None, tolerance=0.0, lists=True):
        """implied_bounds filtered on the GPU: per set the columns whose bound
        moved by more than tolerance or whose implied bounds cross by more
        than it. Returns (col_starts[k+1] int64, cols int32, new_lbs, new_ubs,
        summaries): set j's kept columns, ascending, are
        cols[col_starts[j]:col_starts[j+1]] with their implied bounds beside
        them; summaries (POINT_VIOLATIONS) hold the number of kept columns,
        the largest crossing amount and the lowest column attaining it
        (worst_row, -1 without a crossing column). A set is proven infeasible
        by propagation iff worst_row >= 0. With lists=False only the summaries
        come down and the first four are None."""
        lbs, ubs, k = self._bound_sets(lbs, ubs)
        return self._tightened("bound_tightened_columns", k, lists, (_p(lbs), _p(ubs), k), row_lb,
                               row_ub, tolerance)

    def tightened_columns_from(self, base_lb, base_ub, overrides, row_lb=None, row_ub=None,
                               tolerance=0.0, lists=True):
        """tightened_columns of the sets base + overrides; a column whose own
        bounds differ in bits from the base is kept too, so a set's list is
        its complete override list relative to the base
        (cpsat.tightened_overrides turns the result into overrides)."""
        args, k, _keep = self._bound_overrides(base_lb, base_ub, overrides)
        return self._tightened("bound_tightened_columns_from", k, lists, args, row_lb, row_ub,
                               tolerance)

    def _propagate_args(self, max_rounds, is_integer, row_lb, row_ub, tolerance,
                        integrality_tolerance):
        """The arguments the three propagate calls share, between the sets and
        the outputs, and the arrays behind the pointers."""
        lb, ub = self._row_bounds(row_lb, "row_lb"), self._row_bounds(row_ub, "row_ub")
        if is_integer is not None:
            is_integer = np.ascontiguousarray(np.asarray(is_integer) != 0, dtype=np.uint8)
            if is_integer.shape != (self.lp.n,):
                raise ValueError(f"is_integer must hold {self.lp.n} values")
        keep = (is_integer, lb, ub)
        return (None if is_integer is None or self.lp.n == 0 else _p(is_integer),
                None if lb is None else _p(lb), None if ub is None else _p(ub),
                ctypes.c_double(tolerance), ctypes.c_double(integrality_tolerance),
                int(max_rounds)), keep

    def _propagate(self, name, k, args, common):
        n = self.lp.n
        new_lbs = np.zeros((max(k, 1), max(n, 1)), np.float64)
        new_ubs = np.zeros((max(k, 1), max(n, 1)), np.float64)
        summaries = np.zeros(max(k, 1), PROPAGATION)
        self._call(name, *args, *common, _p(new_lbs), _p(new_ubs), _p(summaries))
        return new_lbs[:k, :n], new_ubs[:k, :n], summaries[:k]

    def propagate_bounds(self, lbs, ubs, max_rounds, is_integer=None, row_lb=None, row_ub=None,
                         tolerance=0.0, integrality_tolerance=0.0):
        """Node propagation on the GPU: implied_bounds repeated per bound set
        (lbs, ubs: (k, n)) until no column moves by more than tolerance, a
        column crosses by more than it, or max_rounds; columns with a non-zero
        is_integer (n values, None: no integer column) are rounded inward
        within integrality_tolerance each round. Returns (new_lbs, new_ubs,
        summaries): the final bounds, each (k, n), and one PROPAGATION record
        per set (status PROPAGATE_ROUND_LIMIT / _FIXPOINT / _INFEASIBLE,
        rounds, moves, worst and worst_col of a crossing, kept = columns that
        differ in bits from the input). The rule is include/mi_lp.h
        mi_lp_bound_propagate; it is not outward-rounded."""
        lbs, ubs, k = self._bound_sets(lbs, ubs)
        common, _keep = self._propagate_args(max_rounds, is_integer, row_lb, row_ub, tolerance,
                                             integrality_tolerance)
        return self._propagate("bound_propagate", k, (_p(lbs), _p(ubs), k), common)

    def propagate_bounds_from(self, base_lb, base_ub, overrides, max_rounds, is_integer=None,
                              row_lb=None, row_ub=None, tolerance=0.0,
                              integrality_tolerance=0.0):
        """propagate_bounds of the sets base + overrides (as
        bound_activity_ranges_from takes them), built on the GPU."""
        args, k, _keep = self._bound_overrides(base_lb, base_ub, overrides)
        common, _keep2 = self._propagate_args(max_rounds, is_integer, row_lb, row_ub, tolerance,
                                              integrality_tolerance)
        return self._propagate("bound_propagate_from", k, args, common)

    def propagated_columns_from(self, base_lb, base_ub, overrides, max_rounds, is_integer=None,
                                row_lb=None, row_ub=None, tolerance=0.0,
                                integrality_tolerance=0.0, lists=True):
        """propagate_bounds_from filtered on the GPU: per set the columns whose
        final bounds differ in bits from the base, or that cross. Returns
        (col_starts[k+1] int64, cols int32, new_lbs, new_ubs, summaries); set
        j's list is its complete override list relative to the base
        (cpsat.tightened_overrides slices it) and summaries[j].kept its length.
        With lists=False only the summaries come down and the first four are
        None."""
        args, k, _keep = self._bound_overrides(base_lb, base_ub, overrides)
        common, _keep2 = self._propagate_args(max_rounds, is_integer, row_lb, row_ub, tolerance,
                                              integrality_tolerance)
        starts = np.zeros(max(k, 1) + 1, np.int64) if lists else None
        summaries = np.zeros(max(k, 1), PROPAGATION)
        self._call("bound_propagated_columns_from", *args, *common,
                   None if starts is None else _p(starts), _p(summaries))
        if not lists:
            return None, None, None, None, summaries[:k]
        kept = int(starts[k])
        cols = np.zeros(max(1, kept), np.int32)
        new_lbs = np.zeros(max(1, kept), np.float64)
        new_ubs = np.zeros(max(1, kept), np.float64)
        self._call("get_propagated_columns", _p(cols), _p(new_lbs), _p(new_ubs))
        return starts[:k + 1], cols[:kept], new_lbs[:kept], new_ubs[:kept], summaries[:k]


def batch_solve(handles, num_threads=4, progress=None, progress_s=15.0):
    """Solves already-loaded handles concurrently (mi_lp_batch_solve).

    progress: optional callable(done_indices, elapsed_s), called every
    progress_s seconds while the batch runs and once at the end with the
    indices whose results have landed (a finished solve writes its positive
    solve_seconds or an error code; the entry is zeroed when it starts)."""
    L = lib()
    for h in handles:
        h._push_params()
    arr = (ctypes.c_void_p * len(handles))(*[h.h.value for h in handles])
    res = (abi.MiLpResult * len(handles))()
    if progress is None:
        L.mi_lp_batch_solve(arr, len(handles), num_threads, res)
        return list(res)
    import threading
    import time
    t0 = time.perf_counter()
    th = threading.Thread(target=L.mi_lp_batch_solve,
                          args=(arr, len(handles), num_threads, res), daemon=True)
    th.start()
    while th.is_alive():
        th.join(progress_s)
        progress([i for i, r in enumerate(res) if r.solve_seconds > 0 or r.error_code != 0],
                 time.perf_counter() - t0)
    return list(res)


def batch_solve_gpus(handles, num_gpus, threads_per_gpu=4):
    """Loaded handles on devices [0, num_gpus) solved concurrently, one thread
    pool per device (mi_lp_batch_solve_gpus)."""
    L = lib()
    for h in handles:
        h._push_params()
    arr = (ctypes.c_void_p * len(handles))(*[h.h.value for h in handles])
    res = (abi.MiLpResult * len(handles))()
    rc = L.mi_lp_batch_solve_gpus(arr, len(handles), num_gpus, threads_per_gpu, res)
    if rc != 0:
        raise RuntimeError(f"mi_lp_batch_solve_gpus failed ({rc})")
    return list(res)


def batch_solve_bounds(workers, lbs, ubs, warm_state=None):
    """Children of one search node: LP i = the workers' loaded LP with
    variable bounds lbs[i], ubs[i], warm-started from warm_state
    (mi_lp_batch_solve_bounds). Returns the list of MiLpResult."""
    L = lib()
    for w in workers:
        w._push_params()
    if not workers:
        raise ValueError("batch_solve_bounds needs at least one worker")
    lp = workers[0].lp
    if lp is None or any(w.lp is None or (w.lp.m, w.lp.n) != (lp.m, lp.n) for w in workers):
        raise ValueError("every worker must have the same LP shape loaded")
    lbs = np.ascontiguousarray(lbs, dtype=np.float64)
    ubs = np.ascontiguousarray(ubs, dtype=np.float64)
    if lbs.ndim != 2 or lbs.shape[1] != lp.n:
        raise ValueError(f"lbs must be (count, {lp.n}), got {lbs.shape}")
    if ubs.shape != lbs.shape:
        raise ValueError(f"ubs shape {ubs.shape} != lbs shape {lbs.shape}")
    if warm_state is not None and len(warm_state) != lp.n + lp.m:
        raise ValueError(f"warm_state must have n+m={lp.n + lp.m} entries, "
                         f"got {len(warm_state)}")
    count = lbs.shape[0]
    arr = (ctypes.c_void_p * len(workers))(*[w.h.value for w in workers])
    res = (abi.MiLpResult * count)()
    ws = None if warm_state is None else np.ascontiguousarray(warm_state, dtype=np.int8)
    rc = L.mi_lp_batch_solve_bounds(arr, len(workers), count, _p(lbs), _p(ubs),
                                    None if ws is None else _p(ws),
                                    0 if ws is None else len(ws), res)
    if rc != 0:
        raise RuntimeError(f"mi_lp_batch_solve_bounds failed ({rc})")
    return list(res)


def scale_lp(lp, solver_params=None):
    """ScalingPreprocessor::Run (mi_lp_scale, host only): returns the scaled
    copy of `lp` plus row/column unscaling factors and the cost/bound divisors."""
    from . import lp as lpmod
    L = lib()
    sp = solver_params or abi.default_solver_params()
    cs = np.ascontiguousarray(lp.col_starts, np.int64)
    ri = np.ascontiguousarray(lp.row_idx, np.int32)
    arrs = [np.array(a, np.float64) for a in (lp.vals, lp.col_lb, lp.col_ub, lp.row_lb,
                                              lp.row_ub, lp.obj)]
    off = ctypes.c_double(lp.obj_offset)
    sc = ctypes.c_double(lp.obj_scale)
    rs = np.zeros(lp.m)
    cl = np.zeros(lp.n)
    cf = ctypes.c_double()
    bf = ctypes.c_double()
    rc = L.mi_lp_scale(ctypes.byref(sp), lp.m, lp.n, _p(cs), _p(ri), *[_p(a) for a in arrs],
                       ctypes.byref(off), ctypes.byref(sc), _p(rs), _p(cl), ctypes.byref(cf),
                       ctypes.byref(bf))
    if rc != 0:
        raise ValueError(f"mi_lp_scale failed with {rc}")
    v, clb, cub, rlb, rub, ob = arrs
    out = lpmod.LinearProgram(lp.m, lp.n, cs, ri, v, clb, cub, rlb, rub, ob, off.value,
                              sc.value, lp.maximize, lp.name)
    return out, {"row_scale": rs, "col_scale": cl, "cost_factor": cf.value,
                 "bound_factor": bf.value}


def _lp_arrays(lp):
    return [np.ascontiguousarray(x, dtype=t) for x, t in (
        (lp.col_starts, np.int64), (lp.row_idx, np.int32), (lp.vals, np.float64),
        (lp.col_lb, np.float64), (lp.col_ub, np.float64), (lp.row_lb, np.float64),
        (lp.row_ub, np.float64), (lp.obj, np.float64))]


class Presolve:
    """Glop's MainLpPreprocessor passes and their postsolve (mi_presolve_*,
    host only): run(lp) -> Glop's status after presolve; presolved() -> the
    reduced LinearProgram; recover(...) -> the solution of the original LP."""

    def __init__(self, solver_params=None):
        self._L = lib()
        self.sp = solver_params or abi.default_solver_params(use_preprocessing=1)
        self.h = ctypes.c_void_p(self._L.mi_presolve_create())
        if not self.h:
            raise MemoryError("mi_presolve_create")

    def __del__(self):
        if getattr(self, "h", None):
            self._L.mi_presolve_destroy(self.h)
            self.h = None

    def run(self, lp):
        self.lp = lp
        keep = _lp_arrays(lp)
        st = ctypes.c_int32()
        rc = self._L.mi_presolve_run(self.h, ctypes.byref(self.sp), lp.m, lp.n,
                                     *[_p(a) for a in keep], lp.obj_offset, lp.obj_scale,
                                     int(lp.maximize), ctypes.byref(st))
        if rc != 0:
            raise RuntimeError(f"mi_presolve_run failed ({rc})")
        return st.value

    def passes(self):
        return [self._L.mi_presolve_pass_name(self.h, i).decode()
                for i in range(self._L.mi_presolve_num_passes(self.h))]

    def presolved(self):
        from . import lp as lpmod
        m, n, mx = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        nnz = ctypes.c_int64()
        self._L.mi_presolve_dims(self.h, ctypes.byref(m), ctypes.byref(n), ctypes.byref(nnz),
                                 ctypes.byref(mx))
        m, n, nnz = m.value, n.value, nnz.value
        cs = np.zeros(n + 1, np.int64)
        ri = np.zeros(nnz, np.int32)
        arrs = [np.zeros(k) for k in (nnz, n, n, m, m, n)]
        off, sc = ctypes.c_double(), ctypes.c_double()
        self._L.mi_presolve_get(self.h, _p(cs), _p(ri), *[_p(a) for a in arrs],
                                ctypes.byref(off), ctypes.byref(sc))
        v, clb, cub, rlb, rub, ob = arrs
        return lpmod.LinearProgram(m, n, cs, ri, v, clb, cub, rlb, rub, ob, off.value,
                                   sc.value, bool(mx.value), "presolved")

    def recover(self, status, primal, duals, vstat, cstat):
        p = np.ascontiguousarray(primal, np.float64)
        d = np.ascontiguousarray(duals, np.float64)
        vs = np.ascontiguousarray(vstat, np.int8)
        cst = np.ascontiguousarray(cstat, np.int8)
        n0, m0 = self.lp.n, self.lp.m
        out = {"x": np.zeros(n0), "y": np.zeros(m0), "vstat": np.zeros(n0, np.int8),
               "cstat": np.zeros(m0, np.int8)}
        st = ctypes.c_int32(status)
        rc = self._L.mi_presolve_recover(self.h, ctypes.byref(st), _p(p), _p(d), _p(vs), _p(cst),
                                         *[_p(out[k]) for k in ("x", "y", "vstat", "cstat")])
        if rc != 0:
            raise RuntimeError(f"mi_presolve_recover failed ({rc})")
        return st.value, out


def solve_lp_with(lp, simplex, solver_params=None):
    """mi_lp_solver_solve_with: Glop's LPSolver flow (presolve, scaling, the
    caller's simplex, postsolve, LoadAndVerifySolution) with `simplex(inner_lp)`
    returning (mi_lp_result, primal, duals, vstat, cstat) for the presolved,
    scaled LP. Returns (result, dict of the original LP's solution arrays)."""
    from . import lp as lpmod
    L = lib()
    sp = solver_params or abi.default_solver_params()
    keep = _lp_arrays(lp)
    errors = []

    def cb(user, m, n, cs, ri, v, clb, cub, rlb, rub, ob, off, sc, mx, out, x, y, vs, cst):
        try:
            nnz = ctypes.cast(cs, ctypes.POINTER(ctypes.c_int64))[n] if n >= 0 else 0

            def arr(ptr, k, t):
                if k == 0:
                    return np.zeros(0, t)
                c = {np.float64: ctypes.c_double, np.int64: ctypes.c_int64,
                     np.int32: ctypes.c_int32}[t]
                return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(c)), (k,)).copy()
            inner = lpmod.LinearProgram(
                m, n, arr(cs, n + 1, np.int64), arr(ri, nnz, np.int32), arr(v, nnz, np.float64),
                arr(clb, n, np.float64), arr(cub, n, np.float64), arr(rlb, m, np.float64),
                arr(rub, m, np.float64), arr(ob, n, np.float64), off, sc, bool(mx), "inner")
            r, px, dy, pvs, pcs = simplex(inner)
            ctypes.memmove(out, ctypes.byref(r), ctypes.sizeof(abi.MiLpResult))
            for ptr, a, t in ((x, px, np.float64), (y, dy, np.float64), (vs, pvs, np.int8),
                              (cst, pcs, np.int8)):
                a = np.ascontiguousarray(a, t)
                if a.size:
                    ctypes.memmove(ptr, a.ctypes.data, a.nbytes)
            return 0
        except Exception as exc:  # noqa: BLE001 (reported after the call)
            errors.append(exc)
            return 102

    fn = SIMPLEX_FN(cb)
    out = {"x": np.zeros(lp.n), "y": np.zeros(lp.m), "rc": np.zeros(lp.n),
           "act": np.zeros(lp.m), "vstat": np.zeros(lp.n, np.int8),
           "cstat": np.zeros(lp.m, np.int8)}
    r = abi.MiLpResult()
    rc = L.mi_lp_solver_solve_with(fn, None, ctypes.byref(sp), lp.m, lp.n,
                                   *[_p(a) for a in keep], lp.obj_offset, lp.obj_scale,
                                   int(lp.maximize), ctypes.byref(r),
                                   *[_p(out[k]) for k in ("x", "y", "rc", "act", "vstat",
                                                          "cstat")])
    if errors:
        raise errors[0]
    if rc != 0:
        raise RuntimeError(f"mi_lp_solver_solve_with failed ({rc})")
    return r, out
