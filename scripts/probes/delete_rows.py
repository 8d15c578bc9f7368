"""Row deletion: mi_lp_delete_rows against the reload route (DESIGN.md section
7, "Rows deleted from the resident matrix").

Two parts, on one LP in one process.

Probe level (include/mi_lp_devop.h, tests/devop_matrix_delete.py), the matrix
resident: three rounds of "append 16 rows, delete those 16", then three
deletes of 1 % of the rows each (random rows). Per delete: device_ms (the
mask's copy and the kernels, by events), the host clock around the call (host
compaction of the pair, the device part, the per-shape buffers re-made) and
bytes_up.

Handle level (include/mi_lp.h), both routes timed up to the first iteration
(mi_lp_begin with pause_at 0 returns there) for the same two deletions:
  (a) mi_lp_delete_rows, then begin;
  (b) mi_lp_load of the reduced LP and mi_lp_load_basis_state of the compacted
      state, then begin: the compare, the rebuild of [A | I] and its
      transpose, and the upload happen inside it.
The handles have solved before (one iteration is enough: the matrix is
resident and there is a state), the reduced LP of (b) is built outside the
timed part, and (a) is the bare C call. host_only_ms is the same call on a
handle that has loaded but not solved (path 0): the column shift, the row
bounds and the hash, the host share of (a).

Usage: python scripts/probes/delete_rows.py dense|sparse [--small] [--probe-only]
  dense   config 2's LP as bench.py generates it (10 000 x 50 000)
  sparse  config 5's LP (100 000 x 1 000 000, ~10 entries per column)
Prints one JSON line per measurement and a summary line.
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(R, "or-tools_amd"), os.path.join(R, "tests")]
import devop_matrix_delete as dmd  # noqa: E402
import lp_gen  # noqa: E402
from mi_glop import abi, engine  # noqa: E402

SEED = 20261015  # bench.py's default
K = 16
ROUNDS = 3
ROW_ENTRIES = 100  # structural entries of an appended row


def log(msg):
    print(f"[{time.perf_counter() - T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


def ms(t):
    return round(1e3 * (time.perf_counter() - t), 3)


T0 = time.perf_counter()
shape = sys.argv[1]
small = "--small" in sys.argv
probe_only = "--probe-only" in sys.argv
if shape == "dense":
    m, n = (1000, 3000) if small else (10000, 50000)
    lp = lp_gen.dense_box_lp(m, n, SEED)
else:
    m, n = (5000, 50000) if small else (100000, 1000000)
    lp = lp_gen.sparse_c5_lp(m, n, 10, SEED)
log(f"{lp.name}: generated, {len(lp.vals)} entries")
rng = np.random.default_rng(SEED + 2)
per_row = min(lp.n, ROW_ENTRIES)
cut_cols = np.concatenate([np.sort(rng.choice(lp.n, per_row, replace=False)) for _ in range(K)])
cuts = (np.arange(K + 1, dtype=np.int64) * per_row, cut_cols.astype(np.int32),
        rng.uniform(0.5, 2.0, K * per_row), np.full(K, -1e6), np.full(K, 1e6))
entries_per_row = np.bincount(lp.row_idx, minlength=lp.m)
summary = {"lp": lp.name, "m": lp.m, "n": lp.n, "entries": int(len(lp.vals)), "k": K}

# ---------------------------------------------------------------------------
# Probe level.
d = dmd.DeleteDevOp(lp.m, lp.n, lp.col_starts, lp.row_idx, lp.vals)
log("matrix on the device")
best = {}
for rnd in range(ROUNDS):
    d.append_rows(*cuts[:3])
    mask = np.arange(d.m) >= lp.m
    t = time.perf_counter()
    d.delete_rows(mask, K * per_row)
    rec = {"what": "probe_delete_16_of_16_appended", "round": rnd, "call_ms": ms(t)}
    rec.update(d.last_delete())
    print(json.dumps(rec), flush=True)
    for key in ("device_ms", "call_ms"):
        best[key] = min(best.get(key, 1e30), rec[key])
    best["bytes_up"] = rec["bytes_up"]
summary["probe_delete_16_of_16_appended"] = dict(best)
best = {}
rows_now = entries_per_row.copy()
for rnd in range(ROUNDS):
    mask = np.zeros(d.m, bool)
    mask[rng.choice(d.m, max(1, d.m // 100), replace=False)] = True
    t = time.perf_counter()
    d.delete_rows(mask, int(rows_now[mask].sum()))
    rec = {"what": "probe_delete_1_percent", "round": rnd, "call_ms": ms(t)}
    rec.update(d.last_delete())
    rows_now = rows_now[~mask]
    print(json.dumps(rec), flush=True)
    for key in ("device_ms", "call_ms"):
        best[key] = min(best.get(key, 1e30), rec[key])
    best["bytes_up"] = rec["bytes_up"]
summary["probe_delete_1_percent"] = dict(best)
d.close()
log("probe level done")

# ---------------------------------------------------------------------------
# Handle level.
_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731


def params():
    return abi.default_params(use_dual_simplex=1, max_number_of_iterations=1)


def solved_handle(ext):
    h = engine.LpHandle(params())
    h.load(ext)
    r = h.solve()
    return h, r


def to_first_iteration(h):
    t = time.perf_counter()
    h.begin(0)
    out = ms(t)
    h.stop()
    h.finish()
    return out


def raw_delete(h, mask):
    info = abi.MiLpDeleteInfo()
    bytes_ = np.ascontiguousarray(mask, dtype=np.uint8)
    t = time.perf_counter()
    rc = h._L.mi_lp_delete_rows(h.h, _p(bytes_), ctypes.byref(info))
    out = ms(t)
    assert rc == 0, h.last_error()
    return out, {"path": info.path, "rows": info.rows, "entries": info.entries,
                 "bytes_up": info.bytes_up}


def handle_level(what, ext, mask):
    reduced = ext.without_rows(mask)
    # (a) the call.
    a, ra = solved_handle(ext)
    state = np.asarray(a.state(), np.int8)
    kept_state = np.concatenate([state[:ext.n], state[ext.n:][~mask]])
    call_ms, info = raw_delete(a, mask)
    a.lp = reduced
    begin_ms = to_first_iteration(a)
    a.close()
    rec = {"what": what, "route": "a_delete_rows", "call_ms": call_ms, "begin_ms": begin_ms,
           "total_ms": round(call_ms + begin_ms, 3), "info": info,
           "first_solve_status": ra.problem_status}
    print(json.dumps(rec), flush=True)
    # (b) the reload route.
    b, _ = solved_handle(ext)
    t = time.perf_counter()
    b.load(reduced)
    b.load_basis_state(kept_state)
    load_ms = ms(t)
    begin_b = to_first_iteration(b)
    b.close()
    rec_b = {"what": what, "route": "b_reload", "call_ms": load_ms, "begin_ms": begin_b,
             "total_ms": round(load_ms + begin_b, 3)}
    print(json.dumps(rec_b), flush=True)
    # The host share of (a): the same call with no device matrix (path 0).
    c = engine.LpHandle(params())
    c.load(ext)
    host_ms, info0 = raw_delete(c, mask)
    c.close()
    assert info0["path"] == 0
    print(json.dumps({"what": what, "route": "a_host_only", "call_ms": host_ms}), flush=True)
    summary[what] = {"delete_rows_total_ms": rec["total_ms"], "delete_rows_call_ms": call_ms,
                     "reload_total_ms": rec_b["total_ms"], "reload_load_ms": load_ms,
                     "host_only_ms": host_ms, "path": info["path"],
                     "bytes_up": info["bytes_up"],
                     "reload_bytes_up": 24 * (int(reduced.col_starts[-1]) + reduced.m)}


if not probe_only:
    ext = lp.with_rows(*cuts)
    handle_level("handle_delete_16_of_16_appended", ext, np.arange(ext.m) >= lp.m)
    log("16 of 16 done")
    mask = np.zeros(lp.m, bool)
    mask[rng.choice(lp.m, max(1, lp.m // 100), replace=False)] = True
    handle_level("handle_delete_1_percent", lp, mask)
    log("1 percent done")
print(json.dumps(summary), flush=True)
