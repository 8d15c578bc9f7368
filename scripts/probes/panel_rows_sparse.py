"""Sparse tableau rows: the dense panel followed by the caller's numpy filter
against the panel filtered and packed on the device (DESIGN.md section 7,
"Sparse tableau rows").

Through the probe table (include/mi_lp_devop.h), on one matrix in one process,
k = 16 vectors, a random-half column mask, after a warm-up, three alternating
rounds of
  (a0) column_dots_panel, then keep = mask & (|out| > 0) and the per-row
       (columns, values) lists in numpy: what a caller does today,
  (a1) the same at the tolerance T that keeps about 1 % of all k x N entries
       (a quantile of (a0)'s dense output over the masked columns),
  (b)  column_dots_panel_sparse with the mask at tolerance 0,
  (c)  column_dots_panel_sparse with the mask at tolerance T.
Per group: device-event time of the kernels alone (take_kernel_ms), the host
clock around the device call and, for (a), around the numpy filter; kept and
bytes_down of the sparse calls. (b) and (c) are compared with the filter of
(a) in every bit, every round.

Usage: python scripts/probes/panel_rows_sparse.py dense|sparse [--small]
  dense   config 2's LP as bench.py generates it (10 000 x 50 000)
  sparse  config 5's LP (100 000 x 1 000 000, ~10 entries per column)
Prints one JSON line per round and a summary line.
"""
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(R, "or-tools_amd"), os.path.join(R, "tests")]
import devop_panel_sparse  # noqa: E402
import lp_gen  # noqa: E402

SEED = 20261015  # bench.py's default
K = 16
ROUNDS = 3
KEPT_SHARE = 0.01


def log(msg):
    print(f"[{time.perf_counter() - T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


T0 = time.perf_counter()
shape = sys.argv[1]
small = "--small" in sys.argv
if shape == "dense":
    m, n = (1000, 3000) if small else (10000, 50000)
    lp = lp_gen.dense_box_lp(m, n, SEED)
else:
    m, n = (5000, 50000) if small else (100000, 1000000)
    lp = lp_gen.sparse_c5_lp(m, n, 10, SEED)
log(f"{lp.name}: generated, {len(lp.vals)} entries")
d = devop_panel_sparse.SparsePanelDevOp(lp.m, lp.n, lp.col_starts, lp.row_idx, lp.vals)
N = lp.n + lp.m
log("matrix on the device")
rng = np.random.default_rng(SEED + 1)
Y = rng.standard_normal((K, lp.m))
mask = rng.random(N) < 0.5
# Reused result buffers, as a caller in a loop would keep them.
dense_out = np.zeros((K, N))
starts = np.zeros(K + 1, np.int64)
cols_buf = np.zeros(K * N, np.int32)
vals_buf = np.zeros(K * N)


def numpy_filter(out, tolerance):
    keep = mask[None, :] & (np.abs(out) > tolerance)
    row_starts = np.zeros(K + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=row_starts[1:])
    rows = [np.nonzero(keep[j])[0] for j in range(K)]
    cols = np.concatenate(rows).astype(np.int32)
    vals = np.concatenate([out[j][rows[j]] for j in range(K)])
    return row_starts, cols, vals


def run_dense(tolerance):
    d.take_kernel_ms()
    t = time.perf_counter()
    out = d.column_dots_panel(Y, out=dense_out)
    call = 1e3 * (time.perf_counter() - t)
    dev = sum(d.take_kernel_ms())
    t = time.perf_counter()
    res = numpy_filter(out, tolerance)
    filt = 1e3 * (time.perf_counter() - t)
    return res, {"kernel_ms": round(dev, 3), "call_host_ms": round(call, 3),
                 "filter_host_ms": round(filt, 3), "host_ms": round(call + filt, 3),
                 "kept": int(res[0][K]), "bytes_down": 8 * K * N}


def run_sparse(tolerance):
    d.take_kernel_ms()
    t = time.perf_counter()
    res = d.column_dots_panel_sparse(Y, tolerance, mask, row_starts=starts, cols=cols_buf,
                                     vals=vals_buf)
    call = 1e3 * (time.perf_counter() - t)
    dev = sum(d.take_kernel_ms())
    p = d.last_panel_sparse()
    return res, {"kernel_ms": round(dev, 3), "host_ms": round(call, 3), "kept": p["kept"],
                 "bytes_down": p["bytes_down"]}


def differ(got, want):
    return int(not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and
                    np.array_equal(got[2].view(np.uint64), want[2].view(np.uint64))))


d.take_kernel_ms()  # turns the event timing on
out = d.column_dots_panel(Y, out=dense_out)
T = float(np.quantile(np.abs(out[:, mask]), 1.0 - KEPT_SHARE * N / mask.sum()))
run_sparse(0.0)  # warm-up: buffers allocated, kernels loaded
run_sparse(T)
log(f"warm-up done; tolerance for {KEPT_SHARE:.0%} kept: {T!r}; last {d.last_panel_sparse()}")
groups = ("a0_dense_filter_tol0", "a1_dense_filter_1pct", "b_sparse_tol0", "c_sparse_1pct")
best = {g: {} for g in groups}
for rnd in range(ROUNDS):
    rec = {"round": rnd}
    a0, rec[groups[0]] = run_dense(0.0)
    a0 = tuple(x.copy() for x in a0)
    a1, rec[groups[1]] = run_dense(T)
    b, rec[groups[2]] = run_sparse(0.0)
    rec["differ_b"] = differ(b, a0)
    c, rec[groups[3]] = run_sparse(T)
    rec["differ_c"] = differ(c, a1)
    for g in groups:
        for key in ("kernel_ms", "host_ms"):
            best[g][key] = min(best[g].get(key, 1e30), rec[g][key])
        best[g]["kept"], best[g]["bytes_down"] = rec[g]["kept"], rec[g]["bytes_down"]
    print(json.dumps(rec), flush=True)
print(json.dumps({"lp": lp.name, "m": lp.m, "N": N, "k": K, "masked_columns": int(mask.sum()),
                  "tolerance_1pct": T, "geometry": devop_panel_sparse.geometry(),
                  "last_panel_sparse": d.last_panel_sparse(), "best": best}), flush=True)
d.close()
