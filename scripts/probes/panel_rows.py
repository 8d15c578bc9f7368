"""Column dots of 16 vectors against one [A | I]: one panel call against
sixteen one-vector calls ("Tableau-row panel").

Through the probe table (include/mi_lp_devop.h), on one matrix in one process,
after a warm-up, three alternating rounds of
  (a) one column_dots_panel call with k = 16,
  (b) sixteen column_dots_panel calls with k = 1,
  (c) sixteen list_dots calls over all N columns (the existing one-vector
      kernel; it reads every column from the CSC arrays, 12 B per entry).
Per group: device-event time of the kernels alone (take_kernel_ms) and the
host clock around the calls, transfers included. The three results are
compared bit for bit.

Usage: python scripts/probes/panel_rows.py dense|sparse [--small]
  dense   config 2's LP as bench.py generates it (10 000 x 50 000, A = 4 GB,
          past the 256 MiB Infinity Cache)
  sparse  config 5's LP (100 000 x 1 000 000, ~10 entries per column, A about
          120 MB: it FITS the Infinity Cache, so the one-vector passes read
          it from cache too)
Prints one JSON line per round and a summary line.
"""
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(R, "or-tools_amd"), os.path.join(R, "tests")]
import devop_panel  # noqa: E402
import lp_gen  # noqa: E402

HBM_PEAK_GBS = 8000.0
SEED = 20261015  # bench.py's default
K = 16
ROUNDS = 3


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
d = devop_panel.PanelDevOp(lp.m, lp.n, lp.col_starts, lp.row_idx, lp.vals)
N = lp.n + lp.m
log("matrix on the device")
col_len = np.diff(lp.col_starts)
nd = int(np.sum(col_len == lp.m)) if shape == "dense" else 0  # the dense block (auto mode)
nnz_sparse = int(len(lp.vals)) + lp.m - nd * lp.m
rng = np.random.default_rng(SEED + 1)
Y = rng.standard_normal((K, lp.m))
cols = np.arange(N, dtype=np.int32)


def panel_bytes(k):
    return 12.0 * nnz_sparse + 8.0 * lp.m * nd + 8.0 * (N + 1) + 8.0 * k * lp.m + 8.0 * k * N


def group(fn):
    d.take_kernel_ms()
    t = time.perf_counter()
    out = fn()
    host = 1e3 * (time.perf_counter() - t)
    panel_ms, list_ms = d.take_kernel_ms()
    return out, host, panel_ms + list_ms


def run_a():
    return d.column_dots_panel(Y)


def run_b():
    return np.concatenate([d.column_dots_panel(Y[j:j + 1]) for j in range(K)])


def run_c():
    return np.stack([d.list_dots(cols, Y[j]) for j in range(K)])


d.take_kernel_ms()  # turns the event timing on
for fn in (run_a, run_b, run_c):  # warm-up: buffers allocated, kernels loaded
    fn()
log(f"warm-up done; last_panel {d.last_panel()}")
best = {}
for rnd in range(ROUNDS):
    rec = {"round": rnd}
    outs = {}
    for name, fn in (("a_panel16", run_a), ("b_16x_panel1", run_b), ("c_16x_list_dots", run_c)):
        outs[name], host, dev = group(fn)
        rec[name] = {"kernel_ms": round(dev, 3), "host_ms": round(host, 3)}
        best[name] = min(best.get(name, 1e30), dev)
    ref = outs["a_panel16"].view(np.uint64)
    rec["bits_differ_b"] = int(np.sum(outs["b_16x_panel1"].view(np.uint64) != ref))
    rec["bits_differ_c"] = int(np.sum(outs["c_16x_list_dots"].view(np.uint64) != ref))
    print(json.dumps(rec), flush=True)
a, b = best["a_panel16"], best["b_16x_panel1"]
print(json.dumps({
    "lp": lp.name, "m": lp.m, "N": N, "dense_columns": nd, "sparse_entries": nnz_sparse,
    "last_panel_k16": d.last_panel() if d.column_dots_panel(Y) is not None else None,
    "best_kernel_ms": {k: round(v, 3) for k, v in best.items()},
    "panel16_bytes": panel_bytes(K), "panel16_gbs": round(panel_bytes(K) / a / 1e6, 1),
    "panel1_x16_bytes": 16 * panel_bytes(1),
    "panel1_x16_gbs": round(16 * panel_bytes(1) / b / 1e6, 1),
    "hbm_peak_gbs": HBM_PEAK_GBS, "panel16_fraction_of_peak": round(panel_bytes(K) / a / 1e6 /
                                                                     HBM_PEAK_GBS, 3),
    "speedup_a_over_b": round(b / a, 2)}), flush=True)
d.close()
