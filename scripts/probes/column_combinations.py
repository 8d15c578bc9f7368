"""Row sums [A | I] x of 16 points against one matrix: one panel call against
sixteen one-point calls ("Column-combination panel").

Through the probe table (include/mi_lp_devop.h), on one matrix in one process,
after a warm-up, three alternating rounds of
  (a) one row_sums_panel call with k = 16,
  (b) sixteen row_sums_panel calls with k = 1,
  (c) sixteen row_sums calls (the existing one-vector kernel, sign 1, no skip;
      the baseline of every comparison),
  (d) one row_sums_panel_from call with k = 16: one base point, each point
      overriding 1 % of the columns.
Per group: the host clock around the calls, transfers included, and for (a),
(b) and (d) the device-event time of the kernels alone (take_kernel_ms; the
one-vector kernel is not behind the panel events, so (c) has host time only).
(a), (b) and (c) run on the points (d) materialises; the four results are
compared bit for bit.

Usage: python scripts/probes/column_combinations.py dense|sparse [--small]
  dense   config 2's LP as bench.py generates it (10 000 x 50 000; the CSR of
          [A | I] is 6 GB, past the 256 MiB Infinity Cache)
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
import devop_row_panel  # noqa: E402
import lp_gen  # noqa: E402

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
d = devop_row_panel.RowPanelDevOp(lp.m, lp.n, lp.col_starts, lp.row_idx, lp.vals)
N = lp.n + lp.m
nnz = int(len(lp.vals)) + lp.m
log("matrix on the device")
rng = np.random.default_rng(SEED + 1)
base = rng.standard_normal(N)
per_point = max(1, N // 100)
sets = [(rng.permutation(N)[:per_point].astype(np.int32), rng.standard_normal(per_point))
        for _ in range(K)]
starts = np.zeros(K + 1, np.int64)
np.cumsum([len(c) for c, _ in sets], out=starts[1:])
ov_cols = np.concatenate([c for c, _ in sets])
ov_vals = np.concatenate([v for _, v in sets])
X = np.tile(base, (K, 1))
for j, (c, v) in enumerate(sets):
    X[j, c] = v


def panel_bytes(k):
    """One pass: the CSR, 8 k gathered per entry, X written, the results."""
    return 12.0 * nnz + 8.0 * (lp.m + 1) + 8.0 * k * nnz + 8.0 * k * N + 8.0 * k * lp.m


def group(fn):
    d.take_kernel_ms()
    t = time.perf_counter()
    out = fn()
    host = 1e3 * (time.perf_counter() - t)
    panel_ms, _ = d.take_kernel_ms()
    return out, host, panel_ms


def run_a():
    return d.row_sums_panel(X)


def run_b():
    return np.concatenate([d.row_sums_panel(X[j:j + 1]) for j in range(K)])


def run_c():
    return np.stack([d.row_sums(X[j], False, 1.0) for j in range(K)])


def run_d():
    return d.row_sums_panel_from(base, starts, ov_cols, ov_vals)


GROUPS = (("a_panel16", run_a), ("b_16x_panel1", run_b), ("c_16x_row_sums", run_c),
          ("d_overrides16", run_d))
d.take_kernel_ms()  # turns the event timing on
for _, fn in GROUPS:  # warm-up: buffers allocated, kernels loaded
    fn()
log(f"warm-up done; last_row_panel {d.last_row_panel()}")
best_dev, best_host = {}, {}
for rnd in range(ROUNDS):
    rec = {"round": rnd}
    outs = {}
    for name, fn in GROUPS:
        outs[name], host, dev = group(fn)
        rec[name] = {"kernel_ms": round(dev, 3) if name != "c_16x_row_sums" else None,
                     "host_ms": round(host, 3)}
        best_dev[name] = min(best_dev.get(name, 1e30), dev)
        best_host[name] = min(best_host.get(name, 1e30), host)
    ref = outs["c_16x_row_sums"].view(np.uint64)
    for name in ("a_panel16", "b_16x_panel1", "d_overrides16"):
        rec["bits_differ_" + name[0]] = int(np.sum(outs[name].view(np.uint64) != ref))
    print(json.dumps(rec), flush=True)
del best_dev["c_16x_row_sums"]
a = best_dev["a_panel16"]
d.row_sums_panel_from(base, starts, ov_cols, ov_vals)
print(json.dumps({
    "lp": lp.name, "m": lp.m, "N": N, "entries": nnz, "overrides": int(starts[-1]),
    "last_row_panel_overrides": d.last_row_panel(),
    "dense_points_up_bytes": 8 * K * N,
    "best_kernel_ms": {k: round(v, 3) for k, v in best_dev.items()},
    "best_host_ms": {k: round(v, 3) for k, v in best_host.items()},
    "panel16_bytes": panel_bytes(K), "panel16_gbs": round(panel_bytes(K) / a / 1e6, 1),
    "kernel_speedup_a_over_b": round(best_dev["b_16x_panel1"] / a, 2),
    "host_speedup_a_over_c": round(best_host["c_16x_row_sums"] / best_host["a_panel16"], 2),
    "host_speedup_d_over_c": round(best_host["c_16x_row_sums"] / best_host["d_overrides16"], 2),
}), flush=True)
d.close()
