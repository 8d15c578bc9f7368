"""Violated rows of 16 points against one matrix: the filter on the GPU against
the dense row sums and the numpy filter a caller writes today (DESIGN.md
section 7, "Column-combination violations").

Through the probe table (include/mi_lp_devop.h), on one matrix in one process,
after a warm-up, three alternating rounds with k = 16 of
  (a)  row_sums_panel, then the numpy filter and summaries (the baseline:
       code of the parent commit),
  (b)  row_violations_panel with lists,
  (c)  row_violations_panel, summaries only,
  (da) row_sums_panel_from, then the numpy filter and summaries,
  (db) row_violations_panel_from with lists,
  (dc) row_violations_panel_from, summaries only.
(a), (b) and (c) run on the points (d*) materialise: one base point, each point
overriding 1 % of the columns. The bounds are the same for every row: the
0.5 % and 99.5 % quantiles of the dense result, so that about 1 % of the k m
(row, point) pairs are violated; the achieved share is printed. Per group: the
host clock around the calls (for (a) and (da): call + filter), the device-event
time of the kernels (take_kernel_ms) and the bytes that came down. Every
round asserts that (b), (c), (db) and (dc) equal (a)'s filter in every bit.

Usage: python scripts/probes/column_violations.py dense|sparse [--small]
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
import devop_row_violations  # noqa: E402
import lp_gen  # noqa: E402

SEED = 20261015  # bench.py's default
K = 16
ROUNDS = 3
TOLERANCE = 1e-9
SUMMARY = devop_row_violations.SUMMARY


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
d = devop_row_violations.RowViolationsDevOp(lp.m, lp.n, lp.col_starts, lp.row_idx, lp.vals)
N = lp.n + lp.m
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
dense_out = np.zeros(K * lp.m)
low, high = np.quantile(d.row_sums_panel(X), [0.005, 0.995])
LB, UB = np.full(lp.m, low), np.full(lp.m, high)


def numpy_filter(acts):
    """What a caller writes today: the header's rule over the k x m result."""
    keep = ~(acts >= LB - TOLERANCE) | ~(acts <= UB + TOLERANCE)
    row_starts = np.zeros(K + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=row_starts[1:])
    point, row = np.nonzero(keep)
    vals = acts[point, row]
    amount = np.where(np.isnan(vals), np.inf, np.maximum(LB[row] - vals, vals - UB[row]))
    summaries = np.zeros(K, SUMMARY)
    summaries["count"] = np.diff(row_starts)
    summaries["worst_row"] = -1
    for j in range(K):
        s, e = row_starts[j], row_starts[j + 1]
        if e > s:
            at = s + np.argmax(amount[s:e])  # the first maximum: the lowest row
            summaries["worst"][j], summaries["worst_row"][j] = amount[at], row[at]
    return row_starts, row.astype(np.int32), vals, summaries


kept_capacity = int(numpy_filter(d.row_sums_panel(X))[0][K])
buffers = {"row_starts": np.zeros(K + 1, np.int64), "rows": np.zeros(kept_capacity, np.int32),
           "activities": np.zeros(kept_capacity), "summaries": np.zeros(K, SUMMARY)}


def run_a():
    return numpy_filter(d.row_sums_panel(X, out=dense_out)), 8 * K * lp.m


def run_da():
    return (numpy_filter(d.row_sums_panel_from(base, starts, ov_cols, ov_vals, out=dense_out)),
            8 * K * lp.m)


def violations(call, lists):
    def run():
        out = call(LB, UB, TOLERANCE, lists=lists, buffers=buffers)
        return out, d.last_row_violations()["bytes_down"]
    return run


def dense_form(*a, **kw):
    return d.row_violations_panel(X, *a, **kw)


def override_form(*a, **kw):
    return d.row_violations_panel_from(base, starts, ov_cols, ov_vals, *a, **kw)


GROUPS = (("a_dense_filter", run_a), ("b_lists", violations(dense_form, True)),
          ("c_summaries", violations(dense_form, False)), ("da_overrides_filter", run_da),
          ("db_overrides_lists", violations(override_form, True)),
          ("dc_overrides_summaries", violations(override_form, False)))


def group(fn):
    d.take_kernel_ms()
    t = time.perf_counter()
    out, down = fn()
    host = 1e3 * (time.perf_counter() - t)
    panel_ms, _ = d.take_kernel_ms()
    return out, down, host, panel_ms


def same(got, want, lists):
    """Every bit of the lists (when built) and of the summaries."""
    if lists:
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(got[2].view(np.uint64), want[2].view(np.uint64))
    assert got[3].tobytes() == want[3].tobytes()


d.take_kernel_ms()  # turns the event timing on
for _, fn in GROUPS:  # warm-up: buffers allocated, kernels loaded
    fn()
log(f"warm-up done; last_row_violations {d.last_row_violations()}")
best_dev, best_host, down_bytes = {}, {}, {}
for rnd in range(ROUNDS):
    rec = {"round": rnd}
    want = None
    for name, fn in GROUPS:
        out, down, host, dev = group(fn)
        if name == "a_dense_filter":
            want = [np.copy(part) for part in out]
        else:
            same(out, want, "summaries" not in name)
        rec[name] = {"kernel_ms": round(dev, 3), "host_ms": round(host, 3), "bytes_down": down}
        best_dev[name] = min(best_dev.get(name, 1e30), dev)
        best_host[name] = min(best_host.get(name, 1e30), host)
        down_bytes[name] = down
    rec["equal_in_every_bit"] = True
    print(json.dumps(rec), flush=True)
kept = int(want[0][K])
print(json.dumps({
    "lp": lp.name, "m": lp.m, "N": N, "k": K, "overrides": int(starts[-1]),
    "tolerance": TOLERANCE, "row_lb": float(low), "row_ub": float(high),
    "kept": kept, "violated_share": round(kept / (K * lp.m), 5),
    "points_without_violations": int(np.sum(want[3]["count"] == 0)),
    "bytes_down": down_bytes,
    "best_kernel_ms": {k: round(v, 3) for k, v in best_dev.items()},
    "best_host_ms": {k: round(v, 3) for k, v in best_host.items()},
    "host_speedup_b_over_a": round(best_host["a_dense_filter"] / best_host["b_lists"], 2),
    "host_speedup_c_over_a": round(best_host["a_dense_filter"] / best_host["c_summaries"], 2),
    "host_speedup_db_over_da": round(best_host["da_overrides_filter"] /
                                     best_host["db_overrides_lists"], 2),
    "host_speedup_dc_over_da": round(best_host["da_overrides_filter"] /
                                     best_host["dc_overrides_summaries"], 2),
}), flush=True)
d.close()
