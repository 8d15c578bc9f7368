"""Gomory cuts: the host route (dense tableau rows, the rule in numpy, a dense
row_combinations call for the slack elimination, numpy subtract and filter)
against the cuts built on the device ("Gomory cuts").

Through the probe table (include/mi_lp_devop.h), on one matrix in one process,
k = 16 rows, statuses of a dual feasible node (30 % BASIC, 10 % FIXED_VALUE,
the rest at a bound), integer steps on half of the columns, zero tolerance
1e-9, drop tolerance 1e-12, after a warm-up, three alternating rounds of
  (a) column_dots_panel (what mi_lp_get_tableau_rows launches and brings
      down), the rule per row in numpy (tests/gomory_cases.py coefficients),
      column_dots_panel again with the slack coefficients, then numpy subtract,
      filter and summaries: what a caller does today,
  (b) column_cuts_panel with lists,
  (c) column_cuts_panel, summaries only.
Per group: device-event time of the kernels alone (take_kernel_ms; for (a)
that of the two dense calls), the host clock around the device calls and, for
(a), around the numpy parts; bytes_down. (b) and (c) are compared with (a) in
every bit and index, every round. status and unit (9 N bytes) go up with every
call of (b) and (c); nothing is cached on the device between calls.

Usage: python scripts/probes/gomory_cuts.py dense|sparse [--small] [--device-only]
  dense   config 2's LP as bench.py generates it (10 000 x 50 000)
  sparse  config 5's LP (100 000 x 1 000 000, ~10 entries per column)
  --device-only  rounds of (b) and (c) alone, for a kernel trace
Prints one JSON line per round and a summary line.
"""
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(R, "or-tools_amd"), os.path.join(R, "tests")]
import devop_cuts  # noqa: E402
import gomory_cases as gc  # noqa: E402
import lp_gen  # noqa: E402

SEED = 20261015  # bench.py's default
K = 16
ROUNDS = 3
ZERO_TOLERANCE = 1e-9
DROP_TOLERANCE = 1e-12


def log(msg):
    print(f"[{time.perf_counter() - T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


T0 = time.perf_counter()
shape = sys.argv[1]
small = "--small" in sys.argv
device_only = "--device-only" in sys.argv
if shape == "dense":
    m, n = (1000, 3000) if small else (10000, 50000)
    lp = lp_gen.dense_box_lp(m, n, SEED)
else:
    m, n = (5000, 50000) if small else (100000, 1000000)
    lp = lp_gen.sparse_c5_lp(m, n, 10, SEED)
log(f"{lp.name}: generated, {len(lp.vals)} entries")
d = devop_cuts.CutsDevOp(lp.m, lp.n, lp.col_starts, lp.row_idx, lp.vals)
N = lp.n + lp.m
log("matrix on the device")
rng = np.random.default_rng(SEED + 1)
Y = rng.standard_normal((K, lp.m))
status = rng.choice([gc.BASIC, gc.FIXED_VALUE, gc.AT_LOWER_BOUND, gc.AT_UPPER_BOUND], N,
                    p=[0.3, 0.1, 0.3, 0.3]).astype(np.int8)
unit = np.where(rng.random(N) < 0.5, 1.0, 0.0)
f0 = 0.05 + 0.9 * rng.random(K)
row_unit = np.ones(K)
# Reused result buffers, as a caller in a loop would keep them.
dense_out = np.zeros((K, N))
dense_out2 = np.zeros((K, N))
summaries = np.zeros(K, devop_cuts.SUMMARY)


def run_host():
    d.take_kernel_ms()
    t = time.perf_counter()
    alpha = d.column_dots_panel(Y, out=dense_out)
    call = 1e3 * (time.perf_counter() - t)
    t = time.perf_counter()
    g, bad = gc.coefficients(alpha, status, unit, f0, row_unit, ZERO_TOLERANCE)
    slack = np.ascontiguousarray(g[:, lp.n:])
    rule = 1e3 * (time.perf_counter() - t)
    t = time.perf_counter()
    s = d.column_dots_panel(slack, out=dense_out2)
    call += 1e3 * (time.perf_counter() - t)
    dev = sum(d.take_kernel_ms())
    t = time.perf_counter()
    c = g[:, :lp.n] - s[:, :lp.n]
    res = gc.cut_lists(c, DROP_TOLERANCE) + (gc.summarize(c, DROP_TOLERANCE, bad.sum(axis=1)),)
    rule += 1e3 * (time.perf_counter() - t)
    return res, {"kernel_ms": round(dev, 3), "calls_host_ms": round(call, 3),
                 "numpy_host_ms": round(rule, 3), "host_ms": round(call + rule, 3),
                 "bytes_down": 2 * 8 * K * N}


def run_device(lists):
    d.take_kernel_ms()
    t = time.perf_counter()
    res = d.column_cuts_panel(Y, status, unit, f0, row_unit, ZERO_TOLERANCE, DROP_TOLERANCE,
                              lists=lists, summaries=summaries)
    call = 1e3 * (time.perf_counter() - t)
    dev = sum(d.take_kernel_ms())
    p = d.last_cuts()
    return res[:3] + (res[3].copy(),), {"kernel_ms": round(dev, 3), "host_ms": round(call, 3),
                                        "bytes_down": p["bytes_down"], "kept": p["kept"]}


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def differ(got, want, lists):
    same = all(np.array_equal(u64(got[3][f]), u64(want[3][f])) for f in ("max_abs", "min_abs"))
    same = same and all(np.array_equal(got[3][f], want[3][f])
                        for f in ("count", "bad_count", "max_col", "min_col"))
    if lists:
        same = same and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) \
            and np.array_equal(u64(got[2]), u64(want[2]))
    return int(not same)


d.take_kernel_ms()  # turns the event timing on
d.column_dots_panel(Y, out=dense_out)
run_device(True)  # warm-up: buffers allocated, kernels loaded
run_device(False)
log(f"warm-up done; last {d.last_cuts()}")
groups = ("a_host_route", "b_device_cuts", "c_device_summaries_only")
best = {g: {} for g in groups}
for rnd in range(ROUNDS):
    rec = {"round": rnd}
    if not device_only:
        a, rec[groups[0]] = run_host()
    b, rec[groups[1]] = run_device(True)
    c, rec[groups[2]] = run_device(False)
    if not device_only:
        rec["differ"] = differ(b, a, True) + differ(c, a, False)
    for g in groups:
        if g in rec:
            for key in ("kernel_ms", "host_ms"):
                best[g][key] = min(best[g].get(key, 1e30), rec[g][key])
            best[g]["bytes_down"] = rec[g]["bytes_down"]
    print(json.dumps(rec), flush=True)
print(json.dumps({"lp": lp.name, "m": lp.m, "N": N, "k": K, "kept": int(b[0][-1]),
                  "bad_cuts": int((b[3]["bad_count"] > 0).sum()),
                  "bytes_up_per_call": 9 * N + 16 * K + 8 * K * lp.m,
                  "last_cuts": d.last_cuts(), "best": best}), flush=True)
d.close()
