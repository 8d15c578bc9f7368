"""Branching penalties: the dense panel followed by the rule in numpy on the
host against the panel reduced to 32-byte records on the device (DESIGN.md
section 7, "Branching penalties").

Through the probe table (include/mi_lp_devop.h), on one matrix in one process,
k = 16 candidate rows, statuses and reduced costs of a dual feasible node
(30 % BASIC, 10 % FIXED_VALUE, the rest at a bound with a reduced cost of the
right sign), integer steps on half of the columns, pivot tolerance 1e-9, after
a warm-up, three alternating rounds of
  (a) column_dots_panel (what mi_lp_get_tableau_rows launches and brings
      down), then the rule per row in numpy (tests/penalty_cases.py reference):
      what a caller does today,
  (b) column_penalties_panel.
Per group: device-event time of the kernels alone (take_kernel_ms; for (a)
that is the dense call's kernels alone), the host clock around the device call
and, for (a), around the numpy rule; bytes_down. (b) is compared with (a) in
every bit and index, every round.

Usage: python scripts/probes/branch_penalties.py dense|sparse [--small]
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
import devop_penalties  # noqa: E402
import lp_gen  # noqa: E402
import penalty_cases as pn  # noqa: E402

SEED = 20261015  # bench.py's default
K = 16
ROUNDS = 3
TOLERANCE = 1e-9


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
d = devop_penalties.PenaltiesDevOp(lp.m, lp.n, lp.col_starts, lp.row_idx, lp.vals)
N = lp.n + lp.m
log("matrix on the device")
rng = np.random.default_rng(SEED + 1)
Y = rng.standard_normal((K, lp.m))
status = rng.choice([pn.BASIC, pn.FIXED_VALUE, pn.AT_LOWER_BOUND, pn.AT_UPPER_BOUND], N,
                    p=[0.3, 0.1, 0.3, 0.3]).astype(np.int8)
cost = rng.random(N) * 10.0
rc = np.where(status == pn.AT_UPPER_BOUND, -cost, cost)
unit = np.where(rng.random(N) < 0.5, 1.0, 0.0)
down = 0.05 + 0.9 * rng.random(K)
up = 1.0 - down
# Reused result buffers, as a caller in a loop would keep them.
dense_out = np.zeros((K, N))
records = np.zeros(K, devop_penalties.RECORD)


def run_host():
    d.take_kernel_ms()
    t = time.perf_counter()
    out = d.column_dots_panel(Y, out=dense_out)
    call = 1e3 * (time.perf_counter() - t)
    dev = sum(d.take_kernel_ms())
    t = time.perf_counter()
    res = np.concatenate([pn.reference(out[j:j + 1], rc, status, unit, down[j:j + 1],
                                       up[j:j + 1], TOLERANCE) for j in range(K)])
    rule = 1e3 * (time.perf_counter() - t)
    return res, {"kernel_ms": round(dev, 3), "call_host_ms": round(call, 3),
                 "rule_host_ms": round(rule, 3), "host_ms": round(call + rule, 3),
                 "bytes_down": 8 * K * N}


def run_device():
    d.take_kernel_ms()
    t = time.perf_counter()
    res = d.column_penalties_panel(Y, rc, status, unit, down, up, TOLERANCE, out=records)
    call = 1e3 * (time.perf_counter() - t)
    dev = sum(d.take_kernel_ms())
    p = d.last_penalties()
    return res.copy(), {"kernel_ms": round(dev, 3), "host_ms": round(call, 3),
                        "bytes_down": p["bytes_down"]}


def differ(got, want):
    same = all(np.array_equal(got[f].view(np.uint64), want[f].view(np.uint64))
               for f in ("down", "up"))
    same = same and all(np.array_equal(got[f], want[f])
                        for f in ("down_col", "up_col", "down_count", "up_count"))
    return int(not same)


d.take_kernel_ms()  # turns the event timing on
d.column_dots_panel(Y, out=dense_out)
run_device()  # warm-up: buffers allocated, kernels loaded
log(f"warm-up done; last {d.last_penalties()}")
groups = ("a_dense_then_numpy_rule", "b_device_penalties")
best = {g: {} for g in groups}
for rnd in range(ROUNDS):
    rec = {"round": rnd}
    a, rec[groups[0]] = run_host()
    b, rec[groups[1]] = run_device()
    rec["differ"] = differ(b, a)
    for g in groups:
        for key in ("kernel_ms", "host_ms"):
            best[g][key] = min(best[g].get(key, 1e30), rec[g][key])
        best[g]["bytes_down"] = rec[g]["bytes_down"]
    print(json.dumps(rec), flush=True)
positive = int((b["down"] > 0).sum() + (b["up"] > 0).sum())
print(json.dumps({"lp": lp.name, "m": lp.m, "N": N, "k": K, "positive_penalties": positive,
                  "infeasible_directions": int((b["down_count"] == 0).sum() +
                                               (b["up_count"] == 0).sum()),
                  "last_penalties": d.last_penalties(), "best": best}), flush=True)
d.close()
