"""Implied column bounds of 16 bound sets (the children of a branching node)
against one matrix: the device calls against the activity ranges alone and
against the host computation a caller writes today (DESIGN.md section 7,
"Implied column bounds").

Through the probe table (include/mi_lp_devop.h), on one matrix in one process,
after a warm-up, three alternating rounds with k = 16 of
  (p)  bound_ranges_panel: phase 1 alone, the ranges with counts brought down,
  (h)  the host baseline: a numpy column walk over (p)'s downloaded ranges, the
       header's rule vectorised over the entries of one child at a time and
       reduced per column with minimum / maximum.reduceat; one thread. On the
       dense matrix it walks the first HOST_COLUMNS columns only and its time
       is scaled to n columns (stated in the summary line). It rounds as the
       header does, so it is compared with the device on bits,
  (a)  bound_implied_panel: dense form,
  (b)  bound_tightened_panel with lists,
  (c)  bound_tightened_panel, summaries only,
  (da) (db) (dc) the same three in the override form.
The node and its children are those of scripts/probes/bound_ranges.py: the
LP's own column bounds; child 2 i fixes the upper and child 2 i + 1 the lower
bound of branching column i at the middle of its box. The row bounds are the
LP's own. Per group: the host clock around the call, the device-event time of
its kernels (take_kernel_ms) and the bytes up and down. Every round asserts
that (da) equals (a) in every bit, that (b) and (db) equal the keep rule
applied in numpy to (a)'s bounds in every bit, that (c) and (dc) carry the
same summaries, and that (h) equals (a) on the columns it walked.

Usage: python scripts/probes/bound_implied.py dense|sparse [--small]
  dense   config 2's LP as bench.py generates it (10 000 x 50 000)
  sparse  config 5's LP (100 000 x 1 000 000, ~10 entries per column)
MILP_IMPLIED_COLUMNS=short|long forces a column shape. Prints one JSON line
per round and a summary line.
"""
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(R, "or-tools_amd"), os.path.join(R, "tests")]
import bound_implied_cases as ic  # noqa: E402
import devop_bound_implied  # noqa: E402
import lp_gen  # noqa: E402

SEED = 20261015  # bench.py's default
K = 16
ROUNDS = 3
TOLERANCE = 1e-9
HOST_COLUMNS = 1000  # of the dense matrix
INF = np.inf


def log(msg):
    print(f"[{time.perf_counter() - T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


T0 = time.perf_counter()
shape = sys.argv[1]
small = "--small" in sys.argv
if shape == "dense":
    m, n = (1000, 3000) if small else (10000, 50000)
    lp = lp_gen.dense_box_lp(m, n, SEED)
    host_cols = min(HOST_COLUMNS, lp.n)
else:
    m, n = (5000, 50000) if small else (100000, 1000000)
    lp = lp_gen.sparse_c5_lp(m, n, 10, SEED)
    host_cols = lp.n
log(f"{lp.name}: generated, {len(lp.vals)} entries")
d = devop_bound_implied.BoundImpliedDevOp(lp.m, lp.n, lp.col_starts, lp.row_idx, lp.vals)
log("matrix on the device")
rng = np.random.default_rng(SEED + 1)
base_lb = np.array(lp.col_lb, np.float64)
base_ub = np.array(lp.col_ub, np.float64)
boxed = np.nonzero(np.isfinite(base_lb) & np.isfinite(base_ub) & (base_ub > base_lb))[0]
branch = rng.permutation(boxed)[:K // 2]
assert len(branch) == K // 2
sets = []
for c in branch:
    mid = 0.5 * (base_lb[c] + base_ub[c])
    col = np.array([c], np.int32)
    sets.append((col, base_lb[[c]], np.array([np.floor(mid)])))
    sets.append((col, np.array([np.floor(mid) + 1.0]), base_ub[[c]]))
starts = np.arange(K + 1, dtype=np.int64)
ov_cols = np.concatenate([c for c, _, _ in sets])
ov_lo = np.concatenate([x for _, x, _ in sets])
ov_hi = np.concatenate([x for _, _, x in sets])
L, U = np.tile(base_lb, (K, 1)), np.tile(base_ub, (K, 1))
for j, (c, lo, hi) in enumerate(sets):
    L[j, c], U[j, c] = lo, hi
ROW_LB, ROW_UB = np.array(lp.row_lb, np.float64), np.array(lp.row_ub, np.float64)

# The host walk's view of the columns it covers.
COL_STARTS = np.asarray(lp.col_starts, np.int64)[:host_cols + 1]
ENTRIES = int(COL_STARTS[-1])
ROWS = np.asarray(lp.row_idx[:ENTRIES], np.int64)
VALS = np.asarray(lp.vals[:ENTRIES], np.float64)
LENS = np.diff(COL_STARTS)
COL_OF = np.repeat(np.arange(host_cols), LENS)
FILLED = LENS > 0
FIRST = COL_STARTS[:-1][FILLED]
LIVE = (VALS != 0.0) & ~np.isnan(VALS)
UP = VALS > 0.0
RUB_E, RLB_E = ROW_UB[ROWS], ROW_LB[ROWS]
log(f"host walk covers {host_cols} columns, {ENTRIES} entries")


def host_side(rb, total, count, b):
    none = count == 0
    own = (count == 1) & np.isinf(b)
    res = np.where(none, total - VALS * b, total)
    q = (rb - res) / VALS
    ok = LIVE & np.isfinite(rb) & (none | own) & np.isfinite(q)
    return q + 0.0, ok


def run_host():
    """What a caller computes on the host today, from the downloaded ranges."""
    lo, hi, lo_inf, hi_inf = RANGES
    new_l, new_u = L[:, :host_cols].copy(), U[:, :host_cols].copy()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(K):
            l_e, u_e = L[j, COL_OF], U[j, COL_OF]
            q_lo, ok_lo = host_side(RUB_E, lo[j, ROWS], lo_inf[j, ROWS], np.where(UP, l_e, u_e))
            q_hi, ok_hi = host_side(RLB_E, hi[j, ROWS], hi_inf[j, ROWS], np.where(UP, u_e, l_e))
            upper = np.where(np.where(UP, ok_lo, ok_hi), np.where(UP, q_lo, q_hi), INF)
            lower = np.where(np.where(UP, ok_hi, ok_lo), np.where(UP, q_hi, q_lo), -INF)
            least = np.minimum.reduceat(upper, FIRST)
            most = np.maximum.reduceat(lower, FIRST)
            own_u, own_l = new_u[j, FILLED], new_l[j, FILLED]
            new_u[j, FILLED] = np.where(least < own_u, least, own_u)
            new_l[j, FILLED] = np.where(most > own_l, most, own_l)
    return (new_l, new_u), 0, 0


def record():
    p = d.last_bound_implied()
    return p["bytes_down"], p["bytes_up"]


def run_p():
    global RANGES
    RANGES = d.bound_ranges_panel(L, U)
    p = d.last_bound_ranges()
    return RANGES, p["bytes_down"], 16 * K * lp.n


def run_a():
    return d.bound_implied_panel(L, U, ROW_LB, ROW_UB), *record()


def run_da():
    out = d.bound_implied_panel_from(base_lb, base_ub, starts, ov_cols, ov_lo, ov_hi, ROW_LB,
                                     ROW_UB)
    return out, *record()


def tightened(override, lists):
    def run():
        if override:
            out = d.bound_tightened_panel_from(base_lb, base_ub, starts, ov_cols, ov_lo, ov_hi,
                                               ROW_LB, ROW_UB, TOLERANCE, lists=lists)
        else:
            out = d.bound_tightened_panel(L, U, ROW_LB, ROW_UB, TOLERANCE, lists=lists)
        return out, *record()
    return run


GROUPS = (("p_ranges", run_p), ("h_host", run_host), ("a_dense", run_a),
          ("b_lists", tightened(False, True)), ("c_summaries", tightened(False, False)),
          ("da_overrides_dense", run_da), ("db_overrides_lists", tightened(True, True)),
          ("dc_overrides_summaries", tightened(True, False)))


def group(fn):
    d.take_kernel_ms()
    t = time.perf_counter()
    out, down, up = fn()
    host = 1e3 * (time.perf_counter() - t)
    panel_ms, _ = d.take_kernel_ms()
    return out, down, up, host, panel_ms


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                          np.ascontiguousarray(b).view(np.uint64))


def same_lists(got, want, lists):
    if lists:
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert same_bits(got[2], want[2]) and same_bits(got[3], want[3])
    assert got[4].tobytes() == want[4].tobytes()


d.take_kernel_ms()  # turns the event timing on
for name, fn in GROUPS:  # warm-up: buffers allocated, kernels loaded
    if name != "h_host":
        fn()
log(f"warm-up done; last_bound_implied {d.last_bound_implied()}")
best_dev, best_host, down_bytes, up_bytes = {}, {}, {}, {}
for rnd in range(ROUNDS):
    rec = {"round": rnd}
    results = {}
    for name, fn in GROUPS:
        out, down, up, host, dev = group(fn)
        results[name] = out
        rec[name] = {"kernel_ms": round(dev, 3), "host_ms": round(host, 3), "bytes_down": down,
                     "bytes_up": up}
        best_dev[name] = min(best_dev.get(name, 1e30), dev)
        best_host[name] = min(best_host.get(name, 1e30), host)
        down_bytes[name], up_bytes[name] = down, up
    a = results["a_dense"]
    for part_a, part_da in zip(a, results["da_overrides_dense"]):
        assert part_a.tobytes() == part_da.tobytes()
    want = ic.keep_reference(L, U, a[0], a[1], TOLERANCE)
    want_from = ic.keep_reference(L, U, a[0], a[1], TOLERANCE, base=(base_lb, base_ub))
    same_lists(results["b_lists"], want, True)
    same_lists(results["c_summaries"], want, False)
    same_lists(results["db_overrides_lists"], want_from, True)
    same_lists(results["dc_overrides_summaries"], want_from, False)
    h = results["h_host"]
    assert same_bits(h[0], a[0][:, :host_cols]) and same_bits(h[1], a[1][:, :host_cols])
    rec["equal_in_every_bit"] = True
    print(json.dumps(rec), flush=True)
scale = lp.n / host_cols
record_now = d.last_bound_implied()
print(json.dumps({
    "lp": lp.name, "m": lp.m, "n": lp.n, "entries": len(lp.vals), "k": K,
    "overrides": int(starts[-1]), "tolerance": TOLERANCE,
    "columns": {1: "short", 2: "long"}[record_now["columns"]],
    "forced": os.environ.get("MILP_IMPLIED_COLUMNS", ""),
    "baseline": "numpy column walk over downloaded ranges, one child at a time, one thread",
    "host_columns": host_cols, "host_scaled_by": round(scale, 3),
    "kept": int(want[0][K]), "kept_override_form": int(want_from[0][K]),
    "kept_share": round(int(want[0][K]) / (K * lp.n), 6),
    "children_proven_by_propagation": int(np.sum(want[4]["worst_row"] >= 0)),
    "columns_moved": int(np.sum(~((a[0].view(np.uint64) == L.view(np.uint64)) &
                                  (a[1].view(np.uint64) == U.view(np.uint64))))),
    "bytes_down": down_bytes, "bytes_up": up_bytes,
    "best_kernel_ms": {k: round(v, 3) for k, v in best_dev.items()},
    "best_host_ms": {k: round(v, 3) for k, v in best_host.items()},
    "host_walk_ms_scaled_to_n": round(best_host["h_host"] * scale, 1),
    "kernel_ratio_a_over_ranges": round(best_dev["a_dense"] / best_dev["p_ranges"], 2),
    "kernel_phase2_over_phase1": round((best_dev["a_dense"] - best_dev["p_ranges"]) /
                                       best_dev["p_ranges"], 2),
    "kernel_ratio_c_over_ranges": round(best_dev["c_summaries"] / best_dev["p_ranges"], 2),
}), flush=True)
d.close()
