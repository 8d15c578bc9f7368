"""Activity ranges of 16 bound sets (the children of a branching node) against
one matrix: the device calls against the host computation a caller writes today
("Bound-set activity ranges").

Through the probe table (include/mi_lp_devop.h), on one matrix in one process,
after a warm-up, three alternating rounds with k = 16 of
  (h)  the host baseline: scipy sparse products with A split by sign
       (A+ L + A- U and its mirror image, infinite bounds counted through
       indicator matrices when there are any), then the screening in numpy.
       scipy's sparse-times-dense product runs on one thread whatever the
       process's share of 16 is; it sums in its own order, so it is compared
       with the device to 1e-9 relative to sum |a b|, not on bits,
  (a)  bound_ranges_panel: dense form, ranges with counts,
  (b)  bound_infeasible_panel with lists,
  (c)  bound_infeasible_panel, summaries only,
  (da) (db) (dc) the same three in the override form,
  (r)  row_sums_panel of 16 points on the same matrix, run beside them.
The node is the LP's own column bounds; child 2 i fixes the upper and child
2 i + 1 the lower bound of branching column i at the middle of its box, so the
override form carries one overridden column per child. The row bounds are the
LP's own. Per group: the host clock around the call, the device-event time of
its kernels (take_kernel_ms) and the bytes up and down. Every round asserts
that (da) equals (a) in every bit, that (b) and (db) equal the screening of
(a)'s ranges done in numpy with the header's rule in every bit, and that (c)
and (dc) carry the same summaries.

Usage: python scripts/probes/bound_ranges.py dense|sparse [--small]
  dense   config 2's LP as bench.py generates it (10 000 x 50 000)
  sparse  config 5's LP (100 000 x 1 000 000, ~10 entries per column)
Prints one JSON line per round and a summary line.
"""
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(R, "or-tools_amd"), os.path.join(R, "tests")]
import devop_bound_ranges  # noqa: E402
import lp_gen  # noqa: E402

SEED = 20261015  # bench.py's default
K = 16
ROUNDS = 3
TOLERANCE = 1e-9
SUMMARY = devop_bound_ranges.SUMMARY
INF = np.inf


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
d = devop_bound_ranges.BoundRangesDevOp(lp.m, lp.n, lp.col_starts, lp.row_idx, lp.vals)
N = lp.n + lp.m
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
X = rng.standard_normal((K, N))
sums_out = np.zeros(K * lp.m)

# The host baseline's matrices: A+ and A- share A's index arrays.
vals = np.asarray(lp.vals, np.float64)
index_type = np.int32 if len(vals) < 2 ** 31 else np.int64  # one type: scipy copies otherwise
pattern = (np.asarray(lp.row_idx, index_type), np.asarray(lp.col_starts, index_type))
A_POS = sp.csc_matrix((np.maximum(vals, 0.0), *pattern), shape=(lp.m, lp.n))
A_NEG = sp.csc_matrix((np.minimum(vals, 0.0), *pattern), shape=(lp.m, lp.n))
ANY_INF = bool(np.isinf(L).any() or np.isinf(U).any())
if ANY_INF:
    IS_POS = sp.csc_matrix(((vals > 0.0).astype(np.float64), *pattern), shape=(lp.m, lp.n))
    IS_NEG = sp.csc_matrix(((vals < 0.0).astype(np.float64), *pattern), shape=(lp.m, lp.n))
# sum |a| max(|l|, |u|) per (row, child): what the host's own summation order
# is allowed to differ by, relative.
_largest = np.maximum(np.abs(np.where(np.isinf(L), 0.0, L)), np.abs(np.where(np.isinf(U), 0.0, U)))
SCALE = (A_POS @ _largest.T - A_NEG @ _largest.T).T + 1e-300
log(f"host matrices built; infinite bounds: {ANY_INF}")


def screen(lo, hi, lo_inf, hi_inf):
    """The header's screening over the k x m ranges, in numpy."""
    g = np.full(lo.shape, -INF)
    with np.errstate(invalid="ignore"):
        over = lo - ROW_UB
        g = np.where((lo_inf == 0) & (over > g), over, g)
        under = ROW_LB - hi
        g = np.where((hi_inf == 0) & (under > g), under, g)
    keep = g > TOLERANCE
    row_starts = np.zeros(K + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=row_starts[1:])
    child, row = np.nonzero(keep)
    amounts = g[child, row]
    summaries = np.zeros(K, SUMMARY)
    summaries["count"] = np.diff(row_starts)
    summaries["worst_row"] = -1
    for j in range(K):
        s, e = row_starts[j], row_starts[j + 1]
        if e > s:
            at = s + np.argmax(amounts[s:e])  # the first maximum: the lowest row
            summaries["worst"][j], summaries["worst_row"][j] = amounts[at], row[at]
    return row_starts, row.astype(np.int32), amounts, summaries


def run_host():
    """What a caller computes on the host today."""
    Lt, Ut = L.T, U.T
    if ANY_INF:
        l_inf, u_inf = np.isinf(Lt), np.isinf(Ut)
        Lf, Uf = np.where(l_inf, 0.0, Lt), np.where(u_inf, 0.0, Ut)
        lo_inf = (IS_POS @ l_inf.astype(np.float64) + IS_NEG @ u_inf.astype(np.float64)).T
        hi_inf = (IS_POS @ u_inf.astype(np.float64) + IS_NEG @ l_inf.astype(np.float64)).T
    else:
        Lf, Uf = np.ascontiguousarray(Lt), np.ascontiguousarray(Ut)
        lo_inf = hi_inf = np.zeros((K, lp.m))
    lo = (A_POS @ Lf + A_NEG @ Uf).T
    hi = (A_POS @ Uf + A_NEG @ Lf).T
    lo_inf, hi_inf = lo_inf.astype(np.int32), hi_inf.astype(np.int32)
    return (lo, hi, lo_inf, hi_inf, screen(lo, hi, lo_inf, hi_inf)), 0, 0


def record():
    p = d.last_bound_ranges()
    return p["bytes_down"], p["overrides_up_bytes"] or 16 * K * lp.n


def run_a():
    out = d.bound_ranges_panel(L, U)
    return out, *record()


def run_da():
    out = d.bound_ranges_panel_from(base_lb, base_ub, starts, ov_cols, ov_lo, ov_hi)
    return out, *record()


def screening(override, lists):
    def run():
        if override:
            out = d.bound_infeasible_panel_from(base_lb, base_ub, starts, ov_cols, ov_lo, ov_hi,
                                                ROW_LB, ROW_UB, TOLERANCE, lists=lists)
        else:
            out = d.bound_infeasible_panel(L, U, ROW_LB, ROW_UB, TOLERANCE, lists=lists)
        return out, *record()
    return run


def run_r():
    return d.row_sums_panel(X, out=sums_out), 8 * K * lp.m, 8 * K * N


GROUPS = (("h_host", run_host), ("a_ranges", run_a), ("b_lists", screening(False, True)),
          ("c_summaries", screening(False, False)), ("da_overrides_ranges", run_da),
          ("db_overrides_lists", screening(True, True)),
          ("dc_overrides_summaries", screening(True, False)), ("r_row_sums", run_r))


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
        assert same_bits(got[2], want[2])
    assert got[3].tobytes() == want[3].tobytes()


d.take_kernel_ms()  # turns the event timing on
for name, fn in GROUPS[1:]:  # warm-up: buffers allocated, kernels loaded
    fn()
log(f"warm-up done; last_bound_ranges {d.last_bound_ranges()}")
best_dev, best_host, down_bytes, up_bytes = {}, {}, {}, {}
host_gap = 0.0
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
    a = results["a_ranges"]
    for part_a, part_da in zip(a, results["da_overrides_ranges"]):
        assert part_a.tobytes() == part_da.tobytes()
    want = screen(*a)
    for name in ("b_lists", "db_overrides_lists", "c_summaries", "dc_overrides_summaries"):
        same_lists(results[name], want, "lists" in name)
    rec["equal_in_every_bit"] = True
    h = results["h_host"]
    assert np.array_equal(h[2], a[2]) and np.array_equal(h[3], a[3])
    gap = max(float(np.max(np.abs(h[0] - a[0]) / SCALE)),
              float(np.max(np.abs(h[1] - a[1]) / SCALE)))
    assert gap <= 1e-9, gap
    host_gap = max(host_gap, gap)
    print(json.dumps(rec), flush=True)
kept = int(want[0][K])
print(json.dumps({
    "lp": lp.name, "m": lp.m, "n": lp.n, "k": K, "overrides": int(starts[-1]),
    "baseline": "scipy CSC products, A split by sign, one thread", "tolerance": TOLERANCE,
    "infinite_bounds": ANY_INF, "kept": kept, "proven_share": round(kept / (K * lp.m), 5),
    "children_without_proving_rows": int(np.sum(want[3]["count"] == 0)),
    "host_against_device_max_gap": host_gap,
    "bytes_down": down_bytes, "bytes_up": up_bytes,
    "best_kernel_ms": {k: round(v, 3) for k, v in best_dev.items()},
    "best_host_ms": {k: round(v, 3) for k, v in best_host.items()},
    "host_speedup_a_over_h": round(best_host["h_host"] / best_host["a_ranges"], 2),
    "host_speedup_da_over_h": round(best_host["h_host"] / best_host["da_overrides_ranges"], 2),
    "host_speedup_dc_over_h": round(best_host["h_host"] / best_host["dc_overrides_summaries"], 2),
    "kernel_ratio_a_over_row_sums": round(best_dev["a_ranges"] / best_dev["r_row_sums"], 2),
}), flush=True)
d.close()
