"""Bound propagation of 16 bound sets (the children of a node) to a fixpoint
against one matrix: the device round loop against the way a caller reached the
same result before it, one tightened_columns_from call per round with the
rounding and the merge on the host ("Bound propagation").

Through the probe table (include/mi_lp_devop.h), on one matrix in one process,
after a warm-up, three alternating rounds with k = 16 of
  (n)  bound_propagated_columns_from with lists,
  (ns) the same, summaries only,
  (f)  the fed-back loop: per round one bound_tightened_panel_from with lists,
       then on the host the header's rounding and move rule on the listed
       columns (numpy, one set at a time) and the merge into the set's override
       list, which goes up again with the next round. It stops per set as the
       rule does. Asserted equal to (n) in every bit of every list and summary
       before any time is reported.
Nodes:
  branch   scripts/probes/bound_ranges.py's branching node: the LP's own column
           bounds; child 2 i fixes the upper and child 2 i + 1 the lower bound
           of branching column i at the middle of its box; the LP's own row
           bounds.
  witness  the node of tests/bound_propagate_cases.py at size: an infinite
           column bound of the base becomes the finite side -+ 10 (a free
           column [-10, 10]); the witness x0 is the box midpoint, rounded on
           integer columns; ub = A x0 + 0.05 w on rows with r % 4 in {0, 2},
           lb = A x0 - 0.05 w on rows with r % 4 in {1, 2}, w = hi - lo of
           that base's activity range; child 0 is the base, child j overrides
           1 + j % 3 random columns, even j with a box of a tenth of the width
           around x0, odd j with a lower bound 60 % of the way from x0 to u,
           integer columns rounded inward.
  range_ends  NOT a node a search would meet, kept to load the round loop: the
           finite base and the branch children under row bounds at the ends
           of every row's range, ub = lo + F w and lb = hi - F w on the same
           rows (F = 0.02 unless --f). Nearly every column moves in round 1
           and every child is infeasible within a few rounds.
Integer columns are c % 3 == 0, tolerance 1e-9, integrality tolerance 1e-6,
max_rounds 30. Per group: the host clock around the call(s), the device-event
time of the kernels (take_kernel_ms), the bytes up and down, the rounds.

Usage: python scripts/probes/bound_propagate.py dense|sparse [--small] [--f F]
  dense   config 2's LP as bench.py generates it (10 000 x 50 000)
  sparse  config 5's LP (100 000 x 1 000 000, ~10 entries per column)
Prints one JSON line per node and round and a summary line per node.
"""
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(R, "or-tools_amd"), os.path.join(R, "tests")]
import devop_bound_propagate  # noqa: E402
import lp_gen  # noqa: E402

SEED = 20261015  # bench.py's default
K = 16
ROUNDS = 3
TOLERANCE = 1e-9
ITOL = 1e-6
MAX_ROUNDS = 30
INF = np.inf
INFEASIBLE, FIXPOINT = 2, 1


def log(msg):
    print(f"[{time.perf_counter() - T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


T0 = time.perf_counter()
shape = sys.argv[1]
small = "--small" in sys.argv
F = float(sys.argv[sys.argv.index("--f") + 1]) if "--f" in sys.argv else 0.02
if shape == "dense":
    m, n = (1000, 3000) if small else (10000, 50000)
    lp = lp_gen.dense_box_lp(m, n, SEED)
else:
    m, n = (5000, 50000) if small else (100000, 1000000)
    lp = lp_gen.sparse_c5_lp(m, n, 10, SEED)
log(f"{lp.name}: generated, {len(lp.vals)} entries")
d = devop_bound_propagate.BoundPropagateDevOp(lp.m, lp.n, lp.col_starts, lp.row_idx, lp.vals)
log("matrix on the device")
rng = np.random.default_rng(SEED + 1)
base_lb = np.array(lp.col_lb, np.float64)
base_ub = np.array(lp.col_ub, np.float64)
IS_INTEGER = (np.arange(lp.n) % 3 == 0).astype(np.uint8)
INTS = IS_INTEGER != 0
# Integer columns start from integral bounds, as a MIP's do.
base_lb[INTS], base_ub[INTS] = np.floor(base_lb[INTS]), np.ceil(base_ub[INTS])
boxed = np.nonzero(np.isfinite(base_lb) & np.isfinite(base_ub) & (base_ub > base_lb))[0]
branch = rng.permutation(boxed)[:K // 2]
assert len(branch) == K // 2


def children():
    out = []
    for c in branch:
        mid = 0.5 * (base_lb[c] + base_ub[c])
        col = np.array([c], np.int32)
        out.append((col, base_lb[[c]], np.array([np.floor(mid)])))
        out.append((col, np.array([np.floor(mid) + 1.0]), base_ub[[c]]))
    return out


sets = children()


def flatten(override_sets):
    starts = np.zeros(len(override_sets) + 1, np.int64)
    np.cumsum([len(c) for c, _, _ in override_sets], out=starts[1:])
    return (starts, np.concatenate([c for c, _, _ in override_sets]).astype(np.int32),
            np.concatenate([x for _, x, _ in override_sets]),
            np.concatenate([x for _, _, x in override_sets]))


def range_end_rows():
    lo, hi, lo_inf, hi_inf = d.bound_ranges_panel(base_lb[None, :], base_ub[None, :])
    lo, hi = lo[0], hi[0]
    finite = (lo_inf[0] == 0) & (hi_inf[0] == 0) & np.isfinite(lo) & np.isfinite(hi)
    w = hi - lo
    r = np.arange(lp.m)
    lb, ub = np.full(lp.m, -INF), np.full(lp.m, INF)
    upper, lower = finite & np.isin(r % 4, (0, 2)), finite & np.isin(r % 4, (1, 2))
    ub[upper] = lo[upper] + F * w[upper]
    lb[lower] = hi[lower] - F * w[lower]
    return lb, ub


def finite_box():
    lb = np.where(np.isfinite(base_lb), base_lb,
                  np.where(np.isfinite(base_ub), base_ub - 10.0, -10.0))
    ub = np.where(np.isfinite(base_ub), base_ub, lb + 20.0)
    return lb, ub


WITNESS_F = 0.05


def witness_node():
    """(sets, row_lb, row_ub) over the current (finite) base."""
    x0 = 0.5 * (base_lb + base_ub)
    x0[INTS] = np.round(x0[INTS])
    lo, hi, lo_inf, hi_inf = d.bound_ranges_panel(base_lb[None, :], base_ub[None, :])
    assert not lo_inf.any() and not hi_inf.any()
    activity = d.bound_ranges_panel(x0[None, :], x0[None, :])[0][0]
    w = hi[0] - lo[0]
    r = np.arange(lp.m)
    lb, ub = np.full(lp.m, -INF), np.full(lp.m, INF)
    upper, lower = np.isin(r % 4, (0, 2)), np.isin(r % 4, (1, 2))
    ub[upper] = activity[upper] + WITNESS_F * w[upper]
    lb[lower] = activity[lower] - WITNESS_F * w[lower]
    draw = np.random.default_rng(SEED + 2)
    width = base_ub - base_lb
    out = [(np.zeros(0, np.int32), np.zeros(0), np.zeros(0))]
    for j in range(1, K):
        cols = np.sort(draw.choice(lp.n, 1 + j % 3, replace=False)).astype(np.int32)
        ints = INTS[cols]
        if j % 2 == 0:
            lo_c, hi_c = x0[cols] - 0.05 * width[cols], x0[cols] + 0.05 * width[cols]
            lo_c, hi_c = np.where(ints, np.ceil(lo_c), lo_c), np.where(ints, np.floor(hi_c), hi_c)
        else:
            lo_c = x0[cols] + 0.6 * (base_ub[cols] - x0[cols])
            lo_c, hi_c = np.where(ints, np.ceil(lo_c), lo_c), base_ub[cols].copy()
        out.append((cols, lo_c, hi_c))
    return out, lb, ub


NODES = ("branch", "witness", "range_ends")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run_n(row_lb, row_ub, lists):
    out = d.bound_propagated_columns_from(base_lb, base_ub, *flatten(sets), row_lb, row_ub,
                                          IS_INTEGER, TOLERANCE, ITOL, MAX_ROUNDS, lists=lists)
    p = d.last_bound_propagate()
    return out, p["bytes_down"], p["bytes_up"], p["rounds"]


def run_f(row_lb, row_ub):
    """The parent's way: dense host copies of the sets, one tightened call per
    round, rounding, move rule and merge in numpy."""
    L, U = np.tile(base_lb, (K, 1)), np.tile(base_ub, (K, 1))
    changed = []
    for j, (c, lo, hi) in enumerate(sets):
        L[j, c], U[j, c] = lo, hi
        changed.append(np.asarray(c, np.int64))
    summaries = np.zeros(K, devop_bound_propagate.SUMMARY)
    summaries["worst_col"] = -1
    active = np.ones(K, bool)
    down = up = rounds = 0
    for rnd in range(1, MAX_ROUNDS + 1):
        if not active.any():
            break
        current = [(changed[j].astype(np.int32), L[j, changed[j]], U[j, changed[j]])
                   for j in range(K)]
        col_starts, cols, nl, nu, _ = d.bound_tightened_panel_from(
            base_lb, base_ub, *flatten(current), row_lb, row_ub, TOLERANCE)
        p = d.last_bound_implied()
        down, up, rounds = down + p["bytes_down"], up + p["bytes_up"], rounds + 1
        for j in np.nonzero(active)[0]:
            idx = cols[col_starts[j]:col_starts[j + 1]].astype(np.int64)
            a, b = nl[col_starts[j]:col_starts[j + 1]].copy(), nu[col_starts[j]:col_starts[j + 1]].copy()
            ints = INTS[idx]
            with np.errstate(invalid="ignore", over="ignore"):
                a[ints] = np.ceil(a[ints] - ITOL) + 0.0
                b[ints] = np.floor(b[ints] + ITOL) + 0.0
                l, u = L[j, idx], U[j, idx]
                moved = (a - l > TOLERANCE) | (u - b > TOLERANCE)
                l2, u2 = np.where(moved, a, l), np.where(moved, b, u)
                cross = l2 - u2
                crossing = cross > TOLERANCE
            L[j, idx], U[j, idx] = l2, u2
            merged = np.union1d(changed[j], idx[moved])
            keep = (bits(L[j, merged]) != bits(base_lb[merged])) | \
                (bits(U[j, merged]) != bits(base_ub[merged]))
            changed[j] = merged[keep]
            summaries["rounds"][j] = rnd
            summaries["moves"][j] += int(moved.sum())
            if crossing.any():
                worst = cross[crossing].max()
                summaries["status"][j] = INFEASIBLE
                summaries["worst"][j] = worst
                summaries["worst_col"][j] = idx[crossing & (cross == worst)].min()
                active[j] = False
            elif not moved.any():
                summaries["status"][j] = FIXPOINT
                active[j] = False
    # The lists of the result: the changed columns and, for an infeasible set,
    # the columns that cross.
    out_cols, out_l, out_u = [], [], []
    starts = np.zeros(K + 1, np.int64)
    for j in range(K):
        keep = changed[j]
        if summaries["status"][j] == INFEASIBLE:
            with np.errstate(invalid="ignore", over="ignore"):
                keep = np.union1d(keep, np.nonzero(L[j] - U[j] > TOLERANCE)[0])
        summaries["kept"][j] = len(keep)
        starts[j + 1] = starts[j] + len(keep)
        out_cols.append(keep.astype(np.int32))
        out_l.append(L[j, keep])
        out_u.append(U[j, keep])
    out = (starts, np.concatenate(out_cols), np.concatenate(out_l), np.concatenate(out_u),
           summaries)
    return out, down, up, rounds


def group(fn):
    d.take_kernel_ms()
    t = time.perf_counter()
    out, down, up, rounds = fn()
    host = 1e3 * (time.perf_counter() - t)
    panel_ms, _ = d.take_kernel_ms()
    return out, {"kernel_ms": round(panel_ms, 3), "host_ms": round(host, 3), "bytes_down": down,
                 "bytes_up": up, "rounds": rounds}


d.take_kernel_ms()  # turns the event timing on
for node in NODES:
    if node == "branch":
        row_lb, row_ub = np.array(lp.row_lb, np.float64), np.array(lp.row_ub, np.float64)
    elif node == "witness":
        base_lb, base_ub = finite_box()
        sets, row_lb, row_ub = witness_node()
    else:
        sets = children()
        row_lb, row_ub = range_end_rows()
    groups = (("n_lists", lambda: run_n(row_lb, row_ub, True)),
              ("ns_summaries", lambda: run_n(row_lb, row_ub, False)),
              ("f_fed_back", lambda: run_f(row_lb, row_ub)))
    for _, fn in groups:  # warm-up: buffers allocated, kernels loaded
        fn()
    log(f"{node}: warm-up done; last_bound_propagate {d.last_bound_propagate()}")
    best = {}
    for rnd in range(ROUNDS):
        rec, results = {"node": node, "round": rnd}, {}
        for name, fn in groups:
            results[name], rec[name] = group(fn)
            for key in ("kernel_ms", "host_ms"):
                best[name, key] = min(best.get((name, key), 1e30), rec[name][key])
        got, want = results["n_lists"], results["f_fed_back"]
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(bits(got[2]), bits(want[2]))
        assert np.array_equal(bits(got[3]), bits(want[3]))
        assert got[4].tobytes() == want[4].tobytes(), (got[4], want[4])
        assert results["ns_summaries"][4].tobytes() == got[4].tobytes()
        rec["equal_in_every_bit"] = True
        print(json.dumps(rec), flush=True)
    s = got[4]
    launched = rec["n_lists"]["rounds"]
    fed = rec["f_fed_back"]["rounds"]
    print(json.dumps({
        "lp": lp.name, "m": lp.m, "n": lp.n, "entries": len(lp.vals), "k": K, "node": node,
        "f": {"witness": WITNESS_F, "range_ends": F}.get(node), "tolerance": TOLERANCE, "integrality_tolerance": ITOL, "max_rounds": MAX_ROUNDS,
        "columns": {1: "short", 2: "long"}[d.last_bound_propagate()["columns"]],
        "status": s["status"].tolist(), "rounds": s["rounds"].tolist(),
        "moves": s["moves"].tolist(), "kept": s["kept"].tolist(),
        "rounds_launched": launched, "rounds_fed_back": fed,
        "bytes": {name: {"up": rec[name]["bytes_up"], "down": rec[name]["bytes_down"]}
                  for name, _ in groups},
        "best_kernel_ms": {name: best[name, "kernel_ms"] for name, _ in groups},
        "best_host_ms": {name: best[name, "host_ms"] for name, _ in groups},
        "per_round_kernel_ms": {"n_lists": round(best["n_lists", "kernel_ms"] / launched, 3),
                                "f_fed_back": round(best["f_fed_back", "kernel_ms"] / fed, 3)},
        "per_round_host_ms": {"n_lists": round(best["n_lists", "host_ms"] / launched, 3),
                              "f_fed_back": round(best["f_fed_back", "host_ms"] / fed, 3)},
    }), flush=True)
d.close()
