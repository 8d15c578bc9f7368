"""tests/tri_ref.py, the reference of the operation-level tests of the device
triangular solves, against the engine's host loops (engine/lu.h) on every
case of tests/tri_cases.py up to 20 000 rows, bit for bit; against exact
arithmetic; and the conditions the inputs must meet for a bit comparison to
tell a wrong evaluation order from the right one. No GPU.

The host loops run in a stand-alone C++ program that links the engine
library's host code (as tests/test_tri_par_cpu.py does) with
MILP_HOST_TRI_PAR=0: the serial loops. It builds each matrix with Reset and
AddTriangularColumn, as the probe's tri_set_matrix does.
"""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import tri_cases as tc
import tri_ref
from tri_ref import LOWER, UPPER, UPPER_T, UPPER_T_UP, bits

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r"""
#include "lu.h"
#include <cstdint>
#include <cstdio>
#include <vector>
// in: problems of (n, nnz, kind, start; starts[n + 1], rows[nnz] (int32),
// vals[nnz], diag[n], x[n]); out: the solved x of each.
template <typename T>
static bool Get(FILE* f, std::vector<T>* v, size_t n) {
  v->resize(n);
  return n == 0 || std::fread(v->data(), sizeof(T), n, f) == n;
}
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  if (in == nullptr || out == nullptr) return 2;
  int64_t head[4];
  while (std::fread(head, sizeof(int64_t), 4, in) == 4) {
    const int n = static_cast<int>(head[0]);
    std::vector<int64_t> starts;
    std::vector<int32_t> rows;
    std::vector<double> vals, diag, x;
    if (!Get(in, &starts, n + 1) || !Get(in, &rows, head[1]) || !Get(in, &vals, head[1]) ||
        !Get(in, &diag, n) || !Get(in, &x, n)) {
      return 3;
    }
    milp::TriangularMatrix t;
    t.Reset(n, n);
    std::vector<int> r;
    std::vector<double> v;
    for (int c = 0; c < n; ++c) {
      r.assign(rows.begin() + starts[c], rows.begin() + starts[c + 1]);
      v.assign(vals.begin() + starts[c], vals.begin() + starts[c + 1]);
      r.push_back(c);
      v.push_back(diag[c]);
      milp::ColumnView view;
      view.rows = r.data();
      view.coefs = v.data();
      view.n = static_cast<int64_t>(r.size());
      t.AddTriangularColumn(view, c);
    }
    switch (head[2]) {
      case 0: case 3: t.TransposeLowerSolve(&x); break;
      case 2: t.TransposeUpperSolve(&x); break;
      case 1: case 4: t.LowerSolveStartingAt(static_cast<int>(head[3]), &x); break;
      case 5: t.UpperSolve(&x); break;
      default: return 4;
    }
    if (std::fwrite(x.data(), sizeof(double), n, out) != static_cast<size_t>(n)) return 5;
  }
  std::fclose(out);
  return 0;
}
"""

HOST_ROWS_MAX = 20000
HOST_CASES = [n for n in tc.SPECS if sum(tc.SPECS[n]["widths"]) <= HOST_ROWS_MAX]


@pytest.fixture(scope="module")
def host_solver(tmp_path_factory):
    d = tmp_path_factory.mktemp("tri_host")
    src, exe = d / "host.cc", d / "host"
    src.write_text(PROG)
    lib = os.path.join(REPO, "or-tools_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off",
                    "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
                    "-I", os.path.join(REPO, "or-tools_amd", "csrc", "engine"), str(src),
                    "-o", str(exe), "-L", lib, "-lmi_lp", f"-Wl,-rpath,{lib}"], check=True)
    calls = [0]

    def run(problems):
        """[(kind, Tri, x, start)] -> the host loops' results."""
        calls[0] += 1
        fin, fout = d / f"in{calls[0]}.bin", d / f"out{calls[0]}.bin"
        with open(fin, "wb") as f:
            for kind, t, x, start in problems:
                np.array([t.n, len(t.rows), kind, start], np.int64).tofile(f)
                for a in (t.starts, t.rows, t.vals, t.diag, np.asarray(x, np.float64)):
                    a.tofile(f)
        env = dict(os.environ, MILP_HOST_TRI_PAR="0")
        r = subprocess.run([str(exe), str(fin), str(fout)], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stderr)
        flat = np.fromfile(fout, np.float64)
        os.remove(fin)
        os.remove(fout)
        outs, o = [], 0
        for _, t, _, _ in problems:
            outs.append(flat[o:o + t.n])
            o += t.n
        assert o == len(flat)
        return outs

    return run


def same_bits(got, want, what):
    bad = np.nonzero(bits(got) != bits(want))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(want)} differ, first at row {bad[0]}: "
                           f"{got[bad[0]]!r} against the reference's {want[bad[0]]!r}")


@pytest.mark.parametrize("name", HOST_CASES)
def test_host_loops_give_the_reference_bits(name, host_solver):
    problems, labels = [], []
    for kind in tc.ALL_KINDS:
        t = tc.tri_of(name, kind)
        for label, x, start in tc.rhs_list(name, kind, full=name not in tc.BIG):
            problems.append((kind, t, x, start))
            labels.append(f"{name} {tri_ref.KIND_NAMES[kind]} {label}")
    outs = host_solver(problems)
    for (kind, t, x, start), got, what in zip(problems, outs, labels):
        same_bits(got, tri_ref.solve(kind, t, x, start), what)


def test_host_loops_give_the_reference_bits_on_the_planted_events(host_solver):
    problems, labels, rows = [], [], []
    for kind in tc.ALL_KINDS:
        for unit in (False, True):
            for which in ("inf_meets_zero", "cancellation"):
                if which == "cancellation" and kind not in tri_ref.SEQUENTIAL:
                    continue
                t, x, ev = tc.special_tri(kind, which, unit)
                problems.append((kind, t, x, 0))
                labels.append((kind, which, unit))
                rows.append(ev)
    outs = host_solver(problems)
    for (kind, t, x, _), got, (_, which, unit), ev in zip(problems, outs, labels, rows):
        ref = tri_ref.solve(kind, t, x)
        same_bits(got, ref, f"{tri_ref.KIND_NAMES[kind]} {which} unit={unit}")
        if which == "inf_meets_zero":
            # inf * 0 is NaN in a grouped sum; a scatter loop skips the column.
            assert np.isnan(ref).any() == (kind in tri_ref.GROUPED)
        else:
            # The cancelled outputs are +0.0 (not divided by their negative
            # diagonal), and nothing read the infinite coefficients behind them.
            assert (bits(ref[ev]) == 0).all() and np.isfinite(ref).all()


def test_host_loops_give_the_reference_bits_on_the_dense_tails(host_solver):
    problems, labels = [], []
    for T in tc.TAIL_COLS:
        for unit in (False, True):
            for identity in (False, True):
                for offset in range(len(tc.TAIL_VARIANTS) if T == 1 else 1):
                    t, first, used = tc.tail_tri(T, unit, identity, offset)
                    assert first == t.n - T
                    if T >= 63:  # every variant and every column-length remainder
                        assert {v for v, _ in used} == set(tc.TAIL_VARIANTS)
                        assert {k % 4 for _, k in used} == {0, 1, 2, 3}
                        assert any(v == "tail_row_first" and k > 72 + 4 for v, k in used)
                    rng = np.random.default_rng(T)
                    for rep in range(2):
                        problems.append((UPPER_T_UP, t, tc.dense_rhs(rng, t.n), 0))
                        labels.append(f"tail T={T} unit={unit} identity={identity} {rep}")
    outs = host_solver(problems)
    for (kind, t, x, _), got, what in zip(problems, outs, labels):
        ref = tri_ref.solve(kind, t, x)
        same_bits(got, ref, what)
        assert np.isfinite(ref).all() and (ref != 0).all()


# --- the reference against exact arithmetic ---------------------------------------------------------

def gather_lists(kind, t):
    """Per output row: its entries (row read, coefficient) in evaluation
    order. The scatter loops are restated as gathers over the matrix's rows,
    by ascending (kLower, kUnitRow) or descending (kUpper) column."""
    st, rows, vals, _ = t.lists()
    lists = [[] for _ in range(t.n)]
    if kind in tri_ref.GROUPED:
        for c in range(t.n):
            e = list(zip(rows[st[c]:st[c + 1]], vals[st[c]:st[c + 1]]))
            lists[c] = e if kind == UPPER_T_UP else e[::-1]
        return lists
    cols = range(t.n) if kind != UPPER else range(t.n - 1, -1, -1)
    for c in cols:
        idx = range(st[c], st[c + 1]) if kind != UPPER else range(st[c + 1] - 1, st[c] - 1, -1)
        for i in idx:
            lists[rows[i]].append((c, vals[i]))
    return lists


def gather_solve(kind, t, x, grouped=None, reverse=False, skip_zero=True):
    """Every output from its gather list: the loops' own order with the
    defaults (asserted below to give the reference's bits), or a wrong one:
    grouped=False in a grouped kind subtracts one product at a time,
    reverse=True takes the entries backwards, skip_zero=False subtracts the
    products of zero values too and divides a zero."""
    sequential = kind in tri_ref.SEQUENTIAL
    grouped = (not sequential) if grouped is None else grouped
    lists = gather_lists(kind, t)
    diag = t.diag.tolist()
    x = list(np.asarray(x, np.float64).tolist())
    first = 0 if kind in (UPPER_T_UP, UPPER) else t.first_non_identity
    top = tri_ref.top_row(kind, t, x)
    order = range(first, top + 1)
    if kind in (UPPER_T, tri_ref.LOWER_T, UPPER):
        order = reversed(order)
    for c in order:
        e = lists[c][::-1] if reverse else lists[c]
        s = x[c]
        i = 0
        if sequential:
            for r, v in e:
                if x[r] != 0.0 or not skip_zero:
                    s -= x[r] * v
            x[c] = s if t.ones or (s == 0.0 and skip_zero) else s / diag[c]
            continue
        if grouped:
            while i + 3 < len(e):
                s -= (e[i][1] * x[e[i][0]] + e[i + 1][1] * x[e[i + 1][0]] +
                      e[i + 2][1] * x[e[i + 2][0]] + e[i + 3][1] * x[e[i + 3][0]])
                i += 4
        for r, v in e[i:]:
            s -= v * x[r]
        x[c] = s if t.ones else s / diag[c]
    return np.array(x, np.float64)


@pytest.mark.parametrize("name", ["entries", "entries_unit"])
@pytest.mark.parametrize("kind", tc.ALL_KINDS)
def test_reference_is_the_exact_solve_rounded(name, kind):
    """Every output within a few ulp of the exact value of its own expression
    on its own (rounded) inputs: k products, k subtractions and one division,
    each rounded once (relative error at most u = 2^-53), so the result is off
    by at most (2k + 1) u times the sum of the magnitudes, to first order;
    3 (k + 1) u covers the higher orders."""
    t = tc.tri_of(name, kind)
    lists = gather_lists(kind, t)
    label, x, start = tc.rhs_list(name, kind)[0]
    ref = tri_ref.solve(kind, t, x, start).tolist()
    first = 0 if kind in (UPPER_T_UP, UPPER) else t.first_non_identity
    u = Fraction(1, 2 ** 53)
    for c in range(first, t.n):
        exact = Fraction(float(x[c]))
        scale = abs(exact)
        for r, v in lists[c]:
            term = Fraction(v) * Fraction(ref[r])
            exact -= term
            scale += abs(term)
        d = Fraction(float(t.diag[c]))
        err = abs(Fraction(ref[c]) - exact / d)
        assert err <= 3 * (len(lists[c]) + 1) * u * scale / abs(d), (name, kind, c, float(err))


# --- conditions on the inputs -----------------------------------------------------------------------

def long_outputs(kind, t):
    return np.array([len(e) > 4 for e in gather_lists(kind, t)])


@pytest.mark.parametrize("name", HOST_CASES)
def test_inputs_can_tell_evaluation_orders_apart(name):
    """Outside the right-hand sides made for it every output is finite and
    non-zero and no division underflows to zero (the one documented deviation
    of the device's gather form, kernels/tri_solve.hip tri_divide); and each
    wrong order, tried alone, changes at least 10 % of the case's outputs of
    more than 4 entries (a floor on the inputs, not a tolerance: the recipe
    measures 25 % and more)."""
    for kind in (UPPER_T, UPPER_T_UP, LOWER, UPPER):
        t = tc.tri_of(name, kind)
        label, x, start = tc.rhs_list(name, kind, full=False)[0]
        assert label == "dense"
        ref = tri_ref.solve(kind, t, x, start)
        assert np.isfinite(ref).all() and (ref != 0.0).all(), (name, kind)
        assert np.isfinite(ref / t.diag).all() and (ref * t.diag != 0).all()
        if name in tc.BIG:
            continue
        same_bits(gather_solve(kind, t, x), ref, f"{name} {kind}: the gather form")
        long_ = long_outputs(kind, t)
        if not long_.any():
            continue
        wrong = {"reversed": {"reverse": True}}
        if kind in tri_ref.GROUPED:
            wrong["one_by_one"] = {"grouped": False}
        for what, how in wrong.items():
            got = gather_solve(kind, t, x, **how)
            changed = (bits(got) != bits(ref))[long_].mean()
            print(f"{name} {tri_ref.KIND_NAMES[kind]} {what}: {100 * changed:.0f} % of "
                  f"{long_.sum()} long outputs change")
            assert changed >= 0.10, (name, kind, what, changed)


@pytest.mark.parametrize("kind", tri_ref.SEQUENTIAL)
@pytest.mark.parametrize("unit", [False, True])
def test_cancellation_case_sees_a_missing_zero_skip(kind, unit):
    t, x, ev = tc.special_tri(kind, "cancellation", unit)
    ref = tri_ref.solve(kind, t, x)
    same_bits(gather_solve(kind, t, x), ref, "the gather form")
    got = gather_solve(kind, t, x, skip_zero=False)
    long_ = long_outputs(kind, t)
    changed = (bits(got) != bits(ref))[long_].mean()
    print(f"{tri_ref.KIND_NAMES[kind]} unit={unit}: {100 * changed:.0f} % change without the skip")
    assert changed >= 0.10
    if not unit:  # the zeros themselves: divided by a negative diagonal they turn -0.0
        assert (bits(got[ev]) != 0).all()


def test_entries_case_covers_every_count_and_place():
    """The `entries` triangles hold every entry count of the cycle with the
    deepest entry first, in the middle and last in evaluation order (from 5
    entries on): the fold stalls in the first group, between groups and in
    the tail."""
    for name in ("entries", "entries_unit"):
        dag = tc.dag_of(name, UPPER_T)
        seen = set()
        for i in range(dag.n):
            s = dag.src[dag.starts[i]:dag.starts[i + 1]]
            k = len(s)
            if k == 0:
                continue
            at = int(np.argmax(dag.level[s]))  # the first entry of the deepest level
            seen.add((k, "first" if at == 0 else "last" if at == k - 1 else "middle"))
        for k in tc.ENTRY_COUNTS:
            assert any(c == k for c, _ in seen), (name, k)
            if k > 4:
                assert {(k, w) for w in ("first", "middle", "last")} <= seen, (name, k, seen)
        assert set(np.diff(dag.starts).tolist()) >= set(tc.ENTRY_COUNTS) | {0}


def test_binding_matches_the_header(tmp_path):
    """tests/devop_tri.py restates mi_devop_tri and the table's length."""
    import ctypes

    import devop_tri
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mi_lp_devop.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(mi_devop_tri), '
                   'offsetof(mi_devop_tri, rows_over), offsetof(mi_devop_tri, entries), '
                   'sizeof(mi_devop_api)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(devop_tri.Tri), devop_tri.Tri.rows_over.offset,
                                     devop_tri.Tri.entries.offset,
                                     ctypes.sizeof(devop_tri.TriApi)]
    devop_tri.api()  # the built library's table is at least that long


def test_expected_plans_of_the_cut_cases():
    """The launch plans the large cases are made for, from the schedule rules
    restated in tri_cases.expected_plan (asserted again on the device)."""
    lv = {"MILP_TRI_SYNCFREE": "0"}
    p = tc.expected_plan(tc.listed_widths("lds_cut_448", UPPER_T), False, lv)
    assert p["plan"] == "levels" and p["cu_run_levels"] == [(0, 36), (36, 40)]
    p = tc.expected_plan(tc.listed_widths("lds_cut_256", UPPER_T), False, lv)
    assert p["cu_run_levels"] == [(0, 64), (64, 65)]
    ch = {"MILP_TRI_CHAIN": "1"}
    p = tc.expected_plan(tc.listed_widths("chain_cut_500", UPPER_T), False, ch)
    assert (p["plan"], p["chain_runs"], p["wide_runs"], p["chain_levels"]) == ("sync_free", 2, 0, 30)
    p = tc.expected_plan(tc.listed_widths("chain_cut_256", UPPER_T), False, ch)
    assert (p["chain_runs"], p["wide_runs"], p["chain_levels"]) == (1, 1, 48)
    p = tc.expected_plan(tc.listed_widths("chain_cut_wide", UPPER_T), False,
                         dict(ch, MILP_TRI_CHAIN_WIDTH="100000"))
    assert (p["chain_runs"], p["wide_runs"], p["max_wide_run"]) == (2, 1, tc.CHAIN_VALS + 1)
    p = tc.expected_plan(tc.listed_widths("syncfree_limit", UPPER_T), False, {})
    assert p["plan"] == "levels" and p["max_wide_run"] > tc.SYNCFREE_MAX and p["fused0"]
    p = tc.expected_plan(tc.listed_widths("syncfree_at_limit", UPPER_T), False, {})
    assert p["plan"] == "sync_free" and p["max_wide_run"] == tc.SYNCFREE_MAX
    p = tc.expected_plan(tc.listed_widths("wide_prefetch", UPPER_T), False,
                         dict(lv, MILP_TRI_WIDE="4000"))
    assert (p["chip_launches"], p["cu_run_levels"]) == (0, [(0, 5)])
    p = tc.expected_plan(tc.listed_widths("wide_prefetch", UPPER_T), False, lv)
    assert (p["chip_launches"], p["cu_run_levels"]) == (4, [(0, 1)])
    p = tc.expected_plan(tc.listed_widths("grid_stride_unit", UPPER_T), True, {})
    assert p["plan"] == "sync_free" and p["work"] == 2000
