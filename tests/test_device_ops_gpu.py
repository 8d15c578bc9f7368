"""Single DeviceLp operations against a plain numpy reference, bit for bit.

The whole-solve parity tests reach only the states a solve's pivots happen to
produce. Here one operation runs on inputs the test chooses (tests/devop.py,
the probe of include/mi_lp_devop.h) at the limits of each kernel, and its
result -- list, values, count, the whole coefficient array -- is compared on
64-bit patterns with tests/device_ref.py, whose arithmetic
tests/test_device_ref_cpu.py checks against exact sums. Every step asserts the
kernel path it was written for (DeviceLp::last_paths).

The cases are the table of tests/device_cases.py; their environment, shape and
asserted path stand there. Every sequence starts with an algorithm-2 row,
which defines every position of the coefficient array whatever the cached
handle computed before.
"""
import functools

import numpy as np
import pytest

import device_cases as dc
import devop
from device_ref import COL_BOXED, COL_CAN_DECREASE, COL_CAN_INCREASE, RefState, bits

pytestmark = pytest.mark.gpu

SWITCHES = ("MILP_SMALL_FUSED", "MILP_ROWWISE_LIST", "MILP_ROWWISE_LIST_MAX_ENTRIES",
            "MILP_DENSE_BLOCK", "MILP_SMALL_THREADS", "MILP_SMALL_SERIAL_ROWS", "MILP_MEDIUM",
            "MILP_FULL_ROWS", "MILP_ROWWISE_CHUNK_MAX_ROWS", "MILP_SMALL_BATCH", "MILP_SHARDS",
            "MILP_DUAL_RATIO_ONE_WG_MAX", "MILP_DUAL_TIGHTEN_MIN", "MILP_DUAL_TIGHTEN_SORT",
            "MILP_TIGHTEN_TARGET")

_matrices = {}


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
    """The cached handles go when this module's tests are done, not at
    interpreter exit."""
    yield
    _cached_handle.cache_clear()
    _matrices.clear()


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A device error is never part of a test here: after one, nothing more
    is started on the GPU."""
    yield
    if devop.device_error is not None:
        pytest.exit(f"device error: {devop.device_error}", returncode=3)


@functools.lru_cache(maxsize=None)
def _cached_handle(mat_id, env, setup):
    mat = _matrices[mat_id]
    d = devop.DevOp(mat.m, mat.n, mat.col_starts, mat.row_idx, mat.vals)
    if "small_batch" in setup:
        d.set_small_batch(True)
    if "no_mirror" in setup:
        d.set_list_mirror(False)
    if "dual_begin" in setup:  # from here on the small launches go out directly
        d.dual_begin(np.zeros(mat.N), np.zeros(mat.N, np.uint8), np.zeros(mat.N))
    return d


def handle(mat, env, setup, monkeypatch):
    """One device handle per (matrix, environment, setup); the MILP_* switches
    are read when it is created."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    _matrices[id(mat)] = mat
    return _cached_handle(id(mat), tuple(sorted(env.items())), tuple(setup))


def same_bits(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(bits(got) != bits(want))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(want)} differ, first at {bad[0]}: "
                           f"device {got[bad[0]]!r} ({got[bad[0]].hex()}) reference "
                           f"{want[bad[0]]!r} ({want[bad[0]].hex()})")


def check_update_row(d, ref, st, what):
    """List, values, count, the coefficient array, ReadCoefficient at three
    unlisted positions; and the path the step was written for."""
    pos, val = d.fetch_update_row()
    p = d.paths()
    print(what, p, "count", len(pos))
    for key, field in (("path", "update_row"), ("compact", "compact"), ("mapped", "list_mapped")):
        want = st.get(key)
        if want is not None:
            assert p[field] in (want if isinstance(want, tuple) else (want,)), (what, key, p)
    assert len(pos) == len(ref.list), (what, len(pos), len(ref.list))
    assert np.array_equal(pos, ref.list), what
    same_bits(val, ref.vals, what + " list values")
    same_bits(d.download_coefficients(), ref.coeff, what + " coefficients")
    unlisted = np.setdiff1d(np.arange(ref.mat.N), ref.list)
    for c in unlisted[[0, len(unlisted) // 2, -1]] if len(unlisted) else []:
        same_bits([d.read_coefficient(c)], [ref.coeff[c]], f"{what} ReadCoefficient({c})")
    if "count" in st:
        assert len(pos) == st["count"], what


def run_case(name, monkeypatch):
    env, _ = dc.CASES[name]
    b = dc.build(name)
    d = handle(b.mat, env, b.setup, monkeypatch)
    ref = RefState(b.mat)
    d.set_mask(b.mask)
    ref.set_relevant(b.mask)
    for i, st in enumerate(b.steps):
        what = f"{name} step {i} ({st['kind']})"
        if st["kind"] == "row":
            if st["mask"] is not None:
                d.set_mask(st["mask"])
                ref.set_relevant(st["mask"])
            assert np.all(np.diff(st["rows"]) > 0)
            d.update_row_row_wise(st["rows"], st["rho"], st["alg"], dc.DROP)
            ref.row_wise(st["rows"], st["rho"], st["alg"], dc.DROP)
            check_update_row(d, ref, st, f"{what} alg {st['alg']} k {len(st['rows'])}")
        elif st["kind"] == "col":
            d.update_row_column_wise(st["rho"], dc.DROP, st["w"])
            ref.column_wise(st["rho"], dc.DROP)
            check_update_row(d, ref, st, what)
        elif st["kind"] == "dots":
            same_bits(d.list_dots_over_update_row(st["v"]), ref.list_dots(ref.list, st["v"]), what)
        else:
            same_bits(d.list_dots(st["cols"], st["v"]), ref.list_dots(st["cols"], st["v"]), what)
    return d, ref


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_update_row_case(name, monkeypatch):
    run_case(name, monkeypatch)


# --- dual device mode -----------------------------------------------------------------------------

# Glop's defaults: 0.5 * 1e-8 and 0.01 * 1e-8.
THRESHOLD, HARRIS, MIN_DELTA = 1e-9, 5e-9, 1e-10


@functools.lru_cache(maxsize=None)
def _dual_matrix():
    """Eight rows of 1024 entries bound a list at 8192; with one slack-only
    row more at 8193 (one past the one-workgroup ratio test)."""
    n, m = 19980, 20
    pool = dc._pool(n, 9000, 201)
    lens = [1023] * 8 + [0] + [50] * (m - 9)
    mat = dc.Matrix(m, n, dc.gen_rows(n, 202, lens, [pool] * m))
    assert mat.entries(range(8)) == 8192 and mat.entries(range(9)) == 8193 and mat.N == 20000
    return mat


def _dual_list(d, ref, rows, density, seed):
    """An algorithm-1 row over `rows` with a random relevant mask."""
    mat = ref.mat
    rows = list(rows)
    mask = np.random.default_rng(seed).random(mat.N) < density
    mask[mat.n + rows[0]] = True
    d.set_mask(mask)
    ref.set_relevant(mask)
    init = list(range(10, 13))
    for f, alg in ((init, 2), (list(rows), 1)):
        rho = dc.rho_for(mat.m, f, seed + alg)
        # The slack of the first row gets a coefficient equal to the ratio
        # test's threshold: listed, but "coeff > threshold" must leave it out.
        rho[rows[0]] = THRESHOLD
        d.update_row_row_wise(f, rho, alg, dc.DROP)
        ref.row_wise(f, rho, alg, dc.DROP)
    check_update_row(d, ref, dict(path="chunk", compact="chip_wide"), f"dual list k {len(rows)}")


def _dual_data(ref, seed, mode, sign):
    """rc, colbits, bound_diff and the variation for the list in `ref`.
    Listed columns get the dual-feasible sign (ratios >= 0).
      few: every boxed column can absorb the variation -> a tight B, few kept
      no_setter: every column boxed with a tiny range -> no B, all eligible kept
      nothing: no column may move
      many: boxed columns of small range and ratio < 1 flip; the few others
            have ratios of 5-10, so B is far and more than 512 are kept
      ties: as many, and the first accepted breakpoint is one of two equal ratios"""
    rng = np.random.default_rng(seed)
    N = ref.mat.N
    rc = rng.uniform(-1.0, 1.0, N)
    signed = ref.vals if sign > 0 else -ref.vals
    rc[ref.list] = -np.sign(signed) * rng.uniform(0.01, 1.0, len(ref.list))
    move = np.array([COL_CAN_DECREASE, COL_CAN_INCREASE, COL_CAN_DECREASE | COL_CAN_INCREASE, 0],
                    np.uint8)
    colbits = move[rng.integers(0, 4, N)]
    bound_diff = rng.uniform(0.5, 1.5, N)
    at_threshold = ref.list[np.abs(ref.vals) == THRESHOLD]
    variation = 1e-3
    if mode == "few":
        colbits |= np.where(rng.random(N) < 0.5, COL_BOXED, 0).astype(np.uint8)
    elif mode == "no_setter":
        colbits |= np.uint8(COL_BOXED)
        bound_diff *= 1e-6
        variation = 1e3
    elif mode == "nothing":
        colbits[:] = 0
    else:
        boxed = rng.random(N) < 0.98
        colbits |= np.where(boxed, COL_BOXED, 0).astype(np.uint8)
        bound_diff *= 1e-2
        variation = 0.05
        free = ~boxed[ref.list]
        rc[ref.list[free]] = (np.sign(rc[ref.list[free]]) * np.abs(ref.vals[free]) *
                              rng.uniform(5.0, 10.0, int(free.sum())))
        if mode == "ties":
            # Five boxed breakpoints ahead of all others (those have ratios >=
            # 0.01): ratios 2^-14, 2^-13, 2^-12 flip, and two of exactly 2^-11
            # share what is left of the variation: the accepted one is a tie.
            near = np.nonzero(boxed[ref.list] & (np.abs(ref.vals) > 0.1) &
                              ((colbits[ref.list] & 3) == 3))[0][:5]
            assert len(near) == 5
            mag = np.abs(ref.vals[near])
            ratio = np.array([2.0 ** -14, 2.0 ** -13, 2.0 ** -12, 2.0 ** -11, 2.0 ** -11])
            rc[ref.list[near]] = -np.sign(signed[near]) * (mag * ratio)
            bound_diff[ref.list[near]] = 0.05 / mag  # each absorbs about 0.05
            delta = bound_diff[ref.list[near]] * mag
            variation = float(delta[:3].sum() + 0.5 * delta[3:].min())
    if mode != "nothing":
        # Free to move and with the smallest ratio of all, were it eligible.
        colbits[at_threshold] = COL_CAN_DECREASE | COL_CAN_INCREASE
        rc[at_threshold] = 0.0
    return rc, colbits, bound_diff, variation


def _ratio(d, ref, sign, variation):
    col, coeff, rc, list_count = d.dual_ratio_candidates(sign, THRESHOLD, HARRIS, MIN_DELTA,
                                                         variation)
    B, kept, popped, _ = ref.dual_ratio(sign, THRESHOLD, HARRIS, MIN_DELTA, variation)
    p = d.paths()
    print("ratio", p, "B", B, "kept", len(kept), "popped", len(popped), "returned", len(col),
          "list", len(ref.list))
    assert list_count == len(ref.list)
    return col, coeff, rc, kept, popped, p


EXACT = [("8192", {}, 8, "one_workgroup"),
         ("8193", {}, 9, "two_kernels"),
         ("8192_one_wg_off", {"MILP_DUAL_RATIO_ONE_WG_MAX": "0"}, 8, "two_kernels")]


@pytest.mark.parametrize("mode,density", [("few", 0.7), ("no_setter", 0.05), ("nothing", 0.7)])
@pytest.mark.parametrize("label,env,k,path", EXACT, ids=[e[0] for e in EXACT])
def test_dual_ratio_candidates_exact(label, env, k, path, mode, density, monkeypatch):
    """Without the tightening round (at most 512 kept) the candidates are the
    reference's kept set, in list order: column, coefficient and rc bits, and
    the list count. List bounds 8192 (one workgroup) and 8193 (two kernels)."""
    mat = _dual_matrix()
    d = handle(mat, dict(dc.OFF, **env), (), monkeypatch)
    ref = RefState(mat)
    _dual_list(d, ref, range(k), density, 300 + k)
    for sign in (1.0, -1.0):
        rc, colbits, bound_diff, variation = _dual_data(ref, 310 + k, mode, sign)
        d.dual_begin(rc, colbits, bound_diff)
        ref.dual_begin(rc, colbits, bound_diff)
        col, coeff, rcs, kept, _, p = _ratio(d, ref, sign, variation)
        assert len(kept) <= 512 and p["ratio"] == path and not p["ratio_tightened"], p
        assert np.count_nonzero(np.abs(ref.vals) == THRESHOLD) == 1
        if mode == "few":
            assert 0 < len(kept) < len(ref.list)
        elif mode == "no_setter":
            assert len(kept) > 50
        else:
            assert len(kept) == 0
        assert np.array_equal(col, ref.list[kept])
        same_bits(coeff, ref.vals[kept], "candidate coefficients")
        same_bits(rcs, ref.rc[ref.list[kept]], "candidate reduced costs")
    # Column bits changed in place (a third of the list may no longer move).
    rc, colbits, bound_diff, variation = _dual_data(ref, 320 + k, mode, 1.0)
    d.dual_begin(rc, colbits, bound_diff)
    ref.dual_begin(rc, colbits, bound_diff)
    cols = ref.list[::3]
    d.dual_set_col_bits(cols, np.zeros(len(cols), np.uint8))
    ref.dual_set_col_bits(cols, np.zeros(len(cols), np.uint8))
    col, coeff, rcs, kept, _, p = _ratio(d, ref, 1.0, variation)
    assert len(kept) <= 512 and not p["ratio_tightened"]
    assert not set(ref.list[kept].tolist()) & set(cols.tolist())
    assert np.array_equal(col, ref.list[kept])
    same_bits(coeff, ref.vals[kept], "candidate coefficients")
    same_bits(rcs, ref.rc[ref.list[kept]], "candidate reduced costs")


TIGHTEN = [({"MILP_DUAL_TIGHTEN_MIN": "0", "MILP_TIGHTEN_TARGET": "1"}, "min0_target1"),
           ({"MILP_DUAL_TIGHTEN_MIN": "0", "MILP_TIGHTEN_TARGET": "3"}, "min0_target3"),
           ({"MILP_DUAL_TIGHTEN_MIN": "0"}, "min0"),
           ({}, "default"),
           ({"MILP_DUAL_TIGHTEN_MIN": "0", "MILP_DUAL_TIGHTEN_SORT": "1"}, "min0_sort"),
           ({"MILP_DUAL_TIGHTEN_SORT": "1"}, "sort")]


@pytest.mark.parametrize("mode", ["many", "ties"])
@pytest.mark.parametrize("k,path", [(8, "one_workgroup"), (9, "two_kernels")])
@pytest.mark.parametrize("env,label", TIGHTEN, ids=[t[1] for t in TIGHTEN])
def test_dual_ratio_candidates_tightened(env, label, k, path, mode, monkeypatch):
    """With the tightening round the bound may be anything between the walk's
    result and B: P (what Glop's second loop pops) is within the returned
    set, which is within the set kept under B; list order, gathered values
    bit-equal."""
    mat = _dual_matrix()
    d = handle(mat, dict(dc.OFF, **env), (), monkeypatch)
    ref = RefState(mat)
    _dual_list(d, ref, range(k), 0.7, 400 + k)
    for sign in (1.0, -1.0):
        rc, colbits, bound_diff, variation = _dual_data(ref, 410 + k, mode, sign)
        d.dual_begin(rc, colbits, bound_diff)
        ref.dual_begin(rc, colbits, bound_diff)
        col, coeff, rcs, kept, popped, p = _ratio(d, ref, sign, variation)
        assert len(kept) > 512 and p["ratio"] == path and p["ratio_tightened"], p
        slot_of = {int(c): s for s, c in enumerate(ref.list)}
        slots = np.array([slot_of[int(c)] for c in col], np.int64)
        assert np.all(np.diff(slots) > 0), "list order"
        assert set(popped.tolist()) <= set(slots.tolist()) <= set(kept.tolist())
        assert len(popped) > 1
        same_bits(coeff, ref.vals[slots], "candidate coefficients")
        same_bits(rcs, ref.rc[ref.list[slots]], "candidate reduced costs")


@pytest.mark.parametrize("count", [0, 255, 256, 257])
def test_dual_update_reduced_costs(count, monkeypatch):
    """Launched at the list's bound (N here), far above the count. The
    entering column is listed; with mult = 1e-310 every mult * coeff is
    subnormal or underflows. All N reduced costs, bit for bit."""
    name = "compact_N16385"
    b = dc.build(name)
    mat = b.mat
    d = handle(mat, dc.CASES[name][0], b.setup, monkeypatch)
    ref = RefState(mat)
    rng = np.random.default_rng(500 + count)
    mask = np.zeros(mat.N, bool)
    mask[rng.choice(mat.n, count, replace=False)] = True
    d.set_mask(mask)
    ref.set_relevant(mask)
    st = b.steps[0]
    d.update_row_row_wise(st["rows"], st["rho"], 2, dc.DROP)
    ref.row_wise(st["rows"], st["rho"], 2, dc.DROP)
    check_update_row(d, ref, dict(path="full_rows", compact="chip_wide", count=count), "rc list")
    rc = rng.uniform(-1.0, 1.0, mat.N)
    rc[rng.random(mat.N) < 0.3] = 0.0
    zeros = np.zeros(mat.N)
    d.dual_begin(rc, zeros.astype(np.uint8), zeros)
    ref.dual_begin(rc, zeros.astype(np.uint8), zeros)
    leaving = mat.N - 2
    entering = int(ref.list[count // 2]) if count else 7
    for mult in (0.75, -1e-310):
        d.dual_update_reduced_costs(mult, leaving, 0.125 * mult, entering)
        ref.update_reduced_costs(mult, leaving, 0.125 * mult, entering)
        same_bits(d.dual_download_reduced_costs(), ref.rc, f"rc after mult {mult}")
    assert ref.rc[entering] == 0.0 and ref.rc[leaving] == 0.125 * -1e-310


def test_dual_on_a_list_kernel_row(monkeypatch):
    """The ratio test and the reduced-cost update on a list the list kernel
    left (bound = the rows' entries, no flags), then FlagsFromList's consumer
    is not needed: both read the list alone."""
    d, ref = run_case("list_k64", monkeypatch)
    assert d.paths()["update_row"] == "list"
    rc, colbits, bound_diff, variation = _dual_data(ref, 600, "few", 1.0)
    d.dual_begin(rc, colbits, bound_diff)
    ref.dual_begin(rc, colbits, bound_diff)
    col, coeff, rcs, kept, _, p = _ratio(d, ref, 1.0, variation)
    assert p["ratio"] == "one_workgroup" and not p["ratio_tightened"] and 0 < len(kept) <= 512
    assert np.array_equal(col, ref.list[kept])
    same_bits(coeff, ref.vals[kept], "candidate coefficients")
    same_bits(rcs, ref.rc[ref.list[kept]], "candidate reduced costs")
    entering = int(col[0])
    d.dual_update_reduced_costs(-0.5, ref.mat.N - 1, 0.25, entering)
    ref.update_reduced_costs(-0.5, ref.mat.N - 1, 0.25, entering)
    same_bits(d.dual_download_reduced_costs(), ref.rc, "rc after the update")
