"""The device triangular solves (engine/device_solve.hip, kernels/
tri_solve.hip), one solve at a time through the probe (tests/devop_tri.py),
bit for bit against tests/tri_ref.py and against the host loop on the same
matrix (tri_host_solve). Every comparison is on all 64 bits, NaNs included,
with the one exception of tests/test_solveops_gpu.py's same_rc: the sign of a
NaN that arithmetic made (gfx950 subtracts by adding a negated source, which
hands a NaN on with its sign flipped); a NaN that only passes through is
compared whole.

A whole solve sees the triangles its own pivots make. Here they are those of
tests/tri_cases.py, built for the limits of each plan: every entry count
around the groups of four and the windows of 8 with the deepest entry first,
middle and last; level widths around the wave, the workgroup and the
prefetch; runs cut at the LDS stores of the single-CU and the chain kernel;
the sync-free plan's size limit; grids past their caps; identity prefixes.
tests/test_tri_ref_cpu.py checks the reference against the host loops and
exact arithmetic and shows that the inputs tell evaluation orders apart.
Every solve asserts what it went through (DeviceLp::LastTri): the plan, the
level widths, the launches and cuts, and the top row.
"""
import functools
import itertools

import numpy as np
import pytest

import devop
import devop_tri
import tri_cases as tc
import tri_ref
from tri_ref import LOWER, UPPER, UPPER_T, UPPER_T_UP, bits

pytestmark = pytest.mark.gpu

SWITCHES = ("MILP_DEVICE_SOLVE", "MILP_DEVICE_SOLVE_MIN_ROWS", "MILP_TRI_WIDE", "MILP_TRI_GRAPH",
            "MILP_TRI_TAU", "MILP_TRI_MAPPED", "MILP_TRI_SYNCFREE", "MILP_TRI_LOWER",
            "MILP_TRI_BTRAN", "MILP_TRI_PAIR", "MILP_SPEC_FLIP", "MILP_TRI_PAD",
            "MILP_DENSE_TAIL", "MILP_DENSE_TAIL_MIN_ENTRIES", "MILP_DENSE_TAIL_MIN_COLS",
            "MILP_TRI_MIN_WIDTH", "MILP_TRI_CHAIN", "MILP_TRI_CHAIN_WIDTH",
            "MILP_TRI_CHAIN_MIN_LEVELS", "MILP_TRI_SYNCFREE_MIN_LEVELS", "MILP_TRI_FUSE0",
            "MILP_TRI_POLL_MAX", "MILP_TRI_PERSIST", "MILP_TRI_XCD", "MILP_TRI_DEBUG",
            "MILP_TRI_SCHED", "MILP_SHARDS", "MILP_SMALL_BATCH")
BASE = {"MILP_DEVICE_SOLVE": "force", "MILP_TRI_BTRAN": "1"}
LEVELS = {"MILP_TRI_SYNCFREE": "0"}
CHAIN = {"MILP_TRI_CHAIN": "1"}
# The plans of VARIANTS in tests/test_device_solve_gpu.py (the persistent ones
# at those values, no larger), and MILP_TRI_FUSE0 / MILP_TRI_WIDE.
VARIANTS = {
    "syncfree": {},
    "levels": LEVELS,
    "levels_copies": dict(LEVELS, MILP_TRI_MAPPED="0"),
    "syncfree_copies": {"MILP_TRI_MAPPED": "0"},
    "persistent_xcd": {"MILP_TRI_PERSIST": "32", "MILP_TRI_XCD": "1", "MILP_TRI_POLL_MAX": "8"},
    "persistent_chip": {"MILP_TRI_PERSIST": "64", "MILP_TRI_POLL_MAX": "4"},
    "chain": CHAIN,
    "wide_chain": dict(CHAIN, MILP_TRI_CHAIN_WIDTH="100000", MILP_TRI_CHAIN_MIN_LEVELS="1"),
    "padded": {"MILP_TRI_PAD": "1"},
    "syncfree_no_fuse0": {"MILP_TRI_FUSE0": "0"},
    "levels_no_fuse0": dict(LEVELS, MILP_TRI_FUSE0="0"),
    "levels_wide_64": dict(LEVELS, MILP_TRI_WIDE="64"),
    "levels_wide_4000": dict(LEVELS, MILP_TRI_WIDE="4000"),
    "persistent_no_fuse0": {"MILP_TRI_PERSIST": "64", "MILP_TRI_POLL_MAX": "4",
                            "MILP_TRI_FUSE0": "0"},
}
SMALL_RUNS = ([(n, v) for n in ("entries", "entries_unit", "widths", "widths_unit")
               for v in VARIANTS] +
              [(f"identity_prefix_{p}{u}", v) for p in tc.PREFIXES for u in ("", "_unit")
               for v in ("syncfree", "levels", "wide_chain", "padded")])
# The large cases, on the plans they are made for.
BIG_RUNS = [
    ("wide_prefetch", dict(LEVELS, MILP_TRI_WIDE="4000")),  # the loop past the prefetch
    ("wide_prefetch", LEVELS),                              # the same levels chip-wide
    ("lds_cut_448", LEVELS),
    ("lds_cut_256", LEVELS),
    ("chain_cut_500", CHAIN),
    ("chain_cut_256", CHAIN),
    ("chain_cut_wide", dict(CHAIN, MILP_TRI_CHAIN_WIDTH="100000")),
    ("syncfree_limit", {}),
    ("syncfree_at_limit", {}),
    ("grid_stride", LEVELS),
    ("grid_stride", dict(LEVELS, MILP_TRI_FUSE0="0")),
    ("grid_stride", dict(LEVELS, MILP_TRI_MAPPED="0")),
    ("grid_stride_unit", {}),
    ("grid_stride_unit", {"MILP_TRI_MAPPED": "0"}),
]


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
    """The cached handles go when this module's tests are done, not at
    interpreter exit."""
    yield
    _cached_handle.cache_clear()


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A device error (a stall reported by the bounded waits included) is
    never part of a test here: after one, nothing more is started on the
    GPU."""
    yield
    if devop.device_error is not None:
        pytest.exit(f"device error: {devop.device_error}", returncode=3)


@functools.lru_cache(maxsize=None)
def _cached_handle(name, env):
    return devop_tri.TriDevOp()


def handle(name, env, monkeypatch, cached=True):
    """One device handle per (case, environment); the MILP_* switches are read
    when it is created. Returns (handle, the full environment)."""
    env = dict(BASE, **env)
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    make = _cached_handle if cached else _cached_handle.__wrapped__
    return make(name, tuple(sorted(env.items()))), env


_keys = itertools.count(1000)


def new_key():
    return next(_keys)


def same_bits(got, want, what, nan_sign_open=None):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = bits(got).copy(), bits(want).copy()
    if nan_sign_open is not None:
        for a, p in ((got, g), (want, w)):
            sel = nan_sign_open & np.isnan(a)
            p[sel] &= np.uint64(0x7FFFFFFFFFFFFFFF)
    bad = np.nonzero(g != w)[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(want)} differ, first at {bad[0]}: "
                           f"device {got[bad[0]]!r} ({int(bits(got)[bad[0]]):#018x}) reference "
                           f"{want[bad[0]]!r} ({int(bits(want)[bad[0]]):#018x})")


def reference(kind, t, x, start=0):
    """(the reference's result, where a NaN's sign is left open: the NaNs that
    the loop's arithmetic wrote)."""
    touched = [False] * t.n
    ref = tri_ref.solve(kind, t, x, start, touched)
    return ref, np.isnan(ref) & np.array(touched)


@functools.lru_cache(maxsize=None)
def case_reference(name, kind, full):
    t = tc.tri_of(name, kind)
    return [(label, x, start) + reference(kind, t, x, start)
            for label, x, start in tc.rhs_list(name, kind, full)]


def shape_of(kind, t):
    """What the schedule of (kind, t) lists: first output, listed rows, entry
    counts of the listed outputs."""
    first = 0 if kind in (UPPER_T_UP, UPPER) else t.first_non_identity
    if kind in tri_ref.GROUPED:
        counts = np.diff(t.starts)
    else:
        counts = np.bincount(t.rows, minlength=t.n)
    listed = (counts > 0) | (not t.ones)
    listed[:first] = False
    return first, listed, counts


def check_record(rec, widths_got, kind, t, x, widths, unit, env, what, vectors=1):
    """last_tri after a solve of x that went to the device."""
    first, listed, counts = shape_of(kind, t)
    top = tri_ref.top_row(kind, t, x)
    want = tc.expected_plan(widths, unit, env)
    trivial = not listed[first:top + 1].any()
    print(what, rec)
    assert rec["plan"] == ("trivial" if trivial else want["plan"]), (what, rec)
    assert rec["kind"] == devop_tri.KINDS[kind] and rec["rows"] == t.n, (what, rec)
    assert rec["first_col"] == first and rec["top"] == top, (what, rec, first, top)
    assert widths_got == list(widths), (what, widths_got)
    for f in ("work", "levels", "chain_levels", "level0_end", "max_wide_run"):
        assert rec[f] == want[f], (what, f, rec, want)
    assert rec["pos"] == want["work"] + (t.n - first) - int(listed.sum()), (what, rec)
    lc = counts[listed]
    assert rec["max_entries"] == (int(lc.max()) if len(lc) else 0), (what, rec)
    assert rec["rows_over"] == [int((lc > k).sum()) for k in (4, 16, 64)], (what, rec)
    if trivial:
        return
    assert rec["vectors"] == vectors, (what, rec)
    for f in ("wide_runs", "chain_runs", "chip_launches", "cu_runs", "fused0"):
        assert rec[f] == want[f], (what, f, rec, want)


def run_case(d, name, kind, env, full):
    t = tc.tri_of(name, kind)
    d.tri_set_matrix(t)
    key = new_key()
    widths = tc.listed_widths(name, kind)
    unit = tc.SPECS[name]["unit"]
    for label, x, start, ref, open_ in case_reference(name, kind, full):
        what = f"{name} {tri_ref.KIND_NAMES[kind]} {label}"
        on, got = d.tri_solve(kind, key, x, start)
        rec, widths_got = d.last_tri(), d.last_tri_level_widths()
        assert on, (what, rec)
        same_bits(got, ref, what, open_)
        same_bits(d.tri_host_solve(kind, x, start), ref, what + " (host loop)")
        check_record(rec, widths_got, kind, t, x, widths, unit, env, what)


@pytest.mark.parametrize("name,variant", SMALL_RUNS)
def test_every_kind_and_right_hand_side(name, variant, monkeypatch):
    """Every kind and every right-hand side of tri_cases.rhs_list under one
    key per kind (the second and later vectors find the pending marks and the
    staging of the one before)."""
    d, env = handle(name, VARIANTS[variant], monkeypatch)
    for kind in tc.ALL_KINDS:
        run_case(d, name, kind, env, full=True)


@pytest.mark.parametrize("kind", tc.ALL_KINDS, ids=tri_ref.KIND_NAMES)
@pytest.mark.parametrize("name,env", BIG_RUNS,
                         ids=[n + "-" + "-".join(f"{k[9:]}={v}" for k, v in sorted(e.items()))
                              for n, e in BIG_RUNS])
def test_plans_at_their_limits(name, env, kind, monkeypatch):
    """The large cases on the plan each is made for; expected_plan says where
    the runs are cut and how many launches of each kind there are, and
    tests/test_tri_ref_cpu.py pins those expectations themselves."""
    d, env = handle(name, env, monkeypatch)
    run_case(d, name, kind, env, full=False)


@pytest.mark.parametrize("variant", ["syncfree", "levels", "wide_chain", "persistent_chip"])
@pytest.mark.parametrize("unit", [False, True], ids=["diag", "unit"])
def test_planted_events(variant, unit, monkeypatch):
    """An infinite coefficient on a zero value (NaN in a grouped sum, skipped
    by a scatter loop), and for the scatter loops exact cancellation: the zero
    is neither divided nor scattered, though its column holds infinities."""
    d, env = handle("planted", VARIANTS[variant], monkeypatch)
    for kind in tc.ALL_KINDS:
        for which in ("inf_meets_zero", "cancellation"):
            if which == "cancellation" and kind not in tri_ref.SEQUENTIAL:
                continue
            t, x, ev = tc.special_tri(kind, which, unit)
            what = f"{which} {tri_ref.KIND_NAMES[kind]} unit={unit}"
            ref, open_ = reference(kind, t, x)
            d.tri_set_matrix(t)
            on, got = d.tri_solve(kind, new_key(), x)
            assert on, what
            same_bits(got, ref, what, open_)
            same_bits(d.tri_host_solve(kind, x), ref, what + " (host loop)")
            if which == "cancellation":
                assert (bits(got[ev]) == 0).all() and np.isfinite(got).all(), what
            else:
                assert np.isnan(got).any() == (kind in tri_ref.GROUPED), what


# --- state ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["syncfree", "levels", "wide_chain"])
def test_key_changes_between_matrices_of_other_sizes(variant, monkeypatch):
    """Key 1 on A, key 2 on a larger B, key 3 on a smaller C, A again under
    key 4: schedules, positions and staging are rebuilt and resized."""
    d, env = handle("keys", VARIANTS[variant], monkeypatch)
    for kind in (UPPER_T, LOWER, UPPER_T_UP):
        for name in ("entries", "widths", "identity_prefix_1", "entries"):
            run_case(d, name, kind, env, full=False)


# --- pair -----------------------------------------------------------------------------------------

def pair_vectors(name):
    t = tc.tri_of(name, UPPER_T)
    rng = np.random.default_rng(5)
    x0, x1 = tc.dense_rhs(rng, t.n), tc.dense_rhs(rng, t.n)
    x1[t.n - t.n // 3:] = 0.0  # another top row
    return t, x0, x1


@pytest.mark.parametrize("name", ["entries", "entries_unit", "widths"])
def test_pair_is_two_single_solves(name, monkeypatch):
    d, env = handle(name, {}, monkeypatch)
    t, x0, x1 = pair_vectors(name)
    d.tri_set_matrix(t)
    key = new_key()
    for a, b in ((x0, x1), (x1, x0)):
        on, g0, g1 = d.tri_solve_pair(UPPER_T, key, a, b)
        rec, widths_got = d.last_tri(), d.last_tri_level_widths()
        assert on, rec
        check_record(rec, widths_got, UPPER_T, t, a, tc.listed_widths(name, UPPER_T),
                     tc.SPECS[name]["unit"], env, f"pair {name}", vectors=2)
        for x, g in ((a, g0), (b, g1)):
            ref, open_ = reference(UPPER_T, t, x)
            same_bits(g, ref, f"pair {name}", open_)
            on1, single = d.tri_solve(UPPER_T, key, x)
            assert on1
            same_bits(single, g, f"pair {name} against a single solve")


def test_pair_with_a_trivial_vector_is_refused(monkeypatch):
    d, env = handle("entries", {}, monkeypatch)
    t, x0, _ = pair_vectors("entries")
    d.tri_set_matrix(t)
    zero = np.zeros(t.n)
    zero[:t.first_non_identity] = 1.0
    for a, b in ((x0, zero), (zero, x0)):
        on, g0, g1 = d.tri_solve_pair(UPPER_T, new_key(), a, b)
        assert not on and d.last_tri()["plan"] == "none"
        same_bits(g0, a, "untouched")
        same_bits(g1, b, "untouched")


@pytest.mark.parametrize("variant,more", [("levels", {}), ("syncfree", {"MILP_TRI_PAIR": "0"}),
                                          ("persistent_chip", {})])
def test_pair_is_refused_off_the_sync_free_plan(variant, more, monkeypatch):
    d, env = handle("entries", dict(VARIANTS[variant], **more), monkeypatch)
    t, x0, x1 = pair_vectors("entries")
    d.tri_set_matrix(t)
    on, g0, g1 = d.tri_solve_pair(UPPER_T, new_key(), x0, x1)
    assert not on and d.last_tri()["plan"] == "none"
    same_bits(g0, x0, "untouched")
    same_bits(g1, x1, "untouched")
    on, g0, g1 = d.tri_solve_pair(LOWER, new_key(), x0, x1)  # only the U solve pairs
    assert not on


# --- the asynchronous U solve -----------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["syncfree", "levels", "chain"])
def test_async_u_solve(variant, monkeypatch):
    d, env = handle("widths", VARIANTS[variant], monkeypatch)
    name = "widths"
    t, x0, x1 = pair_vectors(name)
    d.tri_set_matrix(t)
    ref0, open0 = reference(UPPER_T, t, x0)
    ref1, open1 = reference(UPPER_T, t, x1)
    refl, openl = reference(LOWER, t, x1)
    widths, unit = tc.listed_widths(name, UPPER_T), tc.SPECS[name]["unit"]
    # Begin, an L solve on the same handle in between, finish.
    key = new_key()
    assert d.tri_async_begin(key, x0)
    check_record(d.last_tri(), d.last_tri_level_widths(), UPPER_T, t, x0, widths, unit, env,
                 "async begin")
    on, got = d.tri_solve(LOWER, new_key(), x1)
    assert on
    same_bits(got, refl, "the L solve in between", openl)
    same_bits(d.tri_async_finish(x0), ref0, "async finish", open0)
    # Begin, drop: nothing comes back; the next solve is not disturbed.
    assert d.tri_async_begin(key, x1)
    d.tri_async_drop()
    on, got = d.tri_solve(UPPER_T, key, x0)
    assert on
    same_bits(got, ref0, "after a drop", open0)
    # Begin under key k, a solve that rebuilds the U schedule under key k + 1,
    # finish: the result is that of key k's vector.
    assert d.tri_async_begin(key, x1)
    on, got = d.tri_solve(UPPER_T, new_key(), x0)
    assert on
    same_bits(got, ref0, "the solve that rebuilt the schedule", open0)
    same_bits(d.tri_async_finish(x1), ref1, "async finish after a rebuild", open1)
    # A trivial vector: started, nothing launched, finish leaves x alone.
    zero = np.zeros(t.n)
    assert d.tri_async_begin(key, zero)
    assert d.last_tri()["plan"] == "trivial"
    same_bits(d.tri_async_finish(zero), zero, "trivial async")


def test_async_finish_without_begin_is_an_error_of_the_call(monkeypatch):
    """Not a device error: the handle goes on working."""
    d, env = handle("entries", {}, monkeypatch, cached=False)
    t, x0, _ = pair_vectors("entries")
    d.tri_set_matrix(t)
    with pytest.raises(devop.DevOpError, match="none in flight"):
        d.tri_async_finish(x0)
    devop.device_error = None
    on, got = d.tri_solve(UPPER_T, new_key(), x0)
    assert on
    same_bits(got, reference(UPPER_T, t, x0)[0], "after the refused finish")
    d.close()


def test_probe_checks_its_matrix(monkeypatch):
    d, env = handle("entries", {}, monkeypatch, cached=False)
    t = tc.tri_of("small", UPPER_T)
    bad_rows = t.rows.copy()
    bad_rows[3] = t.n
    bad_starts = t.starts.copy()
    bad_starts[2] = bad_starts[3] + 1
    for starts, rows in ((t.starts, bad_rows), (bad_starts, t.rows)):
        class M:
            n, diag, vals = t.n, t.diag, t.vals
        M.starts, M.rows = starts, rows
        with pytest.raises(devop.DevOpError, match="tri_set_matrix"):
            d.tri_set_matrix(M)
    devop.device_error = None
    d.close()
