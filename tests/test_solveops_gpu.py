"""DeviceLp's pricing, row sums, column norms, boxed flips and reduced-cost
copies, one operation at a time through the probe (tests/devop_solveops.py),
bit for bit against tests/device_ref.py. Every comparison is on all 64 bits,
NaNs included, with one exception (same_rc): the sign of a NaN reduced cost
c - dot whose dot is NaN.

A whole solve reaches only the states its own pivots produce. Here the inputs
are those of tests/solveops_cases.py, at the limits of each kernel: the
unrolled loop of the dense block and its hand-offs, row sums over padded
chunks and a partial workgroup, fused pricing on stale and on fresh flags,
every way the early boxed-flip launch can be out of date, the kBasic mask
changed in three words and in every word of more than 512. tests/test_solveops_ref_cpu.py checks the
reference against exact sums and shows that the inputs tell summation orders
apart. Every pricing step asserts the kernels it went through
(DeviceLp::last_column_dots), every flips step whether the early launch was
taken (DeviceLp::last_flips).

Sequences that need an update row start with an algorithm-2 row, which defines
every position of the coefficient array whatever the cached handle held.
"""
import functools

import numpy as np
import pytest

import devop
import devop_solveops
import solveops_cases as sc
from device_ref import STATUS_AT_LOWER, STATUS_AT_UPPER, STATUS_SHIFT, COL_BOXED, RefState, bits

pytestmark = pytest.mark.gpu

SWITCHES = ("MILP_SMALL_FUSED", "MILP_ROWWISE_LIST", "MILP_ROWWISE_LIST_MAX_ENTRIES",
            "MILP_DENSE_BLOCK", "MILP_SMALL_THREADS", "MILP_SMALL_SERIAL_ROWS", "MILP_MEDIUM",
            "MILP_FULL_ROWS", "MILP_ROWWISE_CHUNK_MAX_ROWS", "MILP_SMALL_BATCH", "MILP_SHARDS",
            "MILP_DENSE_UNROLL", "MILP_EARLY_FLIPS", "MILP_SHARD_DEVICES")
DROP = sc.DROP
SHARDS = {"MILP_SHARDS": "2"}


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
    """The cached handles go when this module's tests are done, not at
    interpreter exit."""
    yield
    _cached_handle.cache_clear()


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A device error is never part of a test here: after one, nothing more
    is started on the GPU."""
    yield
    if devop.device_error is not None:
        pytest.exit(f"device error: {devop.device_error}", returncode=3)


@functools.lru_cache(maxsize=None)
def _cached_handle(name, env):
    mat = sc.matrix(name)
    return devop_solveops.SolveDevOp(mat.m, mat.n, mat.col_starts, mat.row_idx, mat.vals)


def handle(name, env, monkeypatch, cached=True):
    """One device handle per (matrix, environment); the MILP_* switches are
    read when it is created."""
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    make = _cached_handle if cached else _cached_handle.__wrapped__
    return make(name, tuple(sorted(env.items())))


def same_bits(got, want, what, nan_sign_open=None):
    """All 64 bits of every value, NaNs included. nan_sign_open: positions at
    which the sign bit of a NaN (and of nothing else) is left out; same_rc is
    its only user."""
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


def same_rc(got, ref, what):
    """The reduced costs of a pricing call against ref.priced (RefState after
    its own pricing call), on all bits, with the one exception of this file:
    where the reference's dot is NaN, the sign of the NaN rc = c - dot is not
    compared. IEEE 754 leaves the sign of a NaN result open, and here it is not
    the kernel source's to decide: gfx950 has no double subtraction, so c - dot
    is an add with a negated source, which hands on a NaN dot with its sign
    flipped (0xfff8... where x86's subtraction keeps 0x7ff8...). Payload and
    position are still compared, and a NaN that comes from c alone is compared
    whole."""
    same_bits(got, ref.priced, what, nan_sign_open=np.isnan(ref.priced_dots))


def unroll_of(name):
    m = int(name[5:])
    return next((u for u, ms in sc.DENSE_UNROLL_ROWS.items() if m in ms), 8)


def dense_env(name, **more):
    env = dict(sc.environment(name), **more)
    if name.startswith("dense") and unroll_of(name) != 8:
        env["MILP_DENSE_UNROLL"] = str(unroll_of(name))
    return env


def expected_dots(name, env, mode):
    dense = env.get("MILP_DENSE_BLOCK") == "force"
    return {"mode": mode, "wave_per_col": name == "wave", "dense": dense,
            "dense_unroll": int(env.get("MILP_DENSE_UNROLL", "8")) if dense else 0}


# --- pricing --------------------------------------------------------------------------------------

def check_pricing(d, name, env, c, y, what):
    ref = RefState(sc.matrix(name))
    got = d.pricing(c, y)
    p = d.last_column_dots()
    print(what, p)
    ref.pricing(c, y)
    same_rc(got, ref, what)
    assert p == expected_dots(name, env, "pricing"), (what, p)
    return got


@pytest.mark.parametrize("name", ["quad", "wave"])
def test_pricing_sparse(name, monkeypatch):
    """The short-column and the long-column kernel; c holds both zeros, an inf
    and a NaN; then a NaN and an inf in y."""
    p = sc.pricing_inputs(name)
    d = handle(name, {}, monkeypatch)
    check_pricing(d, name, {}, p["c"], p["y"], f"{name} pricing")
    check_pricing(d, name, {}, p["c"], p["w"], f"{name} pricing, second vector")
    check_pricing(d, name, {}, p["c"], p["y_special"], f"{name} pricing, NaN and inf in y")


@pytest.mark.parametrize("name", [f"dense{m}" for m in sc.OLD_DENSE + sc.NEW_DENSE])
def test_pricing_dense_block(name, monkeypatch):
    """Rows below the unrolled loop (unroll 8), and at pairs == U, U + 1 (odd
    step, three tail rows) and 2 U - 1 for U = 8, 16, 32."""
    env = dense_env(name)
    p = sc.pricing_inputs(name)
    d = handle(name, env, monkeypatch)
    m, u = sc.matrix(name).m, unroll_of(name)
    assert ((m >> 3) >= u) == (m in sc.NEW_DENSE)
    check_pricing(d, name, env, p["c"], p["y"], f"{name} U={u} pricing")
    check_pricing(d, name, env, p["c"], p["w"], f"{name} U={u} pricing, second vector")
    check_pricing(d, name, env, p["c"], p["y_special"], f"{name} U={u} pricing, NaN and inf in y")


def check_list(d, ref, what, path=None):
    pos, val = d.fetch_update_row()
    assert np.array_equal(pos, ref.list), what
    same_bits(val, ref.vals, what + " list values")
    if path is not None:
        assert d.paths()["update_row"] in path, (what, d.paths())


def check_fused(d, ref, name, env, p, what):
    rc, dots = d.pricing(p["c"], p["y"], p["w"])
    rec = d.last_column_dots()
    want_rc, want_dots = ref.pricing_with_dots(p["c"], p["y"], p["w"])
    print(what, rec, "list", len(ref.list))
    assert len(dots) == len(ref.list), (what, len(dots), len(ref.list))
    same_rc(rc, ref, what + " rc")
    same_bits(dots, want_dots, what + " list dots")
    assert rec == expected_dots(name, env, "pricing_with_dots"), (what, rec)


FUSED = [("quad", sc.OFF), ("quad", {}), ("wave", sc.OFF), ("dense64", sc.OFF)]


@pytest.mark.parametrize("name,base", FUSED, ids=[f"{n}-{'general' if b else 'small'}"
                                                   for n, b in FUSED])
def test_fused_pricing(name, base, monkeypatch):
    """rc, the list dots in list order and their count after (d) an
    algorithm-2 row whose list holds structural (on dense64: dense) and slack
    columns, (a) a list-kernel row, which leaves the flags stale, (b) a
    column-wise row, (c) an empty list. With the small-LP kernels on (quad,
    default switches) the rows go through them instead of the list kernel."""
    env = dense_env(name, **base)
    mat, p = sc.matrix(name), sc.pricing_inputs(name)
    d = handle(name, env, monkeypatch)
    ref = RefState(mat)
    general = bool(base)
    everything = np.ones(mat.N, bool)
    d.set_mask(everything)
    rows = np.array([2, 5, 11, mat.m - 1], np.int32)
    # (d)
    d.update_row_row_wise(rows, p["rho"], 2, DROP)
    ref.row_wise(rows, p["rho"], 2, DROP)
    check_list(d, ref, f"{name} (d) list")
    assert (ref.list >= mat.n).any() and (ref.list < mat.n).any()
    if name.startswith("dense"):
        assert (mat.col_len[ref.list] == mat.m).any()
    check_fused(d, ref, name, env, p, f"{name} (d) fused after an algorithm-2 row")
    # (a)
    few = np.array([3, 7, 20], np.int32)
    d.update_row_row_wise(few, p["w"], 1, DROP)
    ref.row_wise(few, p["w"], 1, DROP)
    check_list(d, ref, f"{name} (a) list", ("list",) if general else None)
    assert len(ref.list) > 0
    check_fused(d, ref, name, env, p, f"{name} (a) fused after a list-kernel row")
    # (b)
    d.update_row_column_wise(p["rho"], DROP)
    ref.column_wise(p["rho"], DROP)
    check_list(d, ref, f"{name} (b) list",
               ("column_wise_general",) if general else ("column_wise_small",))
    assert len(ref.list) > mat.N // 2
    check_fused(d, ref, name, env, p, f"{name} (b) fused after a column-wise row")
    # (c)
    d.set_mask(np.zeros(mat.N, bool))
    ref.set_relevant(np.zeros(mat.N, bool))
    d.update_row_row_wise(few, p["w"], 1, DROP)
    ref.row_wise(few, p["w"], 1, DROP)
    check_list(d, ref, f"{name} (c) list", ("list",) if general else None)
    assert len(ref.list) == 0
    check_fused(d, ref, name, env, p, f"{name} (c) fused on an empty list")
    d.set_mask(everything)


HAZARD = [("quad", {}), ("quad", sc.OFF), ("dense64", sc.OFF)]


@pytest.mark.parametrize("name,base", HAZARD, ids=[f"{n}-{'general' if b else 'small'}"
                                                    for n, b in HAZARD])
def test_pricing_between_a_fused_update_row_and_its_dots(name, base, monkeypatch):
    """The fused column-wise row parks a_j . w for ListDotsOverUpdateRow(w) in
    the buffer that pricing writes its reduced costs to: after a pricing call
    the dots must be computed again, and the row itself is untouched."""
    env = dense_env(name, **base)
    mat, p = sc.matrix(name), sc.pricing_inputs(name)
    d = handle(name, env, monkeypatch)
    ref = RefState(mat)
    d.set_mask(np.ones(mat.N, bool))
    rows = np.array([1, 4], np.int32)
    d.update_row_row_wise(rows, p["y"], 2, DROP)
    ref.row_wise(rows, p["y"], 2, DROP)
    for fused in (False, True):
        what = f"{name} {'fused' if fused else 'plain'} pricing after a fused row"
        d.update_row_column_wise(p["rho"], DROP, p["w"])
        ref.column_wise(p["rho"], DROP)
        check_list(d, ref, what)
        coeff = d.download_coefficients()
        same_bits(coeff, ref.coeff, what + " coefficients")
        if fused:
            # Other second vector than the parked one: its dots land where the
            # parked ones may be looked for.
            rc, dots = d.pricing(p["c"], p["y"], p["rho"])
            same_bits(dots, ref.list_dots(ref.list, p["rho"]), what + " pricing dots")
        else:
            rc = d.pricing(p["c"], p["y"])
        same_bits(rc, ref.pricing(p["c"], p["y"]), what + " rc")
        same_bits(d.list_dots_over_update_row(p["w"]), ref.list_dots(ref.list, p["w"]),
                  what + " dots over the row")
        same_bits(d.download_coefficients(), coeff, what + " coefficients afterwards")
        check_list(d, ref, what + " afterwards")


@pytest.mark.parametrize("name", ["quad", "dense64"])
def test_pricing_two_column_shards(name, monkeypatch):
    """rc joined in column order; the list dots joined in block order are the
    reference's in list order."""
    env = dense_env(name, **SHARDS)
    mat, p = sc.matrix(name), sc.pricing_inputs(name)
    d = handle(name, env, monkeypatch)
    ref = RefState(mat)
    d.set_mask(np.ones(mat.N, bool))
    check_pricing(d, name, env, p["c"], p["y"], f"{name} two shards")
    check_pricing(d, name, env, p["c"], p["y_special"], f"{name} two shards, NaN and inf in y")
    rows = np.array([2, 5, 11, mat.m - 1], np.int32)
    d.update_row_row_wise(rows, p["rho"], 2, DROP)
    ref.row_wise(rows, p["rho"], 2, DROP)
    check_list(d, ref, f"{name} two shards list")
    assert (ref.list >= mat.n).any() and (ref.list < 64).any()  # both blocks are listed
    check_fused(d, ref, name, env, p, f"{name} two shards fused")


# --- row sums -------------------------------------------------------------------------------------

def check_row_sums(d, ref, x, skip, sign, what):
    got = d.row_sums(x, skip is not None, sign)
    same_bits(got, ref.row_sums(x, skip, sign), what)
    return got


def test_row_sums_short_and_long_rows(monkeypatch):
    """rows70: one-entry rows through the padded chunks of a workgroup whose
    longest row has 200 entries, a slack-only workgroup, a workgroup of 6
    rows. Both signs; zeros, a NaN and an inf in x; without the kBasic mask,
    and with it after its first upload, after a change of three words and
    back at the first mask (by SetMask's code the three words go up as changed
    words; the test sees the results only)."""
    mat, p = sc.matrix("rows70"), sc.row_sum_inputs("rows70")
    d = handle("rows70", {}, monkeypatch, cached=False)
    try:
        ref = RefState(mat)
        for sign in (1.0, -1.0):
            for key in ("x", "x_nan", "x_inf"):
                out = check_row_sums(d, ref, p[key], None, sign, f"rows70 {key} sign {sign}")
            assert np.isinf(out).any()
        out = check_row_sums(d, ref, p["x"], None, -1.0, "rows70 zero row")
        assert bits(out[sc.ROWS70_ZERO_ROW]) == 0
        for label, mask in (("first upload", p["basic"]), ("three words changed", p["basic3"]),
                            ("first mask again", p["basic"])):
            d.set_basic_mask(mask)
            for sign in (1.0, -1.0):
                for key in ("x", "x_nan"):
                    check_row_sums(d, ref, p[key], mask, sign,
                                   f"rows70 skip basic, {label}, {key} sign {sign}")
        # The mask stays on the device when it is not asked for.
        check_row_sums(d, ref, p["x_inf"], None, 1.0, "rows70 no skip after the masks")
    finally:
        d.close()


def test_wide_masks_changed_in_every_word(monkeypatch):
    """More than 512 mask words, a kBasic and a kRelevant mask that change in
    every one of them: more than DeviceLp::SetMask sends as changed words, so
    by its code they go up whole. The test sees the results only: row sums and
    norms under the first mask and under the changed one."""
    mat, p = sc.matrix("wide"), sc.row_sum_inputs("wide")
    words = (mat.N + 63) // 64
    assert words > 512
    d = handle("wide", {}, monkeypatch, cached=False)
    try:
        ref = RefState(mat)
        for label, mask in (("first", p["basic"]), ("every word changed", p["flipped"])):
            d.set_basic_mask(mask)
            check_row_sums(d, ref, p["x"], mask, -1.0, f"wide skip basic, {label}")
        assert sc.changed_words(p["basic"], p["flipped"]) == words
        check_row_sums(d, ref, p["x_nan"], None, 1.0, "wide no skip")
        for label, mask in (("first", sc.relevant_mask("wide")),
                            ("every word changed", sc.relevant_flipped("wide"))):
            d.set_mask(mask)
            ref.set_relevant(mask)
            rel = np.nonzero(mask)[0]
            same_bits(d.column_squared_norms()[rel], ref.column_squared_norms()[rel],
                      f"wide norms, {label}")
        assert sc.changed_words(sc.relevant_mask("wide"), sc.relevant_flipped("wide")) == words
    finally:
        d.close()


def test_row_sums_and_norms_with_column_shards(monkeypatch):
    """Both stay on the unsplit handle, whose own masks go up when first used."""
    mat, p = sc.matrix("rows70"), sc.row_sum_inputs("rows70")
    d = handle("rows70", SHARDS, monkeypatch)
    ref = RefState(mat)
    d.set_basic_mask(p["basic"])
    check_row_sums(d, ref, p["x"], p["basic"], -1.0, "rows70 two shards row sums")
    mask = sc.relevant_mask("rows70")
    d.set_mask(mask)
    ref.set_relevant(mask)
    rel = np.nonzero(mask)[0]
    same_bits(d.column_squared_norms()[rel], ref.column_squared_norms()[rel],
              "rows70 two shards norms")


# --- column norms ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["quad", "wave", "rows70"])
def test_column_squared_norms(name, monkeypatch):
    """Relevant positions only (the others are undefined): bit 0 and bit N - 1
    on, one whole word off; then every column."""
    mat, mask = sc.matrix(name), sc.relevant_mask(name)
    d = handle(name, {}, monkeypatch)
    ref = RefState(mat)
    ref.set_relevant(mask)
    d.set_mask(mask)
    got = d.column_squared_norms()
    rel = np.nonzero(mask)[0]
    assert mask[0] and mask[mat.N - 1]
    if name == "wave":
        assert set(sc.NORM_LENGTHS) <= set(mat.col_len[rel].tolist())
    same_bits(got[rel], ref.column_squared_norms()[rel], f"{name} norms")
    d.set_mask(np.ones(mat.N, bool))
    ref.set_relevant(np.ones(mat.N, bool))
    same_bits(d.column_squared_norms(), ref.column_squared_norms(), f"{name} norms, all columns")


# --- boxed flips and the reduced-cost copy --------------------------------------------------------

def begin(d, ref, rc, colbits):
    ones = np.ones(len(rc))
    d.dual_begin(rc, colbits, ones)
    ref.dual_begin(rc, colbits, ones)


def check_flips(d, ref, cols, threshold, taken, what):
    got = d.dual_boxed_flips(cols, threshold)
    want = ref.boxed_flips(cols, threshold)
    assert got.dtype == np.uint8 and np.array_equal(got, want), (what, np.nonzero(got != want)[0])
    assert d.last_flips() == {"early_taken": taken}, what
    return got


@pytest.mark.parametrize("name", ["quad", "wave"])
def test_boxed_flips_table(name, monkeypatch):
    """The hand-worked rows of FLIP_TABLE among random columns, over all N
    columns and as unsorted lists of 1, 255, 256, 257 and N columns (quad has
    N = 256: a list of 257 would not fit its buffers, so wave runs them too)."""
    mat = sc.matrix(name)
    d = handle(name, {}, monkeypatch)
    ref = RefState(mat)
    for threshold in (0.5, 0.0):
        rc, colbits, at, rows = sc.flip_state(mat.N, threshold, 5000 + mat.N)
        begin(d, ref, rc, colbits)
        got = check_flips(d, ref, None, threshold, False, f"{name} all columns, {threshold}")
        assert got[at].tolist() == [r[3] for r in rows]
        assert 0 < got.sum() < mat.N
        rng = np.random.default_rng(5100)
        for n in sorted({1, 255, 256, 257, mat.N}):
            if n > mat.N:
                continue
            cols = rng.permutation(mat.N)[:n].astype(np.int32)
            if n == 1:
                cols[0] = at[[r[4] for r in rows].index(1)]  # a table row that flips
            assert n < 3 or np.any(np.diff(cols) < 0)
            got = check_flips(d, ref, cols, threshold, False, f"{name} list of {n}, {threshold}")
            assert got.sum() > 0
        # The table's rows as a list of their own, last row first.
        got = check_flips(d, ref, at[::-1].astype(np.int32), threshold, False, f"{name} table")
        assert got.tolist() == [r[4] for r in rows][::-1]


UP = (STATUS_AT_UPPER << STATUS_SHIFT) | COL_BOXED
LO = (STATUS_AT_LOWER << STATUS_SHIFT) | COL_BOXED


def _early_state(mat, seed):
    """Every column boxed at a bound, rc in (-1, 1): flips where the side
    matches and |rc| is above the threshold."""
    rng = np.random.default_rng(seed)
    rc = rng.uniform(-1.0, 1.0, mat.N)
    colbits = np.where(rng.random(mat.N) < 0.5, UP, LO).astype(np.uint8)
    cols = rng.permutation(mat.N)[:100].astype(np.int32)
    return rc, colbits, cols


EARLY = ("same", "threshold", "columns", "length", "bits_listed", "bits_unlisted", "update",
         "set_rc", "take_priced", "all_columns")


@pytest.mark.parametrize("step", EARLY)
def test_early_boxed_flips(step, monkeypatch):
    """DualBoxedFlips takes the early launch's flags only for the same columns
    and threshold, with no reduced cost written since and no listed column's
    bits changed. Every other step changes something that makes at least one
    early flag wrong (asserted on the reference), so taking them would fail."""
    mat, p = sc.matrix("quad"), sc.pricing_inputs("quad")
    d = handle("quad", {}, monkeypatch)
    ref = RefState(mat)
    d.set_mask(np.ones(mat.N, bool))
    rows = np.array([2, 5, 11], np.int32)
    d.update_row_row_wise(rows, p["rho"], 2, DROP)
    ref.row_wise(rows, p["rho"], 2, DROP)
    check_list(d, ref, "early: list")
    rc, colbits, cols = _early_state(mat, 5200)
    # A flipping column of the list, and one that does not flip.
    begin(d, ref, rc, colbits)
    threshold = 0.25
    if step == "take_priced":
        d.pricing(p["c"], p["y"])
        ref.pricing(p["c"], p["y"])
    early_cols = cols
    if step == "length":
        # A listed call for all 100 columns at another threshold leaves them
        # and its flags in the buffers; the early launch then takes the first
        # 99. Asking for all 100 finds the very same 100 columns there: only
        # the length tells that flag 99 is the older call's, and it is wrong.
        stale, fresh = ref.boxed_flips(cols, 0.75), ref.boxed_flips(cols, threshold)
        i = int(np.nonzero(stale != fresh)[0][0])
        cols = cols.copy()
        cols[[i, 99]] = cols[[99, i]]
        stale = check_flips(d, ref, cols, 0.75, False, "early: length, the older call")
        assert stale[99] != ref.boxed_flips(cols, threshold)[99]
        early_cols = cols[:99].copy()
    early = ref.boxed_flips(early_cols, threshold)
    flipping = int(cols[np.nonzero(early)[0][0]])
    assert 0 < early.sum() < len(early_cols)
    d.dual_boxed_flips_early(early_cols, threshold)
    ask, ask_threshold, taken = cols, threshold, False
    if step == "same":
        taken = True
    elif step == "threshold":
        ask_threshold = 0.75
    elif step == "columns":
        ask = cols[::-1].copy()
    elif step == "length":
        pass  # all 100 columns, the early launch's threshold
    elif step == "bits_listed":
        other = LO if colbits[flipping] == UP else UP
        d.dual_set_col_bits([flipping], [other])
        ref.dual_set_col_bits([flipping], [other])
    elif step == "bits_unlisted":
        unlisted = np.setdiff1d(np.arange(mat.N), cols)[:5].astype(np.int32)
        swapped = np.where(colbits[unlisted] == UP, LO, UP).astype(np.uint8)
        d.dual_set_col_bits(unlisted, swapped)
        ref.dual_set_col_bits(unlisted, swapped)
        taken = True
    elif step == "update":
        listed = np.intersect1d(ref.list, cols)
        assert len(listed) > 0
        d.dual_update_reduced_costs(1e6, mat.N - 1, 0.5, int(ref.list[0]))
        ref.update_reduced_costs(1e6, mat.N - 1, 0.5, int(ref.list[0]))
    elif step == "set_rc":
        d.dual_set_reduced_cost(flipping, 0.0)
        ref.set_reduced_cost(flipping, 0.0)
    elif step == "take_priced":
        d.dual_take_priced_reduced_costs()
        ref.take_priced()
    elif step == "all_columns":
        ask = None
    want = ref.boxed_flips(ask, ask_threshold)
    if taken:
        assert np.array_equal(want, early), step
    elif step != "length":  # its own stale flag is asserted above
        k = min(len(want), len(early))
        assert not np.array_equal(want[:k], early[:k]), step
    check_flips(d, ref, ask, ask_threshold, taken, f"early: {step}")
    # The early launch is used up: the same question again is a launch.
    check_flips(d, ref, early_cols, threshold, False, f"early: {step}, asked again")
    if step == "update":
        same_bits(d.dual_download_reduced_costs(), ref.rc, "early: rc after the update")


def test_early_boxed_flips_switched_off(monkeypatch):
    mat = sc.matrix("quad")
    d = handle("quad", {"MILP_EARLY_FLIPS": "0"}, monkeypatch)
    ref = RefState(mat)
    rc, colbits, cols = _early_state(mat, 5300)
    begin(d, ref, rc, colbits)
    for _ in range(2):
        d.dual_boxed_flips_early(cols, 0.25)
        got = check_flips(d, ref, cols, 0.25, False, "early flips off")
        assert 0 < got.sum() < len(cols)


@pytest.mark.parametrize("env", [{}, SHARDS], ids=["one", "two_shards"])
def test_priced_reduced_costs_become_the_device_copy(env, monkeypatch):
    """pricing, take, download: the pricing result bit for bit (the NaN, the
    inf and both zeros of c included); then single positions are set: the
    first and last structural column, the first and last slack."""
    mat, p = sc.matrix("quad"), sc.pricing_inputs("quad")
    d = handle("quad", env, monkeypatch)
    ref = RefState(mat)
    zeros = np.zeros(mat.N)
    begin(d, ref, zeros, zeros.astype(np.uint8))
    got = d.pricing(p["c"], p["y"])
    same_bits(got, ref.pricing(p["c"], p["y"]), "pricing")
    same_bits(d.dual_download_reduced_costs(), zeros, "rc before the take")
    d.dual_take_priced_reduced_costs()
    ref.take_priced()
    same_bits(d.dual_download_reduced_costs(), got, "rc after the take")
    for col, value in ((0, -0.0), (mat.n - 1, 1.5), (mat.n, np.inf), (mat.N - 1, -2.0 ** -1074)):
        assert bits(ref.rc[col]) != bits(value)
        d.dual_set_reduced_cost(col, value)
        ref.set_reduced_cost(col, value)
        same_bits(d.dual_download_reduced_costs(), ref.rc, f"rc after setting column {col}")
    changed = np.nonzero(bits(ref.rc) != bits(got))[0]
    assert changed.tolist() == [0, mat.n - 1, mat.n, mat.N - 1]
    # A second pricing call does not move the device copy until it is taken;
    # then the copy is that call's result on all bits, its NaNs included.
    got = d.pricing(p["c"], p["y_special"])
    ref2 = RefState(mat)
    ref2.pricing(p["c"], p["y_special"])
    same_rc(got, ref2, "second pricing")
    assert np.isnan(ref2.priced_dots).any()
    same_bits(d.dual_download_reduced_costs(), ref.rc, "rc after another pricing")
    d.dual_take_priced_reduced_costs()
    same_bits(d.dual_download_reduced_costs(), got, "rc after the second take")
