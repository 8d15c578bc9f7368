"""Inputs of the operation-level tests of pricing, row sums, column norms and
boxed flips (tests/test_solveops_gpu.py), checked without a GPU by
tests/test_solveops_ref_cpu.py.

TEST INFRASTRUCTURE ONLY. Values are those of tests/panel_cases.py:
+-2^e (1 + u), e uniform in [-12, 12], u uniform in [0, 1); vectors hold about
10 % +0.0 and 2 % -0.0.

  quad, wave, dense5 .. dense23   the matrices of panel_cases
  dense{m}, m in NEW_DENSE        built the same way (n = 80, 70 full columns:
                                  two dense workgroups, the second partial);
                                  m reaches the unrolled loop of
                                  dense_dot_kernel<.., U> and each hand-off
                                  (DENSE_UNROLL_ROWS)
  rows70                          m = 70, n = 230: row lengths chosen per
                                  32-row workgroup of row_sum_kernel
  wide                            m = 40, n = 33000: more than 512 mask words,
                                  one or two entries per column

An inf or NaN input must only ever propagate: no builder lets an operation
create a NaN (inf - inf), and each asserts that every NaN of its reference
carries the input NaN's bits. The device's NaNs are compared on all bits too,
with one exception: the sign of rc = c - dot where the dot is NaN
(tests/test_solveops_gpu.py same_rc).
"""
import functools

import numpy as np

import panel_cases as pc
from device_ref import (COL_BOXED, STATUS_AT_LOWER, STATUS_AT_UPPER, STATUS_SHIFT, Matrix,
                        RefState, bits, column_scalar_products)

DROP = 1e-11
NAN_BITS = np.uint64(0x7FF8000000000000)  # of np.nan, the only NaN the inputs hold
OFF = {"MILP_SMALL_FUSED": "off"}
FORCE = {"MILP_DENSE_BLOCK": "force"}

# Unroll U -> rows m. With pairs = (m >> 2) >> 1: pairs == U (no leftover
# pair, even step count, no tail), pairs == U + 1 with an odd step and three
# tail rows (U = 32: pairs == U with them), pairs == 2 U - 1.
DENSE_UNROLL_ROWS = {8: (64, 79, 120), 16: (128, 143, 248), 32: (256, 263)}
NEW_DENSE = tuple(m for ms in DENSE_UNROLL_ROWS.values() for m in ms)
OLD_DENSE = pc.DENSE_ROWS


def dense_shape(m):
    steps = m >> 2
    return dict(pairs=steps >> 1, odd=steps & 1, tail=m - 4 * steps)


def _check_dense_rows():
    for u, ms in DENSE_UNROLL_ROWS.items():
        s = [dense_shape(m) for m in ms]
        assert s[0] == dict(pairs=u, odd=0, tail=0), (u, s[0])
        if u < 32:
            assert s[1] == dict(pairs=u + 1, odd=1, tail=3) and s[2]["pairs"] == 2 * u - 1
        else:
            assert s[1] == dict(pairs=u, odd=1, tail=3)


_check_dense_rows()


def _from_columns(m, n, lengths, seed):
    """As panel_cases.matrix: column c holds lengths[c] entries in random rows."""
    rng = np.random.default_rng(seed)
    per_row = [([], []) for _ in range(m)]
    for c, length in enumerate(lengths):
        rows = np.sort(rng.choice(m, length, replace=False))
        for r, x in zip(rows, pc._values(rng, length)):
            per_row[r][0].append(c)
            per_row[r][1].append(x)
    mat = Matrix(m, n, [(np.array(c, np.int32), np.array(x, np.float64)) for c, x in per_row])
    assert list(np.diff(mat.col_starts)) == list(lengths)
    return mat


# rows70: lengths include the slack. Workgroup 0 mixes one-entry rows with
# rows at and around one, two and three 64-entry chunks (its chunk count, 4,
# comes from the 200-entry rows); workgroup 1 is slack only (one chunk);
# workgroup 2 has 6 rows.
ROWS70_N = 230
ROWS70_LENS = ((1, 2, 63, 64, 65, 128, 129, 200) * 4 + (1,) * 32 + (3, 64, 1, 65, 130, 3))
ROWS70_ZERO_ROW = 9  # two entries; both multipliers are zeros in every x
WIDE_M, WIDE_N = 40, 33000
# Seeds chosen so that every length class of every case tells summation orders
# apart (tests/test_solveops_ref_cpu.py).
ROWS70_SEED = 3500
MASK_SEEDS = {"quad": 4301, "wave": 4300, "rows70": 4323, "wide": 4300}
# The word that is off in the relevant mask: on wave the third (slack columns;
# its second holds the only order-sensitive columns of 65 entries).
OFF_WORD = {"wave": 2}


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name in pc.CASES:
        return pc.matrix(name)
    if name.startswith("dense"):
        m = int(name[5:])
        assert m in NEW_DENSE
        return _from_columns(m, 80, [min(m, 2) if c % 8 == 7 else m for c in range(80)], 3000 + m)
    if name == "rows70":
        rng = np.random.default_rng(ROWS70_SEED)
        rows = []
        for length in ROWS70_LENS:
            cols = np.sort(rng.choice(ROWS70_N, length - 1, replace=False)).astype(np.int32)
            rows.append((cols, pc._values(rng, length - 1)))
        mat = Matrix(70, ROWS70_N, rows)
        assert tuple(mat.row_len) == ROWS70_LENS and mat.row_len[ROWS70_ZERO_ROW] == 2
        return mat
    assert name == "wide"
    mat = _from_columns(WIDE_M, WIDE_N, [1 + c % 2 for c in range(WIDE_N)], 3600)
    assert (mat.N + 63) // 64 > 512
    return mat


def environment(name):
    return dict(FORCE) if name.startswith("dense") else {}


def _family(rng, k):
    v = pc._values(rng, k)
    kind = rng.random(k)
    v[kind < 0.10] = 0.0
    v[(kind >= 0.10) & (kind < 0.12)] = -0.0
    return v


POOL = pc.MAX_K  # candidate vectors per matrix
# name -> the pool's vectors used as (y, w, rho, the one that gets NaN and inf).
# y, w and rho are chosen so that each of them alone tells the summation
# orders apart in every length class (orders_not_told_apart is empty for it).
VECTOR_PICK = {"quad": (2, 3, 4, 7), "wave": (5, 12, 16, 17), "dense5": (0, 2, 3, 4),
               "dense8": (1, 2, 3, 4)}
DEFAULT_PICK = (0, 1, 2, 3)


@functools.lru_cache(maxsize=None)
def vector_pool(name):
    """(POOL, m), read-only: panel_cases.vectors for its matrices, the same
    family for the others."""
    if name in pc.CASES:
        return pc.vectors(name)
    m = matrix(name).m
    v = _family(np.random.default_rng(4000 + m), POOL * m).reshape(POOL, m)
    v.setflags(write=False)
    return v


def vectors(name):
    """(4, m): y, w, rho and the vector that gets the NaN and inf."""
    return vector_pool(name)[list(VECTOR_PICK.get(name, DEFAULT_PICK))]


def only_input_nans(a):
    a = np.asarray(a, np.float64)
    return bool(np.all(bits(a)[np.isnan(a)] == NAN_BITS))


@functools.lru_cache(maxsize=None)
def pricing_inputs(name):
    """c (N: the family, +0.0 at 3, -0.0 at 4, an inf at 1, NaN at 2), y, w, and
    y_special = a fourth vector with NaN and inf planted. The inf of c takes
    the sign that does not meet an equal inf of a dot."""
    mat = matrix(name)
    v = vectors(name)
    rng = np.random.default_rng(4100 + mat.m)
    c = _family(rng, mat.N)
    c[3], c[4], c[2] = 0.0, -0.0, np.nan
    y_special = v[3].copy()
    y_special[mat.m // 3], y_special[(2 * mat.m) // 3] = np.nan, np.inf
    ref = RefState(mat)
    for sign in (1.0, -1.0):
        c[1] = sign * np.inf
        if only_input_nans(ref.pricing(c, y_special)):
            break
    else:
        raise AssertionError(name)
    for a in (c, y_special):
        a.setflags(write=False)
    out = dict(c=c, y=v[0], w=v[1], rho=v[2], y_special=y_special)
    assert only_input_nans(ref.pricing(c, v[0])) and np.isinf(ref.pricing(c, y_special)).any()
    return out


def dots_in_order(mat, cols, y, order):
    """a_col . y summed in another order (the products round the same way):
    "sequential" left to right, "pairwise" the four chains of
    ColumnScalarProduct folded as (r1 + r2) + (r3 + r4)."""
    out = np.zeros(len(cols))
    for i, c in enumerate(cols):
        s, e = mat.starts[c], mat.starts[c + 1]
        prod = mat.c_vals[s:e] * y[mat.c_rows[s:e]]
        length = e - s
        if order == "sequential":
            res = np.float64(0.0)
            for t in range(length):
                res = res + prod[t]
        else:
            r = [np.float64(0.0)] * 4
            full = (length // 4) * 4
            for t in range(full):
                r[t % 4] = r[t % 4] + prod[t]
            res = (r[0] + r[1]) + (r[2] + r[3])
            for t in range(full, length):
                res = res + prod[t]
        out[i] = res
    return out


def orders_not_told_apart(mat, v):
    """The (order, column length) classes in which the vector v gives
    ColumnScalarProduct's bits in every column although the sum is taken in
    another order: left to right for lengths of at least 8 (up to 7 entries
    each of the four chains holds one product and the orders coincide), the
    fold (r1 + r2) + (r3 + r4) for lengths of at least 5."""
    missed = []
    for order, least in (("sequential", 8), ("pairwise", 5)):
        for L in np.unique(mat.col_len):
            if L < least:
                continue
            cols = np.nonzero(mat.col_len == L)[0]
            ref = column_scalar_products(mat, cols, v)
            if not np.any(bits(ref) != bits(dots_in_order(mat, cols, v, order))):
                missed.append((order, int(L)))
    return missed


# --- row sums -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def row_sum_inputs(name):
    """x (N, the family with both zeros), x_nan and x_inf (one entry replaced, in
    a column that several rows hold), and three kBasic masks: `basic`, the
    same with bits of three words changed, and a mask that differs from `basic`
    in every word."""
    mat = matrix(name)
    rng = np.random.default_rng(4200 + mat.m)
    x = _family(rng, mat.N)
    if name == "rows70":
        cols = mat.t_cols[ROWS70_ZERO_ROW]
        x[cols[0]], x[cols[1]] = 0.0, -0.0
    count = np.zeros(mat.N, np.int64)
    for c in mat.t_cols:
        count[c] += 1
    shared = np.nonzero((count >= 2) & (x != 0.0))[0]
    x_nan, x_inf = x.copy(), x.copy()
    x_nan[shared[0]] = np.nan
    x_inf[shared[1]] = -np.inf
    basic = rng.random(mat.N) < 0.3
    basic[[shared[0], shared[1]]] = False
    words = (mat.N + 63) // 64
    basic3 = basic.copy()
    for w in (0, words // 2, words - 1):  # three changed words
        for b in (64 * w, 64 * w + 5):
            basic3[b] = ~basic3[b]
    flipped = ~basic
    out = dict(x=x, x_nan=x_nan, x_inf=x_inf, basic=basic, basic3=basic3, flipped=flipped)
    for a in out.values():
        a.setflags(write=False)
    ref = RefState(mat)
    for key in ("x", "x_nan", "x_inf"):
        for skip in (None, basic):
            assert only_input_nans(ref.row_sums(out[key], skip, -1.0)), (name, key)
    return out


def row_sums_reversed(mat, x, skip, sign):
    """The reference's terms added from the last entry to the first."""
    skip = np.zeros(mat.N, bool) if skip is None else skip
    out = np.zeros(mat.m)
    for r in range(mat.m):
        cols = mat.t_cols[r]
        mult = sign * x[cols]
        live = ~skip[cols] & (mult != 0.0)
        acc = np.float64(0.0)
        for p in (mult[live] * mat.t_vals[r][live])[::-1]:
            acc = acc + p
        out[r] = acc
    return out


# --- column norms ---------------------------------------------------------------------------------

NORM_LENGTHS = (0, 1, 63, 64, 65, 129)  # around one and two wave-wide steps of the kernel


@functools.lru_cache(maxsize=None)
def relevant_mask(name):
    """Random, with bit 0 and bit N - 1 on and one whole word off (OFF_WORD,
    else the second). On wave the first column of each of NORM_LENGTHS outside
    that word is on."""
    mat = matrix(name)
    mask = np.random.default_rng(MASK_SEEDS[name]).random(mat.N) < 0.7
    off = 64 * OFF_WORD.get(name, 1)
    if name == "wave":
        for length in NORM_LENGTHS:
            c = [c for c in np.nonzero(mat.col_len == length)[0] if not off <= c < off + 64][0]
            mask[c] = True
    mask[0] = mask[mat.N - 1] = True
    mask[off:off + 64] = False
    if name == "wave":
        assert set(NORM_LENGTHS) <= set(mat.col_len[mask].tolist())
    mask.setflags(write=False)
    return mask


def relevant_flipped(name):
    """Differs from relevant_mask(name) in every word."""
    mask = ~relevant_mask(name)
    mask.setflags(write=False)
    return mask


def changed_words(a, b):
    """How many 64-bit words of two column masks differ."""
    diff = np.asarray(a, bool) != np.asarray(b, bool)
    diff = np.concatenate([diff, np.zeros((-len(diff)) % 64, bool)])
    return int(diff.reshape(-1, 64).any(axis=1).sum())


def norms_four_chains(mat, cols):
    """1 + the squares summed as ColumnScalarProduct sums products (four chains,
    ((r1 + r2) + r3) + r4, then the tail): not the order of SquaredNorm."""
    out = np.zeros(len(cols))
    for i, c in enumerate(cols):
        v = mat.c_vals[mat.starts[c]:mat.starts[c + 1]]
        sq = v * v
        r = [np.float64(0.0)] * 4
        full = (len(v) // 4) * 4
        for t in range(full):
            r[t % 4] = r[t % 4] + sq[t]
        res = ((r[0] + r[1]) + r[2]) + r[3]
        for t in range(full, len(v)):
            res = res + sq[t]
        out[i] = 1.0 + res
    return out


# --- boxed flips ----------------------------------------------------------------------------------

_B = COL_BOXED
_LO, _UP = STATUS_AT_LOWER << STATUS_SHIFT, STATUS_AT_UPPER << STATUS_SHIFT
_NAN, _INF = float("nan"), float("inf")
_TINY = 5e-324
# (threshold, rc, column byte, flips without a list, flips in a list)
FLIP_TABLE = (
    (0.5, 0.5, _UP | _B, 0, 0),                       # rc == threshold
    (0.5, -0.5, _LO | _B, 0, 0),                      # rc == -threshold
    (0.5, float(np.nextafter(0.5, 1.0)), _UP | _B, 1, 1),
    (0.5, float(np.nextafter(-0.5, -1.0)), _LO | _B, 1, 1),
    (0.5, _NAN, _UP | _B, 0, 0),
    (0.5, _NAN, _LO | _B, 0, 0),
    (0.5, _INF, _UP | _B, 1, 1),
    (0.5, -_INF, _LO | _B, 1, 1),
    (0.5, _INF, _LO | _B, 0, 0),                      # the wrong side
    (0.5, -_INF, _UP | _B, 0, 0),
    (0.5, 2.0, _UP, 0, 1),                            # boxed bit clear
    (0.5, -2.0, _LO, 0, 1),
    (0.5, 2.0, _B, 0, 0),                             # status 0 (basic)
    (0.5, 2.0, (1 << STATUS_SHIFT) | _B, 0, 0),       # status 1 (fixed)
    (0.5, -2.0, (4 << STATUS_SHIFT) | _B, 0, 0),      # status 4 (free)
    (0.5, 2.0, (7 << STATUS_SHIFT) | _B | 3, 0, 0),   # status 7, the movement bits set
    (0.0, 0.0, _UP | _B, 0, 0),                       # +-0.0 against threshold 0
    (0.0, -0.0, _LO | _B, 0, 0),
    (0.0, -0.0, _UP | _B, 0, 0),
    (0.0, 0.0, _LO | _B, 0, 0),
    (0.0, _TINY, _UP | _B, 1, 1),
    (0.0, -_TINY, _LO | _B, 1, 1),
)


def flip_state(N, threshold, seed):
    """rc, colbits and where the table's rows for `threshold` sit: the rows at
    scattered columns, every other column random (rc in (-1, 1) off the
    thresholds, any status, boxed or not)."""
    rng = np.random.default_rng(seed)
    rc = rng.uniform(-1.0, 1.0, N)
    status = rng.choice([0, 1, STATUS_AT_LOWER, STATUS_AT_UPPER, 4], N, p=[.1, .1, .35, .35, .1])
    colbits = ((status << STATUS_SHIFT) | np.where(rng.random(N) < 0.7, _B, 0) |
               rng.integers(0, 4, N)).astype(np.uint8)
    rows = [t for t in FLIP_TABLE if t[0] == threshold]
    at = np.sort(rng.choice(N, len(rows), replace=False))
    for col, (_, r, b, _, _) in zip(at, rows):
        rc[col], colbits[col] = r, b
    return rc, colbits, at, rows
