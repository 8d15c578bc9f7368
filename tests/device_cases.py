"""The table of operation-level edge cases (tests/test_device_ops_gpu.py runs
it on the device, tests/test_device_ref_cpu.py checks the reference on it).

TEST INFRASTRUCTURE ONLY. A case is (environment, builder); build(name)
returns the matrix, the relevant mask and the steps, generated with numpy from
a seed with entries uniform in (-1, 1) and shaped so that the named limit
holds exactly (the builders assert row lengths and entry totals).

Entries of a row count its slack, as DeviceLp counts them.
"""
import functools

import numpy as np

from device_ref import Matrix

DROP = 1e-11  # Glop's drop tolerance
OFF = {"MILP_SMALL_FUSED": "off"}

CASES = {}


def case(name, env=None):
    def reg(fn):
        assert name not in CASES
        CASES[name] = (dict(env or {}), fn)
        return fn
    return reg


@functools.lru_cache(maxsize=None)
def build(name):
    return CASES[name][1]()


class Built:
    def __init__(self, mat, mask, steps, setup=()):
        self.mat, self.mask, self.steps, self.setup = mat, mask, steps, tuple(setup)


def row(rows, rho, alg, path=None, compact=None, mask=None, mapped=None):
    return dict(kind="row", rows=np.asarray(rows, np.int32), rho=rho, alg=alg, path=path,
                compact=compact, mask=mask, mapped=mapped)


def colwise(rho, w=None, path=None, compact=None):
    return dict(kind="col", rho=rho, w=w, path=path, compact=compact)


def dots(v):
    return dict(kind="dots", v=v)


def listdots(cols, v):
    return dict(kind="listdots", cols=np.asarray(cols, np.int32), v=v)


# --- generators ------------------------------------------------------------

def _vals(rng, k):
    v = rng.uniform(-1.0, 1.0, k)
    v[v == 0.0] = 0.5
    return v


def gen_rows(n, seed, lens, pools, fixed=None):
    """Row r: lens[r] entries of A, the columns drawn from pools[r] (an array
    of candidate columns) plus the fixed[r] columns (counted in lens[r])."""
    rng = np.random.default_rng(seed)
    rows = []
    for r, L in enumerate(lens):
        must = np.asarray((fixed or {}).get(r, []), np.int64)
        cand = np.setdiff1d(pools[r], must)
        cols = np.sort(np.concatenate([must, rng.choice(cand, L - len(must), replace=False)]))
        rows.append((cols.astype(np.int32), _vals(rng, L)))
    return rows


def rows_from_columns(m, n, col_rows, col_vals):
    per = [([], []) for _ in range(m)]
    for c in range(n):
        for r, v in zip(col_rows[c], col_vals[c]):
            per[r][0].append(c)
            per[r][1].append(v)
    return [(np.array(c, np.int32), np.array(v, np.float64)) for c, v in per]


def rho_for(m, rows, seed, tol=None, cancel=None, negzero=None):
    rng = np.random.default_rng(seed)
    rho = np.zeros(m)
    rho[np.asarray(rows)] = _vals(rng, len(rows))
    if tol is not None:
        rho[tol] = DROP  # times the slack's 1.0: a value equal to the tolerance
    if cancel is not None:
        rho[cancel[1]] = -rho[cancel[0]]  # two equal rows: exact cancellation
    if negzero is not None:
        rho[negzero] = 1e-200  # times the row's -1e-200 entry: -0.0
    return rho


def vec(m, seed):
    return _vals(np.random.default_rng(seed), m)


def random_mask(N, seed, force=()):
    mask = np.random.default_rng(seed).random(N) < 0.7
    mask[list(force)] = True
    return mask


def add_specials(rows, n, ra, rb, rz):
    """Row rb becomes a copy of row ra (exact cancellation with rho, -rho); row
    rz trades one entry for -1e-200 at the reserved column n - 1."""
    rows[rb] = (rows[ra][0].copy(), rows[ra][1].copy())
    c, v = rows[rz]
    assert len(c) >= 1 and c[-1] < n - 1
    rows[rz] = (np.concatenate([c[:-1], [n - 1]]).astype(np.int32),
                np.concatenate([v[:-1], [-1e-200]]))
    return rows


def special_steps(mat, rows, seed, algs, path, compact, tol_row, cancel, negzero):
    """The three write-rule details on `rows`: a value equal to the tolerance,
    an exact cancellation, a -0.0 product."""
    rows = sorted(set(list(rows) + [tol_row, cancel[0], cancel[1], negzero]))
    return [row(rows, rho_for(mat.m, rows, seed + a, tol=tol_row, cancel=cancel,
                              negzero=negzero), a, path, compact) for a in algs]


def _pool(n, size, seed):
    """`size` candidate columns spread over [0, n - 1) (n - 1 is reserved)."""
    return np.sort(np.random.default_rng(seed).choice(n - 1, size, replace=False))


def _assert_entries(mat, rows, k, entries):
    assert len(rows) == k and mat.entries(rows) == entries, (len(rows), mat.entries(rows))


# --- the list kernel and its limits (N = 20000, small fused kernels off) ------

LIST_N, LIST_M = 19500, 500


@functools.lru_cache(maxsize=None)
def list_matrix():
    """Row groups by (k, entries): rows of exactly the lengths that put k rows
    at `entries` entries. Short rows share a pool of 1200 columns (columns
    repeat across rows), long rows a pool of 6000."""
    n, m = LIST_N, LIST_M
    short, long_ = _pool(n, 1200, 1), _pool(n, 6000, 2)
    groups, lens, pools = {}, [], []

    def group(name, row_lens, pool):
        groups[name] = list(range(len(lens), len(lens) + len(row_lens)))
        lens.extend(row_lens)
        pools.extend([pool] * len(row_lens))

    group("init", [40] * 6, short)            # the algorithm-2 row of every sequence
    group("k1_4096", [4095], long_)
    group("k1_4095", [4094], long_)
    group("k2_4096", [2047, 2047], long_)
    group("k2_4095", [2047, 2046], long_)
    group("k63_4096", [64] * 62 + [65], short)
    group("k63_4095", [64] * 63, short)
    group("k64_4096", [63] * 64, short)       # equal rows of 64 = 2^6 entries
    group("k64_4095", [63] * 63 + [62], short)
    group("k64_4097", [63] * 63 + [64], short)
    group("empty", [0] * 66, short)           # slack-only rows
    group("pow2_16", [255] * 16, long_)       # 16 rows of 256 entries
    group("one_long", [3999], long_)          # ~4000 entries + 63 rows of one entry
    group("common", [20] * 64, short)         # one column in all 64 rows
    group("special", [30] * 8, short)
    assert len(lens) <= m
    lens.extend([5] * (m - len(lens)))
    pools.extend([short] * (m - len(pools)))
    fixed = {r: [777] for r in groups["common"]}
    rows = gen_rows(n, 11, lens, pools, fixed)
    s = groups["special"]
    add_specials(rows, n, s[1], s[2], s[3])
    mat = Matrix(m, n, rows)
    assert mat.N == 20000
    return mat, groups


def _list_steps(k, algs=(0, 1)):
    mat, g = list_matrix()
    steps = []
    for entries, rows in ((k, g["empty"][:k]), (4095, g[f"k{k}_4095"]), (4096, g[f"k{k}_4096"])):
        _assert_entries(mat, rows, k, entries)
        for a in algs:
            steps.append(row(rows, rho_for(mat.m, rows, 100 * k + entries % 7 + a), a, "list",
                             "none", mapped=True))
    return steps


def _list_case(steps, mask_seed=3, mask=None):
    mat, g = list_matrix()
    s = g["special"]
    force = [mat.n + s[0], mat.n - 1, 777]
    mask = random_mask(mat.N, mask_seed, force) if mask is None else mask
    init = row(g["init"][:2], rho_for(mat.m, g["init"][:2], 5), 2, "chunk", "chip_wide")
    return Built(mat, mask, [init] + steps)


for _k in (1, 2, 63, 64):
    case(f"list_k{_k}", OFF)(functools.partial(lambda k: _list_case(_list_steps(k)), _k))


@case("list_shapes", OFF)
def _():
    mat, g = list_matrix()
    steps = []
    for a in (0, 1):
        _assert_entries(mat, g["common"], 64, 64 * 21)
        assert all(777 in mat.t_cols[r] for r in g["common"])
        steps.append(row(g["common"], rho_for(mat.m, g["common"], 21 + a), a, "list", "none"))
        unequal = sorted(g["one_long"] + g["empty"][:63])
        _assert_entries(mat, unequal, 64, 4000 + 63)
        steps.append(row(unequal, rho_for(mat.m, unequal, 23 + a), a, "list", "none"))
        _assert_entries(mat, g["pow2_16"], 16, 4096)
        steps.append(row(g["pow2_16"], rho_for(mat.m, g["pow2_16"], 25 + a), a, "list", "none"))
    return _list_case(steps)


@case("list_special", OFF)
def _():
    mat, g = list_matrix()
    s = g["special"]
    rows = g["k63_4095"][:50] + s
    assert len(rows) <= 64 and mat.entries(rows) <= 4096
    return _list_case(special_steps(mat, rows, 31, (0, 1), "list", "none", s[0], (s[1], s[2]),
                                    s[3]))


@case("list_nothing_relevant", OFF)
def _():
    """The list comes out empty; algorithm 1 still writes the touched positions."""
    mat, g = list_matrix()
    rows = g["k64_4096"]
    steps = [row(rows, rho_for(mat.m, rows, 41 + a), a, "list", "none") for a in (0, 1)]
    return _list_case(steps, mask=np.zeros(mat.N, bool))


@case("list_slacks_relevant", OFF)
def _():
    mat, g = list_matrix()
    rows = g["k63_4096"]
    mask = np.arange(mat.N) >= mat.n
    steps = [row(rows, rho_for(mat.m, rows, 43 + a), a, "list", "none") for a in (0, 1)]
    return _list_case(steps, mask=mask)


@case("list_fallback", OFF)
def _():
    """One past each limit: the host must leave the list kernel."""
    mat, g = list_matrix()
    r65 = g["empty"][:65]
    _assert_entries(mat, r65, 65, 65)
    r4097 = g["k64_4097"]
    _assert_entries(mat, r4097, 64, 4097)
    general = ("chunk", "by_column")
    return _list_case([row(r65, rho_for(mat.m, r65, 51), 1, general, "chip_wide"),
                       row(r4097, rho_for(mat.m, r4097, 52), 1, general, "chip_wide")])


@case("list_switched_off", dict(OFF, MILP_ROWWISE_LIST="off"))
def _():
    """The 64-row / 4096-entry case through the flag kernels + Compact: the
    same reference, so the same bits as the list kernel's."""
    mat, g = list_matrix()
    rows = g["k64_4096"]
    _assert_entries(mat, rows, 64, 4096)
    steps = [row(rows, rho_for(mat.m, rows, 6400 + 4096 % 7 + 1), 1, ("chunk", "by_column"),
                 "chip_wide")]
    return _list_case(steps)


@case("list_dense_block_dots", dict(OFF, MILP_DENSE_BLOCK="force"))
def _():
    """Three full structural columns form a dense block: the listed dots after
    a list-kernel row need the flags rebuilt from the list (FlagsFromList)."""
    n, m = 19900, 100
    dense = [100, 5000, 19000]
    pool = _pool(n, 1500, 7)
    rows = gen_rows(n, 61, [40] * m, [pool] * m, {r: dense for r in range(m)})
    mat = Matrix(m, n, rows)
    assert all(mat.col_len[c] == m for c in dense) and mat.N == 20000
    mask = random_mask(mat.N, 62, dense)
    f = list(range(10, 90, 2))
    steps = [row(range(4), rho_for(m, range(4), 63), 2, "chunk", "chip_wide")]
    for a in (1, 0):
        steps += [row(f, rho_for(m, f, 64 + a), a, "list", "none"), dots(vec(m, 66 + a))]
    return Built(mat, mask, steps)


# --- chunk kernel -----------------------------------------------------------------

LIST_OFF = dict(OFF, MILP_ROWWISE_LIST="off")


def _chunk_matrix(N, long_column=False):
    m = 60
    n = N - m
    pool = _pool(n, 200, N)
    fixed = {0: [255, 256, 257], 1: [256], 2: [255, 257, n - 2]}
    if long_column:
        for r in range(10, 43):
            fixed[r] = [1000]  # a column of 33 entries
    rows = gen_rows(n, N + 1, [30] * m, [pool] * m, fixed)
    add_specials(rows, n, 4, 5, 6)
    mat = Matrix(m, n, rows)
    assert mat.N == N
    return mat


def _chunk_case(N):
    mat = _chunk_matrix(N)
    m = mat.m
    mask = random_mask(N, N + 2, [255, 256, 257, N - 1, mat.n + 3, mat.n - 1])
    last = [0, 1, 2, m - 1]  # the slack of row m - 1 is column N - 1
    f16 = sorted(set(range(0, 32, 2)))
    steps = [row(range(3), rho_for(m, range(3), 1), 2, "chunk", "small")]
    for a in (0, 1, 2):
        steps.append(row(last, rho_for(m, last, 10 + a), a, "chunk", "small"))
    for a in (1, 2):
        steps.append(row(f16, rho_for(m, f16, 20 + a), a, "chunk", "small"))
    steps += special_steps(mat, [3, 7, 8], 30, (0, 1, 2), "chunk", "small", 3, (4, 5), 6)
    return Built(mat, mask, steps)


for _N in (4096, 4097, 4351):
    case(f"chunk_N{_N}", LIST_OFF)(functools.partial(_chunk_case, _N))


@case("chunk_long_column", LIST_OFF)
def _():
    """A column of 33 entries: the by-column kernel sorts at most 32 hits in
    registers, so 40 filtered rows go to the chunk kernel."""
    mat = _chunk_matrix(4351, long_column=True)
    assert mat.col_len.max() == 33
    f40 = list(range(8, 48))
    steps = [row(range(3), rho_for(mat.m, range(3), 1), 2, "chunk", "small")]
    steps += [row(f40, rho_for(mat.m, f40, 40 + a), a, "chunk", "small") for a in (1, 2)]
    return Built(mat, random_mask(mat.N, 3, [1000]), steps)


# --- by-column kernel ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _bycol_matrix():
    m, n = 260, 4800
    pool = _pool(n, 2000, 71)
    fixed = {r: [3000] for r in range(32)}  # a column of exactly 32 entries
    rows = gen_rows(n, 72, [20] * m, [np.setdiff1d(pool, [3000])] * m, fixed)
    add_specials(rows, n, 41, 42, 43)
    mat = Matrix(m, n, rows)
    assert mat.col_len.max() == 32 and mat.col_len[3000] == 32
    return mat


@case("by_column", LIST_OFF)
def _():
    mat = _bycol_matrix()
    m = mat.m
    mask = random_mask(mat.N, 73, [3000, mat.n + 40, mat.n - 1])
    f17 = list(range(0, 34, 2))
    f200 = list(range(200))
    steps = [row(range(3), rho_for(m, range(3), 1), 2, "chunk", "small")]
    for a in (1, 2):
        steps.append(row(f17, rho_for(m, f17, 74 + a), a, "by_column", "small"))
        steps.append(row(f200, rho_for(m, f200, 76 + a), a, "by_column", "small"))
    steps += special_steps(mat, range(20, 40), 78, (1, 2), "by_column", "small", 40, (41, 42), 43)
    return Built(mat, mask, steps)


# --- full rows -------------------------------------------------------------------------

def _dense_matrix(m, n, seed, tiny_column=True):
    """Every row holds every structural column; column n - 1 is -1e-200
    (tiny_column), rows 1 and 2 are equal."""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(m):
        v = _vals(rng, n)
        if tiny_column:
            v[n - 1] = -1e-200
        rows.append((np.arange(n, dtype=np.int32), v))
    rows[2] = (rows[1][0].copy(), rows[1][1].copy())
    return Matrix(m, n, rows)


@case("full_rows", OFF)
def _():
    m, n = 8, 700
    mat = _dense_matrix(m, n, 81)
    mask = random_mask(mat.N, 82, [n - 1, n + 0])
    steps = [row(range(3), rho_for(m, range(3), 1), 2, "full_rows", "small")]
    for k in (5, 6, 7, 8):
        f = list(range(m - k, m))
        for a in (1, 2):
            steps.append(row(f, rho_for(m, f, 83 + k + a), a, "full_rows", "small"))
    for a in (1, 2):
        f = [0, 1, 2, 3, 5]
        steps.append(row(f, rho_for(m, f, 90 + a, tol=0, cancel=(1, 2)), a, "full_rows", "small"))
        # Every product at column n - 1 is -0.0.
        steps.append(row(f, np.where(np.isin(np.arange(m), f), 1e-200, 0.0), a, "full_rows",
                         "small"))
    return Built(mat, mask, steps)


# --- small LPs (N <= 8192): serial, 256 threads, by column ----------------------------------

@functools.lru_cache(maxsize=None)
def _small_matrix(N):
    if N == 64:
        m, n = 8, 56
        rows = gen_rows(n, 64, [40] * m, [np.arange(n - 1)] * m)
        add_specials(rows, n, 4, 5, 6)
        return Matrix(m, n, rows), {}
    m = 1300
    n = N - m
    pool, wide = _pool(n, 600, N), _pool(n, 5000, N + 1)
    groups, lens, pools = {}, [], []

    def group(name, row_lens, p):
        groups[name] = list(range(len(lens), len(lens) + len(row_lens)))
        lens.extend(row_lens)
        pools.extend([p] * len(row_lens))

    group("k1", [4095], wide)
    group("k1_over", [4096], wide)            # 4097 entries
    group("special", [12] * 8, pool)
    group("r16", [15] * 256, pool)            # 256 rows of 16 entries
    group("r8", [7] * 2, pool)
    group("rest", [3] * (m - len(lens)), pool)
    fixed = {r: [2000] for r in groups["rest"][:40]}  # a column of 40 entries
    rows = gen_rows(n, N + 2, lens, [np.setdiff1d(p, [2000]) for p in pools], fixed)
    s = groups["special"]
    add_specials(rows, n, s[1], s[2], s[3])
    mat = Matrix(m, n, rows)
    assert mat.N == N
    rest = groups["rest"]
    groups["k1024"] = rest[:1024]             # 1024 rows of 4 entries
    groups["k1025"] = rest[:1025]
    groups["k256"] = groups["r16"]
    groups["k257"] = sorted(groups["r16"][:255] + groups["r8"])
    return mat, groups


def _small_case(N, path):
    mat, g = _small_matrix(N)
    m = mat.m
    if N == 64:
        mask = random_mask(N, 3, [mat.n + 3, mat.n - 1])
        steps = [row(range(3), rho_for(m, range(3), 1), 2, path, "none")]
        for a in (0, 1, 2):
            steps.append(row([7], rho_for(m, [7], 10 + a), a, path, "none"))
        for a in (1, 2):
            steps.append(row(range(m), rho_for(m, range(m), 20 + a), a, path, "none"))
        steps += special_steps(mat, [3, 7], 30, (0, 1, 2), path, "none", 3, (4, 5), 6)
        return Built(mat, mask, steps)
    s = g["special"]
    mask = random_mask(N, N + 3, [mat.n + s[0], mat.n - 1, 2000])
    steps = [row(g["rest"][:3], rho_for(m, g["rest"][:3], 1), 2, path, "none")]
    _assert_entries(mat, g["k1"], 1, 4096)
    _assert_entries(mat, g["k1024"], 1024, 4096)
    for a in (0, 1, 2):
        steps.append(row(g["k1"], rho_for(m, g["k1"], 10 + a), a, path, "none"))
    for a in (1, 2):
        steps.append(row(g["k1024"], rho_for(m, g["k1024"], 20 + a), a, path, "none"))
    for k in (256, 257):
        f = g[f"k{k}"]
        _assert_entries(mat, f, k, 4096)
        for a in (1, 2):
            steps.append(row(f, rho_for(m, f, k + a), a, path, "none"))
    steps += special_steps(mat, s, 50, (0, 1, 2), path, "none", s[0], (s[1], s[2]), s[3])
    return Built(mat, mask, steps)


for _N in (64, 8191, 8192):
    case(f"small_serial_N{_N}")(functools.partial(_small_case, _N, "small_serial"))
    case(f"small_serial256_N{_N}", {"MILP_SMALL_THREADS": "256"})(
        functools.partial(_small_case, _N, "small_serial_256"))


def _small_bycol_case(N):
    """One past the serial kernel's limits: 4097 entries, or 1025 rows. The
    1025 rows hold all 40 entries of column 2000 (more hits than the register
    sort takes: repeated minimum selection)."""
    mat, g = _small_matrix(N)
    m = mat.m
    s = g["special"]
    mask = random_mask(N, N + 4, [mat.n + s[0], mat.n - 1, 2000])
    _assert_entries(mat, g["k1_over"], 1, 4097)
    _assert_entries(mat, g["k1025"], 1025, 4100)
    assert mat.col_len[2000] == 40
    steps = [row(g["rest"][:3], rho_for(m, g["rest"][:3], 1), 2, "small_serial", "none")]
    for a in (0, 1, 2):
        steps.append(row(g["k1_over"], rho_for(m, g["k1_over"], 10 + a), a, "small_by_column",
                         "none"))
    for a in (1, 2):
        steps.append(row(g["k1025"], rho_for(m, g["k1025"], 20 + a), a, "small_by_column", "none"))
    big = sorted(s + g["k1025"])
    steps += special_steps(mat, big, 30, (1, 2), "small_by_column", "none", s[0], (s[1], s[2]),
                           s[3])
    return Built(mat, mask, steps)


for _N in (8191, 8192):
    case(f"small_by_column_N{_N}")(functools.partial(_small_bycol_case, _N))


# --- medium LPs (8192 < N <= 65536) in a batch ---------------------------------------------------

def _medium_case(N, direct):
    """Positions equal mod 1024 (the LDS hash table's worst pattern). Batched
    through the small-LP batcher, or launched directly once the dual device
    mode is on."""
    m = 64
    n = N - m
    same = np.arange(5, n - 1, 1024)  # columns = 5 mod 1024
    pool = _pool(n, 800, N)
    lens = [min(len(same), 40)] * 24 + [30] * (m - 24)
    pools = [same] * 24 + [pool] * (m - 24)
    rows = gen_rows(n, N + 1, lens, pools)
    add_specials(rows, n, 41, 42, 43)
    mat = Matrix(m, n, rows)
    assert mat.N == N
    mask = random_mask(N, N + 2, [mat.n + 40, mat.n - 1, 5])
    path = "medium_direct" if direct else "medium_batched"
    f = list(range(24))
    steps = [row(range(30, 33), rho_for(m, range(30, 33), 1), 2, path, "none")]
    for a in (1, 2):
        steps.append(row(f, rho_for(m, f, 10 + a), a, path, "none"))
    steps.append(row([3], rho_for(m, [3], 13), 0, path, "none"))
    f40 = list(range(24, 64))
    steps.append(row(f40, rho_for(m, f40, 14), 1, path, "none"))
    steps += special_steps(mat, range(24, 40), 20, (0, 1, 2), path, "none", 40, (41, 42), 43)
    return Built(mat, mask, steps, setup=("small_batch", "dual_begin") if direct
                 else ("small_batch",))


for _N in (8193, 65536):
    case(f"medium_batched_N{_N}")(functools.partial(_medium_case, _N, False))
    case(f"medium_direct_N{_N}")(functools.partial(_medium_case, _N, True))


# --- column-wise ------------------------------------------------------------------------------------

def _colwise_case(path, compact):
    """Column lengths 0-9 (cyclic) cover every tail of ColumnScalarProduct."""
    m, n = 300, 4700
    rng = np.random.default_rng(91)
    col_rows, col_vals = [], []
    for c in range(n):
        L = c % 10
        col_rows.append(np.sort(rng.choice(m, L, replace=False)))
        col_vals.append(_vals(rng, L))
    mat = Matrix(m, n, rows_from_columns(m, n, col_rows, col_vals))
    assert sorted(set(mat.col_len[:n].tolist())) == list(range(10))
    mask = random_mask(mat.N, 92)
    w = vec(m, 95)
    init = row(range(3), rho_for(m, range(3), 1), 2)
    steps = [init, colwise(vec(m, 93), None, path, compact), dots(vec(m, 94)),
             listdots(np.arange(0, mat.N, 37), vec(m, 96)),
             colwise(vec(m, 97), w, path, compact), dots(w), dots(vec(m, 98))]
    # A sparse rho: most dots are exactly 0 and are dropped (stale positions).
    sparse = np.zeros(m)
    sparse[[3, 77, 200]] = [0.5, -0.25, 0.125]
    steps += [colwise(sparse, None, path, compact), colwise(sparse, w, path, compact), dots(w)]
    return Built(mat, mask, steps)


case("column_wise_small")(functools.partial(_colwise_case, "column_wise_small", "none"))
case("column_wise_general", OFF)(functools.partial(_colwise_case, "column_wise_general", "small"))


# --- compaction and fetch ----------------------------------------------------------------------------

def _compact_case(N):
    """A dense A of four rows: an algorithm-2 row over all of them touches
    every column, so the list is the relevant set: all N columns, none, and
    column N - 1 alone."""
    m = 4
    mat = _dense_matrix(m, N - m, N, tiny_column=False)
    assert mat.N == N
    all_rows = list(range(m))
    rho = rho_for(m, all_rows, N + 1)
    rho[2] = 0.5 * rho[1] + 0.25  # rows 1 and 2 are equal: no cancellation here
    compact = "small" if N <= 16384 else "chip_wide"
    everything = np.ones(N, bool)
    nothing = np.zeros(N, bool)
    only_last = np.zeros(N, bool)
    only_last[N - 1] = True
    steps = [dict(row(all_rows, rho, 2, "full_rows", compact, mask=everything), count=N),
             dict(row(all_rows, rho, 2, "full_rows", compact, mask=nothing), count=0),
             dict(row([m - 1], rho_for(m, [m - 1], N + 2), 2, "full_rows", compact,
                      mask=only_last), count=1),
             row(all_rows, rho, 1, "full_rows", compact, mask=random_mask(N, N + 3))]
    return Built(mat, everything, steps)


for _N in (16384, 16385, 18431, 18432, 18433):
    case(f"compact_N{_N}", OFF)(functools.partial(_compact_case, _N))


@case("fetch_without_mirror", OFF)
def _():
    """Lists of 4096, 4097, 10 and 6000 columns in one sequence: the prefix of
    max(4096, 1.25 * last) and the second round trip."""
    N, m = 18000, 4
    mat = _dense_matrix(m, N - m, 101)
    rho = rho_for(m, range(m), 102)
    rho[2] = 0.5 * rho[1] + 0.25
    steps = []
    for count in (4096, 4097, 10, 6000):
        mask = np.zeros(N, bool)
        mask[np.random.default_rng(count).choice(mat.n - 1, count, replace=False)] = True
        steps.append(dict(row(range(m), rho, 2, "full_rows", "chip_wide", mask=mask, mapped=False),
                          count=count))
    return Built(mat, np.ones(N, bool), steps, setup=("no_mirror",))


@case("mixed_sequence", OFF)
def _():
    """column-wise -> algorithm 1 (list kernel) -> algorithm 0 -> algorithm 2
    (by column) -> algorithm 1: the stale-position contract across kernels."""
    m, n = 200, 19800
    pool = _pool(n, 3000, 111)
    rows = gen_rows(n, 112, [25] * m, [pool] * m)
    mat = Matrix(m, n, rows)
    assert mat.col_len.max() <= 32 and mat.N == 20000
    f30, f1, f100, f40 = list(range(30)), [50], list(range(60, 160)), list(range(10, 50))
    steps = [row(range(3), rho_for(m, range(3), 1), 2, "chunk", "chip_wide"),
             colwise(vec(m, 113), None, "column_wise_general", "chip_wide"),
             row(f30, rho_for(m, f30, 114), 1, "list", "none"),
             row(f1, rho_for(m, f1, 115), 0, "list", "none"),
             row(f100, rho_for(m, f100, 116), 2, "by_column", "chip_wide"),
             row(f40, rho_for(m, f40, 117), 1, "list", "none")]
    return Built(mat, random_mask(mat.N, 118), steps)

