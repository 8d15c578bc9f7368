"""Inputs of the panel tests (DeviceLp::ColumnDotsPanel): matrices whose
column lengths sit at the limits of each panel kernel, and vectors that tell
summation orders apart.

TEST INFRASTRUCTURE ONLY. Matrix values and vector entries are
+-2^e (1 + u), e uniform in [-12, 12], u uniform in [0, 1): sums of such
products round differently in different orders. About 10 % of the vector
entries are +0.0 and about 2 % are -0.0.

  quad      m = 96, n = 160, column lengths cycle through QUAD_LENS; with the
            slacks the average is below 32: the short-column kernel.
  wave      m = 200, n = 96, lengths cycle through WAVE_LENS; the average is
            at least 32: the long-column kernel.
  dense{m}  m in DENSE_ROWS (odd and even step counts, tails of 0 to 3 rows),
            n = 80: seven of every eight columns are full (70 dense columns:
            two 64-column workgroups, the second partial), the eighth has
            min(m, 2) entries. Run with MILP_DENSE_BLOCK=force.
"""
import functools

import numpy as np

from device_ref import Matrix, column_scalar_products

QUAD_LENS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33)
WAVE_LENS = (0, 3, 4, 63, 64, 65, 67, 127, 128, 129, 131, 200, 200, 200, 200, 200)
DENSE_ROWS = (5, 8, 13, 18, 23)
MAX_K = 33  # vectors per case: two full panels and a panel of one

# name -> (m, n, environment)
CASES = {"quad": (96, 160, {}), "wave": (200, 96, {})}
for _m in DENSE_ROWS:
    CASES[f"dense{_m}"] = (_m, 80, {"MILP_DENSE_BLOCK": "force"})


def _values(rng, k):
    e = rng.integers(-12, 13, k)
    sign = np.where(rng.random(k) < 0.5, -1.0, 1.0)
    return sign * np.ldexp(1.0 + rng.random(k), e)


def column_lengths(name):
    m, n, _ = CASES[name]
    if name == "quad":
        return [QUAD_LENS[c % len(QUAD_LENS)] for c in range(n)]
    if name == "wave":
        return [WAVE_LENS[c % len(WAVE_LENS)] for c in range(n)]
    return [min(m, 2) if c % 8 == 7 else m for c in range(n)]


@functools.lru_cache(maxsize=None)
def matrix(name):
    m, n, _ = CASES[name]
    rng = np.random.default_rng(1000 + sorted(CASES).index(name))
    per_row = [([], []) for _ in range(m)]
    for c, length in enumerate(column_lengths(name)):
        rows = np.sort(rng.choice(m, length, replace=False))
        for r, x in zip(rows, _values(rng, length)):
            per_row[r][0].append(c)
            per_row[r][1].append(x)
    mat = Matrix(m, n, [(np.array(c, np.int32), np.array(x, np.float64)) for c, x in per_row])
    assert list(np.diff(mat.col_starts)) == column_lengths(name)
    return mat


@functools.lru_cache(maxsize=None)
def vectors(name):
    """(MAX_K, m), read-only."""
    m = CASES[name][0]
    rng = np.random.default_rng(2000 + sorted(CASES).index(name))
    y = _values(rng, MAX_K * m)
    kind = rng.random(MAX_K * m)
    y[kind < 0.10] = 0.0
    y[(kind >= 0.10) & (kind < 0.12)] = -0.0
    y = y.reshape(MAX_K, m)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def reference(name):
    """(MAX_K, N): ColumnScalarProduct of every column of [A | I] with every
    vector (tests/device_ref.py), computed once and read-only."""
    mat = matrix(name)
    cols = np.arange(mat.N)
    out = np.stack([column_scalar_products(mat, cols, y) for y in vectors(name)])
    out.setflags(write=False)
    return out


def other_order(name, k, order):
    """The same dots of the first k vectors summed in another order (the
    rounding of each product is the same): "sequential" = left to right,
    "pairwise" = the four chains folded as (r1 + r2) + (r3 + r4)."""
    mat = matrix(name)
    y = vectors(name)[:k]
    out = np.zeros((k, mat.N))
    for c in range(mat.N):
        s, e = mat.starts[c], mat.starts[c + 1]
        prod = mat.c_vals[s:e][None, :] * y[:, mat.c_rows[s:e]]  # (k, len)
        length = e - s
        if order == "sequential":
            res = np.zeros(k)
            for t in range(length):
                res = res + prod[:, t]
        else:
            r = [np.zeros(k) for _ in range(4)]
            full = (length // 4) * 4
            for t in range(full):
                r[t % 4] = r[t % 4] + prod[:, t]
            res = (r[0] + r[1]) + (r[2] + r[3])
            for t in range(full, length):
                res = res + prod[:, t]
        out[:, c] = res
    return out
