"""The dense tail of BTRAN's forward U^T solve (DeviceLp::DenseTailSolve,
kernels/dense_tail.hip), one solve at a time through the probe
(tests/devop_tri.py), bit for bit against tests/tri_ref.py's
TransposeUpperSolve and the host loop on the same matrix.

The triangles are tri_cases.tail_tri: 400 rows, so a dense column has at
least 50 entries, with tails of 1, 63, 64, 65 and 129 columns -- one block, a
last block of one column, and three blocks. Their columns hold prefixes below
the tail of exactly 64 j and 64 j + 4 entries (the advance ends on and just
past a 64-entry step), every length remainder of the groups of four, a tail
row inside the first group with more than 72 entries behind it (the finish
reads past its staged entries), rows out of order, and a column of exactly 50
entries next to one of 49 (where the tail starts). last_tri states t, T and
the blocks of every solve.
"""
import functools
import itertools

import numpy as np
import pytest

import devop
import devop_tri
import tri_cases as tc
from test_tri_ops_gpu import SWITCHES, reference, same_bits
from tri_ref import UPPER_T_UP

pytestmark = pytest.mark.gpu

TAIL = {"MILP_DEVICE_SOLVE": "force", "MILP_TRI_BTRAN": "1", "MILP_DENSE_TAIL": "1",
        "MILP_DENSE_TAIL_MIN_COLS": "1", "MILP_DENSE_TAIL_MIN_ENTRIES": "1"}


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
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
def _cached_handle(env):
    return devop_tri.TriDevOp()


def handle(env, monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    return _cached_handle(tuple(sorted(env.items())))


_keys = itertools.count(5000)


def solve_twice(d, t, first, T, seed, tail=True):
    """Two right-hand sides under one key; the record of each."""
    d.tri_set_matrix(t)
    key = next(_keys)
    rng = np.random.default_rng(seed)
    for rep in range(2):
        x = tc.dense_rhs(rng, t.n)
        ref, open_ = reference(UPPER_T_UP, t, x)
        on, got = d.tri_solve(UPPER_T_UP, key, x)
        rec = d.last_tri()
        print(rec)
        assert on, rec
        what = f"tail n={t.n} T={T} vector {rep}"
        same_bits(got, ref, what, None if tail else open_)
        same_bits(d.tri_host_solve(UPPER_T_UP, x), ref, what + " (host loop)")
        if tail:
            assert rec["plan"] == "dense_tail", rec
            assert (rec["rows"], rec["t"], rec["tail_cols"], rec["blocks"]) == \
                (t.n, first, T, (T + 63) // 64), rec
            assert rec["first_col"] == t.first_non_identity and rec["top"] == t.n - 1, rec
            assert rec["entries"] == int(t.starts[t.n] - t.starts[first]), rec
        else:
            assert rec["plan"] == "sync_free" and rec["kind"] == "upper_t_up", rec


@pytest.mark.parametrize("identity", [False, True], ids=["sparse_head", "identity_head"])
@pytest.mark.parametrize("unit", [False, True], ids=["diag", "unit"])
@pytest.mark.parametrize("T", tc.TAIL_COLS)
def test_dense_tail(T, unit, identity, monkeypatch):
    d = handle(TAIL, monkeypatch)
    for offset in range(len(tc.TAIL_VARIANTS) if T == 1 else 2):
        t, first, used = tc.tail_tri(T, unit, identity, offset)
        assert first == t.n - T and (not identity or t.first_non_identity == first)
        solve_twice(d, t, first, T, 100 * T + offset)


def test_key_change_to_a_larger_tail_and_back(monkeypatch):
    """The staging buffers grow with n and T, and the smaller tail then runs
    in the larger buffers."""
    d = handle(TAIL, monkeypatch)
    small = tc.tail_tri(63, False)
    large = tc.tail_tri(129, False, n=500, seed=3)
    for t, first, _ in (small, large, small, large):
        solve_twice(d, t, first, t.n - first, t.n)


@pytest.mark.parametrize("env", [{"MILP_DENSE_TAIL": "0"}, {"MILP_DENSE_TAIL_MIN_COLS": "130"},
                                 {"MILP_DENSE_TAIL_MIN_ENTRIES": "1000000"}],
                         ids=["off", "too_few_columns", "too_few_entries"])
def test_without_the_dense_tail_the_ordinary_path_gives_the_same_bits(env, monkeypatch):
    d = handle(dict(TAIL, **env), monkeypatch)
    for unit in (False, True):
        t, first, _ = tc.tail_tri(129, unit)
        solve_twice(d, t, first, 129, 7, tail=False)
