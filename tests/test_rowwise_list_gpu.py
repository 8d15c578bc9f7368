"""Hypersparse update rows emitted straight as their list (row_wise_list_kernel)
and the list consumers launched at the list's bound, against the CPU oracle.

Every case is a whole solve compared bit for bit (parity_util.compare) with
the small fused kernels off and the dual device mode forced, so that the
update row, the dual ratio test and the reduced-cost update run on the
general kernels this change touches. MILP_ROWWISE_LIST=off is the flag
kernels + compaction the list kernel replaces; both must equal the oracle."""
import functools

import pytest

from mi_glop import abi, engine

import kat_lps
import lp_gen
import oracle_lib
import parity_util

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _c5(m, n, per_col, seed):
    return lp_gen.sparse_c5_lp(m, n, per_col, seed)


@functools.lru_cache(maxsize=None)
def _oracle(m, n, per_col, seed, dual):
    """The reference of one LP, solved once and shared by its cases."""
    o = oracle_lib.OracleLp(abi.default_params(use_dual_simplex=dual))
    o.load(_c5(m, n, per_col, seed))
    return o, o.solve()


def _engine(lp, dual):
    g = engine.LpHandle(abi.default_params(use_dual_simplex=dual))
    g.load(lp)
    return g, g.solve()


def _switches(monkeypatch, **env):
    monkeypatch.setenv("MILP_SMALL_FUSED", "off")
    monkeypatch.setenv("MILP_DEVICE_DUAL", "force")
    for name in ("MILP_ROWWISE_LIST", "MILP_ROWWISE_LIST_MAX_ENTRIES",
                 "MILP_DUAL_RATIO_ONE_WG_MAX"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        if value is not None:
            monkeypatch.setenv(name, value)


def _row_stats(g):
    st = g.kernel_stats()
    launches = st["update_row"]["launches"] + st["single_row"]["launches"]
    nbytes = st["update_row"]["bytes"] + st["single_row"]["bytes"]
    print("update_row", st["update_row"], "single_row", st["single_row"],
          "dual_ratio", st["dual_ratio"])
    return launches, nbytes


@pytest.mark.parametrize("list_switch", [None, "off"])
@pytest.mark.parametrize("dual", [1, 0])
@pytest.mark.parametrize("seed", [41, 42, 43])
def test_duplicate_columns_across_rows(seed, dual, list_switch, monkeypatch):
    """Rows of ~135 entries over 2000 columns: a column often sits in two
    filtered rows, so runs of equal columns are folded in filtered-row order.
    The primal parametrization reads the list through the mapped mirrors
    (FetchUpdateRow) instead of the device ratio test."""
    _switches(monkeypatch, MILP_ROWWISE_LIST=list_switch)
    lp = _c5(120, 2000, 8, seed)
    o, ro = _oracle(120, 2000, 8, seed, dual)
    g, rg = _engine(lp, dual)
    parity_util.compare(o, ro, g, rg, lp)
    launches, _ = _row_stats(g)
    assert launches > 0


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_list_and_chunk_kernels_in_one_solve(seed, monkeypatch):
    """With the entry cap at 64 a solve alternates between the list kernel
    (single rows, about 60 entries here) and the chunk kernel (everything
    longer), so d_coeff_'s stale-position contract is crossed both ways. The
    same LP three ways: the launch counts agree, and the byte model orders
    them (the list path drops the 9 N term), which shows both paths ran."""
    m = 300 + 50 * (seed % 3)
    lp = _c5(m, 3000, 6, seed)
    o, ro = _oracle(m, 3000, 6, seed, 1)
    got = {}
    for name, env in (("default", {}),
                      ("cap64", {"MILP_ROWWISE_LIST_MAX_ENTRIES": "64"}),
                      ("off", {"MILP_ROWWISE_LIST": "off"})):
        _switches(monkeypatch, **env)
        g, rg = _engine(lp, 1)
        parity_util.compare(o, ro, g, rg, lp)
        got[name] = _row_stats(g)
    assert got["default"][0] == got["cap64"][0] == got["off"][0] > 0, got
    assert got["default"][1] < got["cap64"][1] < got["off"][1], got


@pytest.mark.parametrize("one_wg_max", [None, "0"])
@pytest.mark.parametrize("seed", [51, 52])
def test_bound_above_one_scan_tile(seed, one_wg_max, monkeypatch):
    """Rows of ~600 entries: four filtered rows already bound the list above
    one scan tile (2048 slots). Once through the one-workgroup ratio test,
    once (cap 0) through the two ratio kernels at a bound-sized grid."""
    _switches(monkeypatch, MILP_DUAL_RATIO_ONE_WG_MAX=one_wg_max)
    lp = _c5(200, 20000, 6, seed)
    o, ro = _oracle(200, 20000, 6, seed, 1)
    g, rg = _engine(lp, 1)
    parity_util.compare(o, ro, g, rg, lp)
    launches, _ = _row_stats(g)
    assert launches > 0
    assert g.kernel_stats()["dual_ratio"]["launches"] > 0


@pytest.mark.parametrize("builder", kat_lps.ALL, ids=lambda f: f.__name__)
@pytest.mark.parametrize("list_switch", [None, "off"])
def test_known_answer_single_row_and_empty_list(builder, list_switch, monkeypatch):
    """The known-answer LPs (a handful of rows): single-row update rows
    (algorithm 0) and update rows whose list comes out empty."""
    _switches(monkeypatch, MILP_ROWWISE_LIST=list_switch)
    lp, _ = builder()
    p = abi.default_params(use_dual_simplex=1)
    o, ro, g, rg = parity_util.solve_both(lp, p, engine.LpHandle)
    parity_util.compare(o, ro, g, rg, lp)
    _row_stats(g)
