"""The panel cases (tests/panel_cases.py) can tell summation orders apart, and
have the shapes their kernels need. Reference only: no engine, no GPU.

A bit-for-bit comparison shows nothing if every order gives the same bits.
Over the results of columns with at least 8 entries (two terms per chain), a
plain left-to-right sum must change at least a quarter and the fold
(r1 + r2) + (r3 + r4) at least a tenth. dense5 has no such column.
"""
import numpy as np
import pytest

import panel_cases as pc
from device_ref import bits

K = 5


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_orders_are_distinguishable(name):
    mat = pc.matrix(name)
    long_cols = np.nonzero(mat.col_len >= 8)[0]
    if name == "dense5":
        assert len(long_cols) == 0
        return
    assert len(long_cols) >= 8
    ref = pc.reference(name)[:K][:, long_cols]
    for order, least in (("sequential", 0.25), ("pairwise", 0.10)):
        other = pc.other_order(name, K, order)[:, long_cols]
        changed = np.mean(bits(other) != bits(ref))
        print(name, order, f"{changed:.3f}")
        assert changed >= least, (name, order, changed)


def test_vectors_hold_both_zeros():
    for name in pc.CASES:
        y = pc.vectors(name)
        zero = y == 0.0
        neg = zero & np.signbit(y)
        assert 0.05 < np.mean(zero & ~neg) < 0.15, name
        assert 0.005 < np.mean(neg) < 0.04, name
        assert y.shape == (pc.MAX_K, pc.CASES[name][0])


def test_shapes_meet_their_kernels_preconditions():
    # DeviceLp takes the long-column kernel when the CSC columns it visits
    # average at least 32 entries; with a dense block those are the others.
    quad, wave = pc.matrix("quad"), pc.matrix("wave")
    assert quad.col_len.mean() < 32 and abs(quad.col_len.mean() - 6.9) < 0.1
    assert wave.col_len.mean() >= 32 and abs(wave.col_len.mean() - 36.8) < 0.1
    assert set(pc.QUAD_LENS) <= set(quad.col_len) and set(pc.WAVE_LENS) <= set(wave.col_len)
    for m in pc.DENSE_ROWS:
        mat = pc.matrix(f"dense{m}")
        full = mat.col_len[:mat.n] == m
        assert full.sum() == 70 and 64 < full.sum() < 128
        assert mat.col_len[~np.concatenate([full, np.zeros(m, bool)])].mean() < 32
    assert sorted(m % 4 for m in pc.DENSE_ROWS) == [0, 1, 1, 2, 3]
    assert {(m // 4) % 2 for m in pc.DENSE_ROWS} == {0, 1}


def test_empty_and_slack_columns():
    mat, y, ref = pc.matrix("quad"), pc.vectors("quad"), pc.reference("quad")
    empty = np.nonzero(mat.col_len == 0)[0]
    assert len(empty) and np.all(bits(ref[:, empty]) == 0)  # +0.0
    slack = np.arange(mat.n, mat.N)
    assert np.array_equal(bits(ref[:, slack]), bits(0.0 + y))  # -0.0 becomes +0.0
