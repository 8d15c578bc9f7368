"""The inputs of tests/test_panel_sparse_gpu.py, checked on the reference
alone: every (case, mask, tolerance) must make the filter do something, or a
kernel that keeps everything, nothing, or the wrong side of a tie would pass.

These are conditions on tests/panel_sparse_cases.py, not measurements of the
engine. For every case, the masks all / structural / random and every vector
the case uses:
  * tolerance 0 drops at least one masked entry (a +-0.0 dot) and keeps at
    least one. The dropped entry is asserted wherever the mask holds a slack
    column or an empty structural column; the structural mask of the dense
    cases holds neither (every structural column there has entries), so a
    drop is not required of it;
  * the median tolerance keeps between 30 % and 70 % of the masked entries;
  * +inf keeps nothing;
  * t* and nextafter(t*, 0) keep different numbers of entries: t* drops its
    anchor entry, the next smaller double keeps it.
"""
import numpy as np
import pytest

import panel_sparse_cases as sc

FILTER_MASKS = ("all", "structural", "random")


def test_long_case_is_built_for_the_assumed_geometry():
    m, n = sc.CASES["long"][:2]
    N = m + n
    assert sc.satisfies_geometry(N, sc.TILE_COLUMNS, sc.OFFSETS_STEP_TILES)
    assert sc.CASES["long"][3] <= 5
    assert sc.matrix("long").N == N and sc.reference("long").shape == (sc.CASES["long"][3], N)


def test_edge_case_is_smaller_than_a_tile():
    mat = sc.matrix("edge")
    assert (mat.m, mat.n, mat.N) == (37, 100, 137)
    assert mat.N % 64 != 0 and mat.N < sc.TILE_COLUMNS
    assert max(sc.column_lengths("edge")) <= mat.m


@pytest.mark.parametrize("which", sc.MASKS)
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_masks(name, which):
    mat, b = sc.matrix(name), sc.mask(name, which)
    want = {"all": mat.N, "structural": mat.n, "none": 0, "last": 1, "first": 1}
    if which == "random":
        assert 0.35 * mat.N < b.sum() < 0.65 * mat.N
    else:
        assert b.sum() == want[which]
    if which == "last":
        assert b[mat.N - 1]
    if which == "first":
        assert b[0]


@pytest.mark.parametrize("which", FILTER_MASKS)
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_every_vector_meets_the_filter_conditions(name, which):
    mat, ref, b = sc.matrix(name), sc.reference(name), sc.mask(name, which)
    tol = sc.tolerances(name, which)
    assert set(tol) == set(sc.TOLERANCES)
    a = np.abs(ref[:, b])  # (vectors, masked columns)
    masked = a.shape[1]
    kept0 = (a > 0.0).sum(axis=1)
    has_zero_dot_column = b[mat.n:].any() or (mat.col_len[:mat.n][b[:mat.n]] == 0).any()
    if has_zero_dot_column:
        assert np.all(masked - kept0 >= 1), (name, which, "tolerance 0 drops nothing")
    else:
        assert which == "structural" and name.startswith("dense")
    assert np.all(kept0 >= 1)
    share = (a > tol["median"]).sum(axis=1) / masked
    assert np.all((share >= 0.3) & (share <= 0.7)), (name, which, share.min(), share.max())
    assert (a > tol["inf"]).sum() == 0
    j0, c0 = sc.anchor(name, which)
    assert b[c0] and ref[j0, c0] != 0.0 and tol["tstar"] == abs(ref[j0, c0])
    assert 0.0 <= tol["below_tstar"] < tol["tstar"]
    assert not abs(ref[j0, c0]) > tol["tstar"] and abs(ref[j0, c0]) > tol["below_tstar"]
    assert (a > tol["below_tstar"]).sum() - (a > tol["tstar"]).sum() >= 1


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_filtered_reference_is_a_sorted_sparse_form_of_the_dense_one(name):
    ref = sc.reference(name)[:3]
    for which in sc.MASKS:
        for t in sc.tolerances(name, which).values():
            starts, cols, vals = sc.filtered(ref, sc.mask(name, which), t)
            assert starts[0] == 0 and starts[-1] == len(cols) == len(vals)
            for j in range(len(ref)):
                c = cols[starts[j]:starts[j + 1]]
                assert np.all(np.diff(c) > 0)
                assert np.array_equal(vals[starts[j]:starts[j + 1]], ref[j][c])
