"""The states of tests/rhs_pack_states.py are where they claim to be -- NumPy only, no GPU.

tests/test_gpu_rhs_pack.py compares the packed cell model of the 5-cells-per-lane step kernel with the full one bit for bit;
a state on the wrong side of the boundary would pass that comparison without entering the path it is there for.  So, at
every depth the GPU file runs (site tables and crafted ones): each state's deepest unsaturated slot is the one it claims, the
path it must take follows from it (by slot index and, independently, by the kernel's lane flags), both paths are taken on
either side of midpoint 80 with nothing in between left out, and the crafted tables put cells of no layer inside the packed
row and in the saturated zone behind it."""
import numpy as np
import pytest

import rhs_pack_states as ps
import rhs_states as rs

CASES = [(D, crafted) for D in ps.DEPTHS for crafted in (False, True)]


def test_depths_are_the_edges_and_the_middle_of_five_cells_per_lane():
    assert [rs.cells_per_lane(D) for D in ps.DEPTHS] == [ps.CPL] * 3
    assert rs.cells_per_lane(ps.DEPTHS[0] - 1) == ps.CPL - 1 and rs.cells_per_lane(ps.DEPTHS[-1] + 1) == ps.CPL + 1
    assert ps.PACK_END == 80 and set(ps.DEPTHS) <= set(rs.DEPTHS_DEFAULT)


@pytest.mark.parametrize("D,crafted", CASES)
def test_every_state_sits_where_it_claims(D, crafted):
    cols, _, _ = rs.case_column(D, crafted=crafted)
    names, Y, Z, claims = ps.pack_states(cols)
    psi_sat = cols.soil.psi_sat
    assert len(set(names)) == len(names) and np.isfinite(Y).all() and np.isfinite(Z).all()
    for name, y in zip(names, Y):
        deepest, packed = claims[name]
        assert ps.deepest_unsaturated_slot(cols, y) == deepest, name
        assert ps.takes_packed_path(cols, y) == packed == ps.takes_packed_path_by_lane(cols, y), name
        if 1 <= deepest <= D - 2:                              # ... and it is the index the lateral-flow search returns
            assert rs.deepest_unsaturated(cols, y) == deepest, name
    # every water-table index of lanes 14 .. 16, packed up to 79 and not from 80 on
    assert [claims[f"pk:wt@{j}"] for j in range(70, 85)] == [(j, j < 80) for j in range(70, 85)]
    assert claims["pk:saturated"] == (-1, True) and not claims["pk:unsaturated"][1]
    by = dict(zip(names, Y))
    # perched lens inside the packed row: saturated cells at midpoints 20 .. 28, unsaturated ones on both sides of them
    for name, below in (("pk:perched_inside", 60), ("pk:perched_across", 100)):
        sat = ps.slot_psi(cols, by[name]) >= psi_sat
        assert sat[20:29].all() and not sat[:19].any() and not sat[30:below - 1].any() and sat[below:].all(), name
    assert claims["pk:perched_inside"] == (59, True) and claims["pk:perched_across"] == (99, False)
    # the threshold at the boundary: midpoint a exactly psi_sat is saturated, one ulp lower it is not
    for a in (79, 80):
        exact, below = ps.slot_psi(cols, by[f"pk:thr_exact@{a}"]), ps.slot_psi(cols, by[f"pk:thr_below@{a}"])
        assert exact[a] == psi_sat and below[a] == np.nextafter(psi_sat, -np.inf)
        assert (exact[a + 1:] >= psi_sat).all() and (below[a + 1:] >= psi_sat).all()
    assert claims["pk:thr_exact@79"] == (78, True) and claims["pk:thr_below@79"] == (79, True)
    assert claims["pk:thr_exact@80"] == (79, True) and claims["pk:thr_below@80"] == (80, False)     # one ulp decides the path


@pytest.mark.parametrize("D,crafted", CASES)
def test_the_joint_bank_takes_both_paths(D, crafted):
    cols, _, _ = rs.case_column(D, crafted=crafted)
    names, Y, Z = ps.pack_bank(cols)
    assert len(set(names)) == len(names) and Y.shape == Z.shape == (len(names), D)
    packed = np.array([ps.takes_packed_path(cols, y) for y in Y])
    assert packed.sum() >= 16 and (~packed).sum() >= 8
    by = dict(zip(names, packed))
    assert by["saturated"] and not by["unsaturated"]            # rhs_states' own: the paths do not depend on the module
    if crafted:
        # cells of no layer (K = sat_soil): inside the packed row -- evaluated by the model -- and in the saturated zone
        # behind it, where the packed path takes K from the table
        no_layer = np.nonzero(cols.noisec_mid < 0.0)[0]
        assert ((no_layer >= 3) & (no_layer < 9)).sum() == 6 and (no_layer >= ps.PACK_END).sum() == 7
        assert no_layer.size == 13


def test_the_step_test_spreads_its_members_over_the_boundary():
    """tests/test_gpu_step_pack.py: hydrostatic columns with the water table at nodes 60 .. 100."""
    cols, _, _ = rs.case_column(300)
    Y = ps.hydrostatic_spread(cols, 512)
    packed = np.array([ps.takes_packed_path(cols, y) for y in Y])
    deepest = np.array([ps.deepest_unsaturated_slot(cols, y) for y in Y])
    assert deepest.min() <= 60 and deepest.max() >= 99 and packed.sum() >= 200 and (~packed).sum() >= 200
    assert set(range(75, 85)) <= set(deepest.tolist())          # members right at the boundary, on both sides
    from oracle.oracle import Oracle
    wtd = np.array([Oracle.find_wtd(y >= cols.soil.psi_sat) for y in Y])      # the index the stepper reports per row
    assert wtd.min() in (59, 60, 61) and wtd.max() in (99, 100, 101) and (np.abs(wtd - deepest) <= 2).all()
