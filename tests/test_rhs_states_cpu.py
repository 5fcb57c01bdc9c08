"""The state bank of tests/rhs_states.py reaches what it claims to reach -- proved with the CPU oracle and NumPy, no GPU.

tests/test_gpu_rhs_as_stepped.py compares the two instantiations of the RHS bit for bit on this bank; a branch no state
enters would pass that comparison whatever the kernel did there.  So every depth the GPU file runs is checked here for:
saturated midpoints inside and below the root zone, the water table at every targeted index and the fully saturated case
(index -1), lateral flow acting on every row type, transpiration, C clamped to epsilon at an unsaturated cell, the exact-threshold
midpoint and -- on the crafted columns: no well of the site reaches the first, only the deepest reach the second -- the
uptake's renormalisation and an uptake weight decided by the cumulative water fraction.  The counts are pinned: a change of the bank shows up here, with the row of the table to update."""
import numpy as np
import pytest

import rhs_states as rs

KEYS = ("states", "sat_in_root", "sat_below_root", "transpiring", "renormalised", "c_clamped", "no_layer_unsat",
        "cumulative_weight", "lf:night", "lf:day_dry", "lf:day_demand", "lf:rain", "lf:wet", "lf:spinup")
# (depth, crafted column): the counts of rhs_states.coverage in the order of KEYS
PINNED = {
    (193, False): (17, 13, 0, 48, 0, 4, 0, 0, 8, 8, 12, 10, 8, 8),
    (200, False): (31, 26, 0, 87, 0, 4, 0, 0, 21, 21, 25, 23, 21, 21),
    (256, False): (23, 12, 18, 54, 0, 4, 0, 0, 8, 8, 16, 10, 8, 8),
    (257, False): (19, 14, 14, 51, 0, 4, 0, 0, 10, 10, 13, 12, 10, 10),
    (300, False): (33, 27, 27, 90, 0, 4, 0, 0, 23, 23, 26, 25, 23, 23),
    (320, False): (27, 14, 22, 51, 0, 4, 0, 0, 10, 10, 20, 12, 10, 10),
    (321, False): (21, 16, 16, 57, 0, 4, 0, 0, 12, 12, 15, 14, 12, 12),
    (361, False): (21, 16, 16, 57, 0, 4, 0, 0, 12, 12, 15, 14, 12, 12),
    (384, False): (31, 16, 26, 57, 0, 4, 0, 0, 12, 12, 24, 14, 12, 12),
    (385, False): (23, 18, 18, 63, 0, 4, 0, 0, 14, 14, 17, 16, 14, 14),
    (401, False): (37, 31, 31, 102, 0, 4, 0, 0, 27, 27, 30, 29, 27, 27),
    (448, False): (35, 18, 30, 63, 0, 4, 0, 1, 14, 14, 28, 16, 14, 14),
    (513, False): (47, 22, 42, 75, 0, 4, 0, 1, 18, 18, 41, 20, 18, 18),
    (581, False): (63, 37, 57, 117, 0, 4, 0, 2, 33, 33, 56, 35, 33, 33),
    (640, False): (67, 24, 62, 78, 0, 4, 0, 2, 20, 20, 60, 32, 20, 20),
    (461, False): (25, 20, 20, 69, 0, 4, 0, 1, 16, 16, 19, 18, 16, 16),
    (300, True): (33, 27, 27, 96, 2, 4, 30, 1, 23, 23, 26, 25, 23, 23),
    (581, True): (63, 37, 57, 183, 6, 4, 60, 24, 33, 33, 56, 35, 33, 33),
}


def test_the_pinned_table_covers_every_depth_the_gpu_file_runs():
    site = {d for d, crafted in PINNED if not crafted}
    assert site == set(rs.DEPTHS_DEFAULT) | set(rs.DEPTHS_SPLIT) | {rs.DEPTH_PLAIN}
    assert set(rs.DEPTHS_GENERIC) <= site                       # generic exponents: the same banks on the same wells
    assert {d for d, crafted in PINNED if crafted} == set(rs.DEPTHS_CRAFTED)


@pytest.mark.parametrize("D,crafted", sorted(PINNED))
def test_bank_reaches_every_branch(D, crafted):
    from oracle.oracle import Oracle
    cols, forcing, rows = rs.case_column(D, crafted=crafted)
    names, Y, Z = rs.case_bank(cols)
    assert np.isfinite(Y).all() and np.isfinite(Z).all() and len(set(names)) == len(names)
    assert np.abs(Z).max() == 6.0                                        # noise entries of +-6
    by = dict(zip(names, Y))
    k = D - 2
    # ---- the water table: every targeted index, by NumPy on the midpoints and by the oracle's own search
    found = {}
    for name, y in by.items():
        j = rs.deepest_unsaturated(cols, y)
        found[name] = j
        sat_int = rs.midpoints(y)[1:D - 1] >= cols.soil.psi_sat
        assert Oracle.find_wtd(sat_int) == min(max(j, 0), k - 1), name
    targets = rs.ballot_targets(D)
    assert [found[f"wt@{j}"] for j in targets] == targets
    cpl = rs.cells_per_lane(D)
    for c in range(cpl):                                                 # lanes 0 and 1 of every cell slot; 62 and 63 where they hold midpoints
        for lane in rs.LANES:
            j = lane * cpl + c
            assert (j in targets) == (1 <= j <= D - 2), (lane, c)
    assert D - 2 in targets
    if rs.is_split(D):
        cut = rs.WAVE * rs.PAIR_CPL
        assert {cut - 2, cut - 1, cut, cut + 1} <= set(targets)
        assert {half * cut + lane * rs.PAIR_CPL + c for half in (0, 1) for lane in rs.LANES for c in range(rs.PAIR_CPL)
                if 1 <= half * cut + lane * rs.PAIR_CPL + c <= D - 2} <= set(targets)
    assert found["saturated"] == -1 and found["unsaturated"] == D - 2
    # perched: the deepest unsaturated midpoint lies below a saturated lens, with unsaturated cells in between
    sat = rs.midpoints(by["perched"]) >= cols.soil.psi_sat
    first_sat = int(np.argmax(sat[1:])) + 1
    assert first_sat + 3 < found["perched"] and not sat[first_sat + 3:found["perched"] + 1].all() and sat[found["perched"] + 1:D - 1].all()
    # ---- the threshold: the midpoint AT psi_sat is saturated, its one-ulp neighbour is not
    a = rs.threshold_node(cols)
    assert 1 <= a <= cols.n_root_int
    m_exact, m_below = rs.midpoints(by["thr_exact"])[a], rs.midpoints(by["thr_below"])[a]
    assert m_exact == cols.soil.psi_sat and m_below == np.nextafter(cols.soil.psi_sat, -np.inf)
    assert found["thr_exact"] == a - 1 and found["thr_below"] == a
    # ---- the cell model's range
    assert np.abs(by["range_down"]).min() == 1e-3 and np.abs(by["range_down"]).max() == 1e5
    # ---- what the oracle sees on the bank's rows
    cov = rs.coverage(cols, forcing, rows, names, Y, Z)
    cov["states"] = len(names)
    assert cov["sat_in_root"] >= 1 and cov["transpiring"] >= 1 and cov["c_clamped"] >= 1
    assert cov["sat_below_root"] >= 1 or cols.n_root_int == D - 2        # (the two shallowest wells are root zone throughout)
    assert all(cov[f"lf:{name}"] >= 1 for name, _, _ in rows)
    assert [name for name, _, _ in rows] == ["night", "day_dry", "day_demand", "rain", "wet", "spinup"]
    if crafted:
        assert cov["renormalised"] >= 1 and cov["no_layer_unsat"] >= 1 and cov["cumulative_weight"] >= 1
        assert (cols.noisec_mid[1:1 + cols.n_root_int] < 0).any() and (cols.noisec_mid[1 + cols.n_root_int:] < 0).any()
    assert tuple(cov[key] for key in KEYS) == PINNED[(D, crafted)], dict(zip(KEYS, (cov[key] for key in KEYS)))


def test_bank_rows_are_the_row_types():
    cols, forcing, rows = rs.case_column(300)
    r = {name: row for name, row, _ in rows}
    assert forcing.daylight[r["night"]] == 0 and forcing.precip[r["night"]] == 0.0
    assert forcing.daylight[r["day_dry"]] == 1 and forcing.precip[r["day_dry"]] == 0.0
    assert forcing.daylight[r["day_demand"]] == 1 and forcing.atm[r["day_demand"]] == 50.0 and forcing.wtd_obs[r["day_demand"]] >= cols.dim_d - 3
    assert forcing.precip[r["rain"]] > 0.0 and forcing.wet_season[r["wet"]] == 1 and forcing.wet_season[r["night"]] == 0
    assert rows[-1] == ("spinup", r["night"], True) and not forcing.refresh[[row for _, row, _ in rows]].any()


def test_conductivity_uncertainty_marks_the_cells_next_to_saturation():
    """rhs_states.conductivity_uncertainty -- where the GPU file leaves the flux uncompared.  vrettas_fung: 0 at a saturated
    cell, below 1e-13 away from saturation (1 - S_e > 1e-2, noise of +-6 included), and above a tenth of the flux tier
    (4 u > 1e-12) only at unsaturated cells with 1 - S_e < 1e-4 -- cells of the two range states, at most a quarter of
    them.  van Genuchten's K: the cell one ulp below psi_sat is marked too."""
    cols, _, _ = rs.case_column(300)
    names, Y, Z = rs.case_bank(cols)
    marked = {}
    for name, y, z in zip(names, Y, Z):
        u = rs.conductivity_uncertainty(cols, y, z)
        ym = rs.midpoints(y)
        sat = ym >= cols.soil.psi_sat
        one_minus_s = -np.expm1(-cols.soil.m * np.log1p((cols.soil.alpha * np.abs(ym)) ** cols.soil.n))
        assert u.shape == (cols.dim_d - 1,) and (u[sat] == 0.0).all() and (u[~sat] > 0.0).all()
        assert (u[~sat & (one_minus_s > 1e-2)] < 1e-13).all(), name
        big = 4.0 * u > 1e-12
        assert (one_minus_s[big] < 1e-4).all(), name
        if big.any():
            marked[name] = int(big.sum())
    assert set(marked) == {"range_down", "range_up"} and all(v <= (cols.dim_d - 1) // 4 for v in marked.values()), marked
    cols, _, _ = rs.case_column(300, model="vanGenuchten", n=2.0, lam=1.0)
    names, Y, Z = rs.case_bank(cols)
    k, a = names.index("thr_below"), rs.threshold_node(cols)
    u = rs.conductivity_uncertainty(cols, Y[k], Z[k])
    assert 4.0 * u[a] > 1e-12 and u[a + 1] == 0.0 and 4.0 * u[a - 1] < 1e-12
