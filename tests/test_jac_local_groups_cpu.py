"""The three FD-Jacobian column groups of the 5-cells-per-lane step kernel (csrc/hc_step.h, JAC3), without the kernel.

(a) The ids i % 3, formed the way the kernel forms them per lane (a chain of increments from (5 lane - 1) % 3, -1 where a node
    has no column), are a valid grouping of the tridiagonal pattern at D = 257, 300 and 320: no two columns of a group share
    a row, and the sub-, main- and super-diagonal ids of every row are those of its columns.
(b) The mathematical claim, on the independent C oracle: where the RHS is local -- night rows, and every row with ET off --
    a one-row solve with the groups i % 3 gives the state and the solver statistics of the solve with scipy's five groups,
    byte for byte.  (The oracle has no guard for the water-table search: a row on which it disagrees would show a coupling
    the kernel's guard has to cover.  None does on these members.)
(c) Daylight rows with ET on are NOT local: the kernel must keep the five groups there (that they differ on the oracle is
    printed, not asserted: it is the reason for the rule, not a property to hold)."""
import copy

import numpy as np

import rhs_pack_states as ps
from hydromodel_amd.digest import ColumnTables, ForcingDigest, group_columns_tridiagonal
from hydromodel_amd.synthetic import default_parameters, synthetic_forcing_frame, synthetic_well
from oracle.oracle import Oracle

CPL, WAVE = 5, 64
ROWS = 96           # two synthetic days
MEMBERS = 8


def kernel_ids(D):
    """gs, gp, gn per node as HC_GROUPS_FILL derives them: [64 lanes][5 slots], -1 = no column."""
    gs, gp, gn = (np.full((WAVE, CPL), -1) for _ in range(3))
    for lane in range(WAVE):
        i0 = lane * CPL
        q = [(i0 + 2) % 3]
        for k in range(1, CPL + 2):
            q.append(0 if q[-1] == 2 else q[-1] + 1)
        for c in range(CPL):
            i = i0 + c
            gs[lane, c] = q[c + 1] if i < D else -1
            gp[lane, c] = q[c] if 1 <= i < D else -1
            gn[lane, c] = q[c + 2] if i < D - 1 else -1
    return gs.reshape(-1), gp.reshape(-1), gn.reshape(-1)


def test_the_ids_are_a_valid_grouping_of_the_tridiagonal_pattern():
    for D in ps.DEPTHS:
        assert (D + WAVE - 1) // WAVE == CPL
        gs, gp, gn = kernel_ids(D)
        groups = np.arange(D) % 3
        assert (gs[:D] == groups).all() and (gs[D:] == -1).all()
        # row i stores columns i - 1, i, i + 1: their ids, -1 where the column does not exist (and in the padding)
        assert gp[0] == -1 and (gp[1:D] == groups[:-1]).all() and (gp[D:] == -1).all()
        assert (gn[:D - 1] == groups[1:]).all() and (gn[D - 1:] == -1).all()
        # no two columns of a group share a row: column j touches rows j - 1 .. j + 1
        for g in range(3):
            rows = np.zeros(D, dtype=int)
            for j in np.nonzero(groups == g)[0]:
                rows[max(j - 1, 0):min(j + 1, D - 1) + 1] += 1
            assert rows.max() == 1, (D, g)
        # the host's groups (scipy's, in its random visiting order) are five, valid as well, and another partition
        host = group_columns_tridiagonal(D)
        assert host.max() + 1 == 5 and (np.abs(np.diff(np.nonzero(host == 0)[0])) >= 3).all()


def _setup():
    params = default_parameters()
    cols = ColumnTables(params, synthetic_well(300))
    forcing = ForcingDigest(params, synthetic_forcing_frame(1), cols)
    cols3 = copy.copy(cols)
    cols3.groups = (np.arange(cols.dim_d) % 3).astype(cols.groups.dtype)
    cols3.n_groups = 3
    psi = ps.hydrostatic_spread(cols, MEMBERS)
    noise = np.random.default_rng(300).standard_normal((MEMBERS, cols.dim_d))
    return cols, cols3, forcing, psi, noise


def _solve_rows(cols, cols3, forcing, psi, noise, flags, local):
    """Members through ROWS rows on the five groups; every row is solved a second time on the three from the same state.
    -> (rows compared, rows that differ, indices of the differing rows)"""
    o5 = Oracle(cols, forcing.surface_evap, flags=flags)
    o3 = Oracle(cols3, forcing.surface_evap, flags=flags)
    compared, differ = 0, []
    for m in range(MEMBERS):
        y = psi[m].copy()
        for row in range(1, 1 + ROWS):
            r = Oracle.row(forcing.precip[row], forcing.atm[row], forcing.daylight[row], forcing.wtd_obs[row])
            y5, s5, n5, _ = o5.solve_row(r, row - 1, row, y, noise[m])
            if local(row):
                y3, s3, n3, _ = o3.solve_row(r, row - 1, row, y, noise[m])
                compared += 1
                if not (y3.tobytes() == y5.tobytes() and s3 == s5 and n3.tobytes() == n5.tobytes()):
                    differ.append((m, row))
            y = y5
    return compared, differ


def test_night_rows_give_the_same_bytes_on_three_groups_as_on_five():
    cols, cols3, forcing, psi, noise = _setup()
    night = lambda row: not forcing.daylight[row]
    compared, differ = _solve_rows(cols, cols3, forcing, psi, noise, None, night)
    assert compared == MEMBERS * ROWS // 2          # daylight is hours 6 .. 17: half of the rows
    assert not differ, f"(member, row) solved differently on the groups i % 3: {differ[:10]}"


def test_every_row_is_local_with_et_off():
    cols, cols3, forcing, psi, noise = _setup()
    compared, differ = _solve_rows(cols, cols3, forcing, psi, noise, {"ET": False}, lambda row: True)
    assert compared == MEMBERS * ROWS and not differ, f"(member, row) solved differently with ET off: {differ[:10]}"


def test_daylight_rows_with_et_are_why_the_five_groups_stay():
    cols, cols3, forcing, psi, noise = _setup()
    day = lambda row: bool(forcing.daylight[row])
    compared, differ = _solve_rows(cols, cols3, forcing, psi, noise, None, day)
    print(f"daylight rows compared on the oracle: {compared}, solved differently: {len(differ)}")
    assert compared == MEMBERS * ROWS // 2
