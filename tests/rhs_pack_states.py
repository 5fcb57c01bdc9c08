"""States for the packed cell model of the 5-cells-per-lane step kernel (csrc/hc_device.h, rhs_eval: HC_MODEL_PACK).

The kernel holds midpoint j in lane j // 5, slot j % 5.  An evaluation takes the packed path when no lane >= 16 holds an
unsaturated cell (psi < psi_sat) -- the virtual top-node cell in lane 63's last slot does not count -- i.e. when every
unsaturated midpoint has an index below PACK_END = 16 lanes x 5 cells = 80.  The slots behind the last midpoint count like
any other: slot D - 1 evaluates 0.5 (psi[D - 1] + 0), the padding slots psi = 0.

`pack_bank` adds, to the bank of tests/rhs_states.py, the states that sit on both sides of that boundary; every entry
carries the deepest unsaturated midpoint it claims and the path it must take (tests/test_rhs_pack_states_cpu.py proves both
with NumPy; tests/test_gpu_rhs_pack.py runs the kernels on them)."""
import numpy as np

import rhs_states as rs

CPL = 5
PACK_LANES = 16
PACK_END = PACK_LANES * CPL        # 80: the first midpoint index outside the packed row
DEPTHS = (257, 300, 320)           # the edges and the middle of 5 cells per lane
WT_TARGETS = tuple(range(70, 85))  # lane 14's and 15's five slots, lane 16's, the boundary itself
FLAG_SETS = {k: rs.FLAG_SETS[k] for k in ("default", "no_et", "no_lf", "hlift")}


def slot_psi(cols, y):
    """[64 * 5 - 1]: the pressure head every cell slot but the top-node cell's evaluates, in midpoint order."""
    D = cols.dim_d
    assert rs.cells_per_lane(D) == CPL
    n = rs.WAVE * CPL
    ext = np.zeros(n + 1)
    ext[:D] = y
    return 0.5 * (ext[:-1] + ext[1:])[:n - 1]


def deepest_unsaturated_slot(cols, y):
    """Index of the deepest slot below psi_sat (midpoint 0 and the slots behind the last midpoint included), or -1."""
    idx = np.nonzero(~(slot_psi(cols, y) >= cols.soil.psi_sat))[0]
    return int(idx[-1]) if idx.size else -1


def takes_packed_path(cols, y):
    return deepest_unsaturated_slot(cols, y) < PACK_END


def takes_packed_path_by_lane(cols, y):
    """The same decision the way the kernel forms it: a flag per lane, any lane >= 16 set -> the full evaluation."""
    unsat = ~(slot_psi(cols, y) >= cols.soil.psi_sat)
    unsat = np.append(unsat, False).reshape(rs.WAVE, CPL)       # [lane][slot]; lane 63's last slot: the top-node cell
    return not unsat[PACK_LANES:].any()


def perched(cols, lens, below):
    """Unsaturated column with a saturated lens at nodes [lens[0], lens[1]) and saturated from node `below` on."""
    D, dz = cols.dim_d, cols.dz
    y = np.full(D, -80.0) - 0.3 * dz * np.arange(D)
    y[lens[0]:lens[1]] = 5.0 + 0.2 * dz * np.arange(lens[1] - lens[0])
    y[below:] = 2.0 + 1.2 * dz * np.arange(D - below)
    return y


def threshold(cols, a, v):
    """rhs_states' thr_* profile with the threshold midpoint at a: nodes a and a + 1 at v, saturated below."""
    D, dz = cols.dim_d, cols.dz
    y = np.full(D, -40.0) - 0.1 * dz * np.arange(D)
    y[a:a + 2] = v
    y[a + 2:] = 3.0 + 1.1 * dz * np.arange(D - a - 2)
    return y


def pack_states(cols, seed=0):
    """-> (names, Y, noise, claims): claims[name] = (deepest unsaturated slot, takes the packed path)."""
    D, psi_sat = cols.dim_d, cols.soil.psi_sat
    rng = np.random.default_rng(2000 + D + seed)
    names, Y, Z, claims = [], [], [], {}

    def add(name, y, deepest, packed, noise=None):
        names.append(name)
        Y.append(np.asarray(y, dtype=float))
        Z.append(rng.standard_normal(D) if noise is None else noise)
        claims[name] = (deepest, packed)

    for j in WT_TARGETS:
        add(f"pk:wt@{j}", rs.water_table_at(cols, j), j, j < PACK_END)
    add("pk:saturated", 10.0 + 0.1 * cols.dz * np.arange(D), -1, True)
    from hydromodel_amd.ensemble import pressure_head
    fc_psi, _ = pressure_head(cols, 0.5 * (cols.wlt_node + cols.fc_node))
    # (slot D - 1 evaluates half the last node's head; at D = 320 it is the top-node cell's and does not count)
    add("pk:unsaturated", fc_psi, min(D - 1, rs.WAVE * CPL - 2), False)
    add("pk:perched_inside", perched(cols, (20, 30), 60), 59, True)
    add("pk:perched_across", perched(cols, (20, 30), 100), 99, False)
    below = np.nextafter(psi_sat, -np.inf)
    for a in (PACK_END - 1, PACK_END):
        for tag, v in (("exact", psi_sat), ("below", below)):
            noise = rng.standard_normal(D)
            noise[a - 3:a + 4] = 0.0                         # (rhs_states: the noise term next to saturation)
            # exact: midpoint a IS psi_sat, so saturated, and a - 1 is the deepest unsaturated one; below: a is
            deepest = a - 1 if tag == "exact" else a
            add(f"pk:thr_{tag}@{a}", threshold(cols, a, v), deepest, deepest < PACK_END, noise)
    return names, np.array(Y), np.array(Z), claims


def hydrostatic_spread(cols, n, first=60.0, last=100.0):
    """[n][D]: hydrostatic columns whose water tables stand evenly spread between nodes `first` and `last`."""
    w = np.linspace(first, last, n)
    return cols.z[None, :] - (cols.z[0] + w[:, None] * cols.dz)


def pack_bank(cols):
    """The bank of rhs_states (its coverage conditions hold on it) followed by the states above."""
    n0, Y0, Z0 = rs.case_bank(cols)
    n1, Y1, Z1, _ = pack_states(cols)
    return list(n0) + list(n1), np.concatenate([Y0, Y1]), np.concatenate([Z0, Z1])
