"""`rhs_eval` with its latency chains side by side (csrc/hc_device.h, HC_RHS_ILP: the step kernel of 5 cells per lane with
default exponents and its step RHS hook) against the plain instantiation, BIT FOR BIT.

`hc_rhs_ex` variant "step" runs the step kernel's own instantiation of rhs_eval, which carries the change; variant
"hook_layout" the plain one, which does not.  HC_RHS_ILP only moves independent instructions -- the five divisions of the
assembly of dy/dt line by line across the cells (every cell with fast_div's operations and operands), the first-midpoint ET
call's table reads ahead of the interior call, the interior call's table reads back to back -- so dy/dt, c, s, f, pL and both
diagnostics must be the same bytes (LAB_NOTES.md §43).

Depths: 257, 300, 320 -- the shallowest, the bench's and the deepest column of 5 cells per lane.
States: the bank of tests/rhs_states.py (saturated, unsaturated, wet root zones, perched, threshold midpoints, ...) followed by
those of tests/rhs_pack_states.py (water tables at every midpoint 70 .. 84, both sides of the lane-15/16 boundary: the packed and
the full cell model; a saturated column) and a dry column (theta at the residual water content: no water above the wilting
point, the ET interior call's `water_k <= 0` side).
Rows: the bank's night, daylight (dry, water-limited demand, wet season), rain and spin-up rows.
Runs, each with host noise and with Philox noise: the default flags, ET off, HLIFT on, `n_root_first` = 0 and 1, `n_root_int` = 0;
all of it on the site's tables and on rhs_states.crafted_column's (a root density 1000 times the site's: `tot_x > 1`, the
renormalisation branch -- tests/test_rhs_states_cpu.py proves that on the CPU at D = 300).

Nothing here steps a row or builds a library; a case takes a few seconds."""
import copy

import numpy as np
import pytest

import rhs_pack_states as ps
import rhs_states as rs
import test_gpu_rhs_as_stepped as base

pytestmark = pytest.mark.gpu

# (name, flags, n_root_first, n_root_int): None = as the column has it
RUNS = (("default", None, 1, None), ("no_et", {"ET": False}, 1, None), ("hlift", {"HLIFT": True}, 1, None),
        ("no_first", None, 0, None), ("no_interior", None, 1, 0), ("hlift_no_first", {"HLIFT": True}, 0, None))


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("these tests need a GPU")
    import __graft_entry__ as ge
    ge.build()
    from hydromodel_amd import stepper
    return stepper


def _bank(cols):
    names, Y, Z = ps.pack_bank(cols)
    D = cols.dim_d
    dry = np.full(D, -1.0e8) - cols.dz * np.arange(D)
    rng = np.random.default_rng(4300 + D)
    names = list(names) + ["ilp:dry"]
    Y, Z = np.concatenate([Y, dry[None]]), np.concatenate([Z, rng.standard_normal((1, D))])
    # what the bank must contain: both sides of the packed row's boundary, a saturated column
    _, Yp, _, claims = ps.pack_states(cols)
    packed = [p for _, p in claims.values()]
    assert any(packed) and not all(packed)
    assert {ps.PACK_END - 2, ps.PACK_END - 1, ps.PACK_END, ps.PACK_END + 1} <= {rs.deepest_unsaturated(cols, y) for y in Yp}
    assert any((rs.midpoints(y) >= cols.soil.psi_sat).all() for y in Y)
    return names, Y, Z


@pytest.mark.parametrize("crafted", (False, True), ids=("site", "crafted"))
@pytest.mark.parametrize("D", ps.DEPTHS)
def test_step_variant_against_plain(gpu, D, crafted):
    cols0, forcing, rows = rs.case_column(D, crafted=crafted)
    assert rs.cells_per_lane(D) == ps.CPL and cols0.n_root_first == 1 and cols0.n_root_int > 0
    assert {r for r, _, _ in rows} >= {"night", "day_dry", "day_demand", "wet", "spinup"}
    names, Y, Z = _bank(cols0)
    k_dry, k_wet = names.index("ilp:dry"), names.index("wet_roots")
    cases = 0
    for run, flags, n_first, n_int in RUNS:
        cols = copy.copy(cols0)
        cols.n_root_first = n_first
        cols.n_root_int = cols0.n_root_int if n_int is None else n_int
        st = gpu.EnsembleStepper(cols, forcing, len(names), flags=flags)
        st.set_state(Y)
        for noise in ("host", "philox"):
            if noise == "host":
                st.set_noise_host(Z)
            else:
                st.set_noise_philox(43 + D, 0)
            for rname, row, spin in rows:
                where = f"D = {D}{', crafted tables' if crafted else ''}, run {run}, {noise} noise, row {rname}"
                step, hook = base._evaluate(st, row, spin, "step"), base._evaluate(st, row, spin, "hook_layout")
                base._same_bytes(step, hook, where, names)
                for q in base.QUANTITIES:
                    assert np.isfinite(step[q]).all(), (where, q)
                cases += 1
                if rname == "day_demand" and noise == "host":
                    # the branches the run is there for were taken: uptake in the interior call where it is on, none in the
                    # dry column (diag[0]: the interior call's transpiration)
                    et = (flags or {}).get("ET", True)
                    assert (step["diag"][k_wet, 0] > 0.0) == (et and cols.n_root_int > 0), where
                    assert step["diag"][k_dry, 0] == 0.0, where
        st.close()
    assert cases == len(RUNS) * 2 * len(rows)
