"""`rhs_eval`'s reads asked for early and together (csrc/hc_device.h, HC_RHS_ILP bits 16 .. 512: the step kernel of 5 cells per
lane with default exponents and its step RHS hook), at the shapes where those parts in particular can go wrong.  BIT FOR BIT.

The parts move reads, never arithmetic: the column parameters of one evaluation in one scalar-memory round trip (16), the
packed cell model's table values and the saturated rows' constants in one group (32), the assembly's five table values ahead
of the top boundary (64), the lateral-flow block's water-table search ahead of evapo-transpiration (128), hydraulic lift's five
table values ahead of its per-lane conditions (512).  LAB_NOTES.md section 45 says which of them the shipped build carries;
the tests below hold for any subset.

(1) Parameters read early: a two-point sweep in one handle at D = 300 (both points default exponents, different a0 and
    psi_sat, 64 members each, 48 rows) against each point's stand-alone handle: states, noise scales, moments, water-table
    indices, solver statistics.  A read hoisted past the point switch would give one point the other's parameters.
    A third case puts a predictive point next to a monitoring-mode one: the launch then runs the PREDICT instantiation,
    the monitoring-mode point with flag_predict off -- the one setting of (2)'s list the RHS hook cannot reach (it serves
    one point, and a single monitoring-mode point selects the monitoring-mode build).
(2) `hc_rhs_ex` variant "step" against "hook_layout" by bytes at D = 257, 300, 320 on the banks of tests/rhs_states.py and
    tests/rhs_pack_states.py plus a dry column (tests/test_gpu_rhs_ilp.py's bank), in the settings that file does not
    cross: HYDROCOL_MODEL_PACK=0 (the full cell model with the packed path's early reads never issued), the PREDICT
    instantiation with flag_predict on, LF off, ET off, HLIFT on (night rows: the lift runs; daylight rows: it does
    not), n_root_first 0 / 1; every evaluation with R.diag on (the diagnostic sums).
(3) The search ahead of ET: states whose estimated water table lies above, at and below the observed one and a column with
    no unsaturated midpoint (jstar < 0), on daylight rows with ET on: the sink and diag_lf against "hook_layout".
(4) Stepped: 128 members around the packed/full boundary (tests/test_gpu_step_pack.py's construction) through 48 rows at
    D = 300 with HLIFT on, against the same run on a build of this unit with -DHC_RHS_ILP=13 (the parts of section 43 alone),
    which the test compiles itself as tests/test_gpu_two_layout.py compiles its variants: states, noise scales, moments,
    water-table indices, solver statistics, failed attempts and counters.

`python tests/test_gpu_rhs_waits.py <library> <out.npz>` runs (4)'s case on another library (the test starts it)."""
import copy
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
D_BENCH, ROWS = 300, 48
ARRAYS = ("psi", "noise_scale", "moments", "wtd", "stats", "failed")
COUNTED = ("jac_retry", "failed_attempts", "guard_trips")     # (guard_last_*: the last writer among the waves wins, run by run)


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("these tests need a GPU")
    import __graft_entry__ as ge
    ge.build()
    from hydromodel_amd import stepper
    return stepper


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        k = np.unravel_index(int(np.nonzero(a.reshape(-1) != b.reshape(-1))[0][0]), a.shape)
        raise AssertionError(f"{what}{list(k)}: {a[k]!r} against {b[k]!r}; {int((a != b).sum())} of {a.size} entries differ")


# ------------------------------------------------------------------------------------------------ (1) the point switch
MPP = 64
SWEEPS = {"a0_psi_sat": ({"Soil_Properties": {"a0": 0.012, "psi_sat": -0.01}}, {"Soil_Properties": {"a0": 0.006, "psi_sat": -0.1}}),
          "swapped": ({"Soil_Properties": {"a0": 0.006, "psi_sat": -0.1}}, {"Soil_Properties": {"a0": 0.012, "psi_sat": -0.01}}),
          "predict_next_to_monitoring": ({"Soil_Properties": {"a0": 0.012, "psi_sat": -0.01}, "PREDICT": True},
                                         {"Soil_Properties": {"a0": 0.006, "psi_sat": -0.1}})}


def _stepped(st, psi, seed, offset=0):
    st.set_state(psi)
    st.set_noise_philox(seed, offset)
    out = st.step_rows(1, ROWS, want_wtd=True, want_stats=True)
    return {"psi": st.get_state(), "noise_scale": st.noise_scale(), "moments": np.asarray(st.moments()), "wtd": out["wtd"],
            "stats": out["stats"], "failed": out["failed"]}


@pytest.mark.parametrize("sweep", sorted(SWEEPS))
def test_each_point_of_a_sweep_is_its_stand_alone_run(gpu, sweep):
    import rhs_pack_states as ps
    import rhs_states as rs
    from helpers import WELLS, forcing_frame
    from hydromodel_amd.digest import ColumnTables, ForcingDigest
    from hydromodel_amd.ensemble import check_sweep_points
    from hydromodel_amd.synthetic import default_parameters
    params = default_parameters()
    pts = [dict(p) for p in SWEEPS[sweep]]
    predict = [bool(p.pop("PREDICT", False)) for p in pts]
    cols_all = [ColumnTables(mp, WELLS[D_BENCH]) for mp in check_sweep_points(params, pts)]
    for c, pr in zip(cols_all, predict):
        assert rs.cells_per_lane(c.dim_d) == ps.CPL and c.soil.n == 2.0        # default exponents
        c.flags = dict(c.flags, PREDICT=pr)
    assert cols_all[0].soil.psi_sat != cols_all[1].soil.psi_sat and cols_all[0].soil.alpha != cols_all[1].soil.alpha
    forcing = ForcingDigest(params, forcing_frame(1), cols_all[0])
    sl = slice(1, 1 + ROWS)
    assert forcing.daylight[sl].any() and not forcing.daylight[sl].all()
    one = ps.hydrostatic_spread(cols_all[0], MPP)
    st = gpu.EnsembleStepper(cols_all, forcing, 2 * MPP)
    both = _stepped(st, np.concatenate([one, one]), 45)
    st.close()
    assert np.isfinite(both["psi"]).all()
    alone = []
    for k, c in enumerate(cols_all):
        st = gpu.EnsembleStepper(c, forcing, MPP)
        alone.append(_stepped(st, one, 45, k * MPP))
        st.close()
        sel = slice(k * MPP, (k + 1) * MPP)
        _same(both["psi"][sel], alone[k]["psi"], f"{sweep}, point {k}: psi")
        _same(both["noise_scale"][sel], alone[k]["noise_scale"], f"{sweep}, point {k}: noise_scale")
        _same(both["moments"][k], alone[k]["moments"], f"{sweep}, point {k}: moments")
        for q in ("wtd", "stats", "failed"):
            _same(both[q][:, sel], alone[k][q], f"{sweep}, point {k}: {q}")
    # the points are different runs: a sweep that gave both the same parameters would not pass by accident
    assert alone[0]["psi"].tobytes() != alone[1]["psi"].tobytes()


# ------------------------------------------------------------------------------------------------ (2) the other settings
# (name, flags, n_root_first, HYDROCOL_MODEL_PACK)
RUNS = (("pack_off", None, 1, "0"), ("pack_off_hlift_no_first", {"HLIFT": True}, 0, "0"), ("predict", {"PREDICT": True}, 1, None),
        ("predict_hlift_no_first", {"PREDICT": True, "HLIFT": True}, 0, None), ("no_lf", {"LF": False}, 1, None),
        ("no_lf_no_et_no_first", {"LF": False, "ET": False}, 0, None), ("hlift_no_et", {"HLIFT": True, "ET": False}, 1, None))


@pytest.mark.parametrize("D", (257, 300, 320))
def test_step_variant_against_plain_in_the_other_settings(gpu, D, monkeypatch):
    import rhs_states as rs
    import test_gpu_rhs_as_stepped as base
    import test_gpu_rhs_ilp as ilp
    cols0, forcing, rows = rs.case_column(D)
    assert {r for r, _, _ in rows} >= {"night", "day_dry", "day_demand", "wet", "spinup"}
    assert not forcing.daylight[dict((r, k) for r, k, _ in rows)["night"]]
    names, Y, Z = ilp._bank(cols0)
    k_wet = names.index("wet_roots")
    cases = 0
    for run, flags, n_first, pack in RUNS:
        cols = copy.copy(cols0)
        cols.n_root_first = n_first
        if pack is None:
            monkeypatch.delenv("HYDROCOL_MODEL_PACK", raising=False)
        else:
            monkeypatch.setenv("HYDROCOL_MODEL_PACK", pack)
        st = gpu.EnsembleStepper(cols, forcing, len(names), flags=flags)
        st.set_state(Y)
        for noise in ("host", "philox"):
            if noise == "host":
                st.set_noise_host(Z)
            else:
                st.set_noise_philox(45 + D, 0)
            for rname, row, spin in rows:
                where = f"D = {D}, run {run}, {noise} noise, row {rname}"
                step, hook = base._evaluate(st, row, spin, "step"), base._evaluate(st, row, spin, "hook_layout")
                base._same_bytes(step, hook, where, names)
                for q in base.QUANTITIES:
                    assert np.isfinite(step[q]).all(), (where, q)
                cases += 1
                if rname == "day_demand" and noise == "host":      # the diagnostic sums ran: uptake where ET is on
                    assert (step["diag"][k_wet, 0] > 0.0) == (flags or {}).get("ET", True), where
                if rname == "night" and noise == "host" and (flags or {}).get("LF", True) and not (flags or {}).get("PREDICT"):
                    assert (step["diag"][:, 1] > 0.0).any(), where
        st.close()
    monkeypatch.delenv("HYDROCOL_MODEL_PACK", raising=False)
    assert cases == len(RUNS) * 2 * len(rows)


# ------------------------------------------------------------------------------------------------ (3) the search ahead of ET
def test_the_lateral_flow_search_ahead_of_et(gpu):
    import rhs_states as rs
    import test_gpu_rhs_as_stepped as base
    from helpers import forcing_with_row
    cols, forcing, _ = rs.case_column(D_BENCH)
    D, k = cols.dim_d, cols.dim_d - 2
    targets = (3, 40, 79, 80, 150, D - 2)                  # the estimated water table: both sides of the packed row's end, the last midpoint
    names = [f"wt{j}" for j in targets] + ["saturated"]
    Y = np.stack([rs.water_table_at(cols, j) for j in targets] + [cols.dz * (np.arange(D) + 5.0)])
    jstar = [rs.deepest_unsaturated(cols, y) for y in Y]
    assert jstar == list(targets) + [-1]
    Z = np.random.default_rng(128).standard_normal(Y.shape)
    # one daylight row per observed water table: around each target and the two ends
    obs = sorted({o for j in targets for o in (j - 1, j, j + 1)} | {0, 1, k - 1, k, D})
    f = forcing
    for q, o in enumerate(obs):
        f = forcing_with_row(f, rs.ROW_FIRST + q, 0.0, float(forcing.atm.max()), 1, o, wet=0)
    st = gpu.EnsembleStepper(cols, f, len(names))           # default flags: ET and LF on
    st.set_state(Y)
    st.set_noise_host(Z)
    seen = {"above": 0, "at": 0, "below": 0, "none": 0}
    for q, o in enumerate(obs):
        where = f"observed water table {o}"
        step, hook = base._evaluate(st, rs.ROW_FIRST + q, False, "step"), base._evaluate(st, rs.ROW_FIRST + q, False, "hook_layout")
        base._same_bytes(step, hook, where, names)
        assert (step["diag"][:, 0] > 0.0).any(), where      # ET ran on this row
        for m, j in enumerate(jstar):
            est, ob = min(max(j, 0), k - 1), min(o, k - 1)
            seen["none" if j < 0 else "above" if est < ob else "at" if est == ob else "below"] += 1
            # the sink acts on [est, ob): its total is positive exactly when the estimate lies above the observation
            assert (step["diag"][m, 1] > 0.0) == (est < ob), (where, names[m], step["diag"][m, 1])
    st.close()
    assert min(seen.values()) >= 1, seen


# ------------------------------------------------------------------------------------------------ (4) stepped against -DHC_RHS_ILP=13
N4 = 128


def run4(stepper):
    """-> {name: array}: what 48 rows with hydraulic lift leave behind"""
    import rhs_pack_states as ps
    import rhs_states as rs
    from hydromodel_amd.digest import ColumnTables, ForcingDigest
    from hydromodel_amd.synthetic import default_parameters, synthetic_forcing_frame, synthetic_well
    params = default_parameters()
    cols = ColumnTables(params, synthetic_well(D_BENCH))
    forcing = ForcingDigest(params, synthetic_forcing_frame(1), cols)
    assert rs.cells_per_lane(cols.dim_d) == ps.CPL
    sl = slice(1, 1 + ROWS)
    assert forcing.daylight[sl].any() and not forcing.daylight[sl].all()
    psi = ps.hydrostatic_spread(cols, N4)
    start = np.array([ps.takes_packed_path(cols, y) for y in psi])
    assert start.any() and not start.all()                  # both sides of the boundary
    st = stepper.EnsembleStepper(cols, forcing, N4, flags={"HLIFT": True})
    res = _stepped(st, psi, 45)
    counters = st.counters()
    res["counted"] = np.array([int(counters[q]) for q in COUNTED], dtype=np.int64)
    st.close()
    return res


def test_48_rows_with_hydraulic_lift_against_the_build_without_the_new_parts(gpu, tmp_path):
    import __graft_entry__ as ge
    lib = ge.build_library(tmp_path / "lib_ilp13.so", cpls=(5,), obj_dir=tmp_path / "obj", force=True,
                           defines=("-DHC_CPL_MASK=32", "-DHC_RHS_ILP=13"))
    out = tmp_path / "ilp13.npz"
    p = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(lib), str(out)], cwd=REPO, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    want, got = dict(np.load(out)), run4(gpu)
    assert np.isfinite(got["psi"]).all()
    assert got["counted"].tolist() == want["counted"].tolist()
    for q in ARRAYS:
        _same(got[q], want[q], q)


if __name__ == "__main__":       # python tests/test_gpu_rhs_waits.py <libhydrocol.so> <out.npz>
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    from hydromodel_amd import _lib
    _lib.LIB_PATH = Path(sys.argv[1]).resolve()
    from hydromodel_amd import stepper
    np.savez_compressed(sys.argv[2], **run4(stepper))
