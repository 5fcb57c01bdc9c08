"""Perturbed forcing, the parts that need no GPU (include/hydrocol.h hc_set_forcing_perturbation): the NumPy restatement of
the recursion, the coefficients, the day of a row, the CLI block and its refusals, the checkpoint's layout, the library's
entry points."""
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. the recursion
def test_recursion_is_the_scalar_loop_written_out():
    from hydromodel_amd.stepper import forcing_coefficients, forcing_recursion_of
    phi, c = forcing_coefficients(3)
    xi = np.random.default_rng(3).standard_normal((9, 2, 5))
    g = forcing_recursion_of(xi, phi, c)
    for s in range(2):
        for m in range(5):
            v = float(xi[0, s, m])
            assert g[0, s, m] == v
            for k in range(1, 9):
                keep = phi * v
                fresh = c * float(xi[k, s, m])
                v = keep + fresh
                assert g[k, s, m] == v, (k, s, m)


def test_recursion_at_tau_zero_is_the_identity_on_the_normals():
    from hydromodel_amd.stepper import forcing_coefficients, forcing_recursion_of
    xi = np.random.default_rng(4).standard_normal((12, 7))
    assert _same(forcing_recursion_of(xi, *forcing_coefficients(0)), xi)


def test_recursion_on_a_hand_built_sequence():
    from hydromodel_amd.stepper import forcing_coefficients, forcing_recursion_of
    phi, c = forcing_coefficients(3)
    assert phi == float(np.exp(-1.0 / 3.0))
    xi = np.array([1.0, 0.0, 0.0, -2.0, 0.5])
    g = forcing_recursion_of(xi, phi, c)
    want = [1.0, phi, phi * phi, (phi * (phi * phi)) + (c * -2.0)]
    want.append((phi * want[3]) + (c * 0.5))
    assert g.tolist() == want
    unit = forcing_recursion_of(np.random.default_rng(5).standard_normal((400, 2000)), phi, c)
    assert abs(unit[-1].var() - 1.0) < 5.0 * np.sqrt(2.0 / 2000)                # an AR(1) of unit variance


@pytest.mark.parametrize("tau", [0, 0.25, 1, 3, 30, 365])
def test_coefficients_are_a_unit_variance_step(tau):
    from hydromodel_amd.stepper import forcing_coefficients
    phi, c = forcing_coefficients(tau)
    assert abs(phi * phi + c * c - 1.0) <= 1e-15
    assert 0.0 <= phi < 1.0 and 0.0 < c <= 1.0
    if tau == 0:
        assert (phi, c) == (0.0, 1.0)
    else:
        assert phi == float(np.exp(-1.0 / tau))


@pytest.mark.parametrize("bad", [True, -1, float("nan"), float("inf"), "3", None])
def test_coefficients_refuse_what_is_no_time(bad):
    from hydromodel_amd.stepper import forcing_coefficients
    with pytest.raises(ValueError):
        forcing_coefficients(bad)


def test_factors_of_sigma_zero_are_exactly_one_and_the_mean_is_one():
    from hydromodel_amd.stepper import forcing_factors_of
    g = np.random.default_rng(6).standard_normal(200000)
    assert _same(forcing_factors_of(g, 0.0), np.ones_like(g))
    f = forcing_factors_of(g, 0.3)
    assert abs(f.mean() - 1.0) < 5.0 * np.sqrt(np.exp(0.09) - 1.0) / np.sqrt(g.size)
    assert f[0] == np.exp((0.3 * g[0]) - 0.045)


def test_the_day_of_a_row_is_the_noise_refresh_clock():
    from hydromodel_amd.stepper import FORCING_DAY_ROWS, forcing_day_of_row
    assert FORCING_DAY_ROWS == 48
    assert forcing_day_of_row(np.array([0, 1, 47, 48, 95, 96])).tolist() == [0, 0, 0, 1, 1, 2]
    assert int(forcing_day_of_row(47)) == 0 and int(forcing_day_of_row(48)) == 1
    header = (REPO / "include" / "hydrocol.h").read_text()
    assert "#define HC_FORCING_DAY_ROWS 48" in header


# ---- 2. the settings
def test_constructor_settings_and_their_refusals():
    from hydromodel_amd.stepper import forcing_perturbation_settings as settings
    assert settings(None) is None
    assert settings({"precipitation_sigma": 0.3}) == {"precipitation_sigma": 0.3, "demand_sigma": 0.0,
                                                      "correlation_days": 0.0, "seed": None}
    assert settings({"demand_sigma": 1, "correlation_days": 3, "seed": 9})["seed"] == 9
    for bad in (3, {}, {"correlation_days": 3}, {"precipitation_sigma": 0.1, "sigma": 1}, {"precipitation_sigma": True},
                {"precipitation_sigma": 1.01}, {"demand_sigma": -0.1}, {"demand_sigma": float("nan")},
                {"demand_sigma": 0.1, "correlation_days": 366}, {"demand_sigma": 0.1, "correlation_days": -1},
                {"demand_sigma": 0.1, "seed": -1}, {"demand_sigma": 0.1, "seed": 1.5}):
        with pytest.raises(ValueError):
            settings(bad)


def test_cli_block():
    from hydromodel_amd.cli import forcing_perturbation_settings as settings
    assert settings({"Members": 8}) is None
    got = settings({"Seed": 5, "Forcing_Perturbation": {"Precipitation_Sigma": 0.3, "Demand_Sigma": 0.1, "Correlation_Days": 3}})
    assert got == {"precipitation_sigma": 0.3, "demand_sigma": 0.1, "correlation_days": 3.0, "seed": 5}     # the ensemble's seed
    got = settings({"Seed": 5, "Forcing_Perturbation": {"Demand_Sigma": 0.1, "Seed": 77}})
    assert got == {"precipitation_sigma": 0.0, "demand_sigma": 0.1, "correlation_days": 0.0, "seed": 77}
    # a sharded filter in a sweep is ignored (its points are dealt whole), so the block stands
    assert settings({"Points": [{}], "Filter": {"Stride": 48, "Sharded": True},
                     "Forcing_Perturbation": {"Demand_Sigma": 0.1}}) is not None


BAD_BLOCKS = [
    (3, "must be an object"),
    ([0.3], "must be an object"),
    ({"Precipitation_Sigma": 0.3, "Tau": 3}, "unknown keys ['Tau']"),
    ({"Correlation_Days": 3}, "needs Precipitation_Sigma or Demand_Sigma"),
    ({"Precipitation_Sigma": True}, "Precipitation_Sigma = True"),
    ({"Precipitation_Sigma": "0.3"}, "Precipitation_Sigma = '0.3'"),
    ({"Demand_Sigma": float("nan")}, "Demand_Sigma = nan"),
    ({"Demand_Sigma": float("inf")}, "Demand_Sigma = inf"),
    ({"Precipitation_Sigma": 1.5}, "in [0, 1]"),
    ({"Demand_Sigma": -0.01}, "in [0, 1]"),
    ({"Demand_Sigma": 0.1, "Correlation_Days": 366}, "in [0, 365]"),
    ({"Demand_Sigma": 0.1, "Correlation_Days": -1}, "in [0, 365]"),
    ({"Demand_Sigma": 0.1, "Correlation_Days": False}, "Correlation_Days = False"),
    ({"Demand_Sigma": 0.1, "Seed": -3}, "Seed = -3"),
    ({"Demand_Sigma": 0.1, "Seed": True}, "Seed = True"),
]


@pytest.mark.parametrize("block, message", BAD_BLOCKS)
def test_a_bad_block_ends_the_command_with_status_1_before_any_gpu_call(tmp_path, capsys, block, message):
    from hydromodel_amd.cli import run_cli
    from hydromodel_amd.synthetic import default_parameters
    params = default_parameters()
    params["Data_Filename"] = str(tmp_path / "missing.csv")          # never reached: the block is refused first
    params["Ensemble"] = {"Members": 8, "Days": 1, "Forcing_Perturbation": block}
    (tmp_path / "p.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as stop:
        run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "p.json")])
    assert stop.value.code == 1
    out = capsys.readouterr().out
    assert message in out and "missing.csv" not in out


def test_a_sharded_filter_on_one_point_is_refused(tmp_path, capsys):
    from hydromodel_amd.cli import forcing_perturbation_settings as settings
    ens = {"Members": 8, "Filter": {"Stride": 48, "Sigma_cm": 5.0, "Sharded": True},
           "Forcing_Perturbation": {"Precipitation_Sigma": 0.3}}
    with pytest.raises(ValueError, match="do not carry the members' forcing state"):
        settings(ens)
    from hydromodel_amd.ensemble import EnsembleSimulation
    with pytest.raises(ValueError, match="filter_shard and forcing_perturbation exclude each other"):
        EnsembleSimulation(None, None, 8, filter_stride=48, filter_sigma_cm=5.0, filter_shard=([0, 8], 0, None),
                           forcing_perturbation={"precipitation_sigma": 0.3})


def test_a_host_noise_ensemble_is_initialised_as_it_was():
    """The perturbed forcing has a member offset of its own (hc_set_forcing_member_offset): nothing re-keys the handle of
    a host-noise run, whose particle filter, rejuvenation and EnKF draw by the handle's Philox offset."""
    import inspect
    from hydromodel_amd.ensemble import EnsembleSimulation
    assert "set_noise_philox" not in inspect.getsource(EnsembleSimulation._init_numpy)


# ---- 3. the checkpoint and the results file
class _FakeStepper:
    def forcing_state(self):
        return np.arange(6, dtype=np.float64).reshape(2, 3), 4

    def set_forcing_state(self, g, day):
        self.got = (np.array(g), day)


def test_dump_layout_and_the_way_back():
    from hydromodel_amd import settings
    plain = settings.normalise("EnsembleSimulation", {}, [None], 0)
    assert plain.forcing_perturbation is None and settings.checkpoint_datasets(plain) == {}      # without it: no key
    assert settings.checkpoint_keywords({}, "ck.h5") == {}
    given = {"precipitation_sigma": 0.3, "demand_sigma": 0.1, "correlation_days": 3.0, "seed": 11}
    sim = settings.normalise("EnsembleSimulation", {"forcing_perturbation": given}, [None], 0)
    sim.stepper = _FakeStepper()
    (_, write, install), = [f for f in settings.RUN_STATE if f[0] == "forcing_perturbation"]
    arrays = dict(settings.checkpoint_datasets(sim), **write(sim, sim.stepper))
    assert sorted(arrays) == ["forcing_correlation_days", "forcing_demand_sigma", "forcing_precipitation_sigma",
                              "forcing_seed", "forcing_state", "forcing_state_day"]
    assert arrays["forcing_state"].shape == (2, 3) and arrays["forcing_state"].dtype == np.float64
    assert arrays["forcing_state_day"].dtype == np.int64 and int(arrays["forcing_state_day"]) == 4
    assert arrays["forcing_seed"].dtype == np.uint64
    back = settings.checkpoint_keywords(arrays, "ck.h5")
    assert back == {"forcing_perturbation": given}
    install(sim, {k: np.asarray(v).reshape(-1) for k, v in arrays.items()}, "ck.h5")            # (a flat container)
    assert _same(sim.stepper.got[0], np.arange(6, dtype=np.float64).reshape(2, 3)) and sim.stepper.got[1] == 4


def test_results_file_entries_and_the_closing_line():
    from hydromodel_amd.cli import _forcing_perturbation_arrays
    from hydromodel_amd.stepper import forcing_coefficients
    assert _forcing_perturbation_arrays(None, "Ensemble x8") == ({}, None)
    pert = {"precipitation_sigma": 0.3, "demand_sigma": 0.1, "correlation_days": 3.0, "seed": 5}
    arrays, line = _forcing_perturbation_arrays(pert, "Ensemble x8")
    assert sorted(arrays) == ["forcing_correlation_days", "forcing_demand_sigma", "forcing_phi",
                              "forcing_precipitation_sigma", "forcing_seed"]
    assert float(arrays["forcing_phi"]) == forcing_coefficients(3.0)[0] and int(arrays["forcing_seed"]) == 5
    assert line == " [Ensemble x8] forcing perturbation: precipitation sigma 0.3, demand sigma 0.1, correlation 3 days"


# ---- 4. the library
def test_the_header_declares_what_the_library_exports():
    from hydromodel_amd import _lib
    header = (REPO / "include" / "hydrocol.h").read_text()
    declared = set(re.findall(r"^int (hc_\w*forcing_\w+)\(", header, flags=re.M)) - {"hc_set_forcing_row"}
    want = {"hc_set_forcing_perturbation", "hc_clear_forcing_perturbation", "hc_set_forcing_member_offset",
            "hc_get_forcing_perturbation",
            "hc_get_forcing_state", "hc_set_forcing_state", "hc_forcing_normals", "hc_forcing_factors"}
    assert declared == want
    assert want <= set(_lib.EXPORTS)
    for word in ("HC_FORCING_WORD_PRECIP 0xFFFFFFE0u", "HC_FORCING_WORD_DEMAND 0xFFFFFFE1u"):
        assert word in header


def test_the_host_unit_compiles_for_gfx950_without_warnings_and_exports_the_entry_points():
    import __graft_entry__ as ge
    ge.build()
    src = ge.CSRC / "hydrocol.hip"
    text = src.read_text()
    assert all(k in text for k in ("forcing_factor_fill_kernel", "forcing_normals_kernel"))
    p = subprocess.run([ge._hipcc(), *ge.HIPCC_FLAGS, '-DHC_KERNEL_HASH="test"', "-Wall", "-fsyntax-only", str(src)],
                       cwd=str(ge.CSRC), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "forcing" not in p.stderr and "fp_" not in p.stderr and "fmul" not in p.stderr, p.stderr[-3000:]
    from hydromodel_amd import _lib
    lib = _lib.load()
    names = [n for n in _lib.EXPORTS if "forcing_" in n and n != "hc_set_forcing_row"]
    assert len(names) == 8 and all(hasattr(lib, n) for n in names)


def test_the_monitoring_mode_kernels_are_the_parents_to_the_instruction():
    """profiles/r08_isa_vs_parent.txt (tools/isa_vs_parent.py): every step kernel without the predictive branch and every RHS
    hook has the instruction stream it had; only builds with the branch carry the two products."""
    lines = [ln for ln in (REPO / "profiles" / "r08_isa_vs_parent.txt").read_text().splitlines() if not ln.startswith("#")]
    assert len(lines) >= 100
    for ln in lines:
        unit, kernel, counts, differ = [f.strip() for f in ln.split("|")]
        predict = re.match(r"hc::step_kernel<\d+, \w+, \d+, true,", kernel) is not None
        assert (differ != "none") == predict, ln
