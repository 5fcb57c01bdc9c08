"""The well's record inside the window of the particle filter (include/hydrocol.h hc_set_filter_window), the parts that need
no GPU: the NumPy restatement of the per-member log-likelihood with lagged terms, the offsets' validation, the window's
summary, the CLI's "Filter": {"Window_Offsets": ...} key with its refusals, and the ABI's symbols."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

from hydromodel_amd.cli import FILTER_KEYS, filter_settings, filter_window_settings, run_cli
from hydromodel_amd.stepper import (WINDOW_WIDTH, enkf_window_settings, filter_member_loglik, filter_window_summary)
from hydromodel_amd.stepper import filter_window_settings as window_of

REPO = Path(__file__).resolve().parent.parent
SYMBOLS = ("hc_set_filter_window", "hc_get_filter_window_stats", "hc_set_filter_window_stats",
           "hc_get_filter_window_capture", "hc_set_filter_window_capture", "hc_get_filter_window_width")
SM3 = {"Filename": "sm.csv", "Depths_cm": [30, 60, 120], "Sigma": 0.02}


def _ens(**block):
    return {"Members": 8, "Filter": {"Sigma_cm": 10.0, **block}}


def _inputs(N=300, ms=2, mw=3, seed=5):
    rng = np.random.default_rng(seed)
    return dict(w=rng.integers(20, 70, size=N), theta=rng.uniform(0.05, 0.45, size=(N, ms)), obs=40,
                theta_obs=rng.uniform(0.1, 0.4, size=ms), sigma=rng.uniform(0.01, 0.05, size=ms),
                lag_w=rng.integers(20, 70, size=(N, mw)), lag_obs=rng.integers(35, 45, size=mw), dz=5.0, sigma_cm=7.5)


# ---- 1. the per-member log-likelihood ----------------------------------------------------------------------------------
@pytest.mark.parametrize("ms, mw", [(0, 1), (0, 3), (2, 3), (3, 5)])
def test_lagged_terms_follow_the_sensors_in_a_plain_loop(ms, mw):
    g = _inputs(ms=ms, mw=mw)
    ell = filter_member_loglik(g["w"], g["theta"], g["obs"], g["theta_obs"], g["dz"], g["sigma_cm"], g["sigma"],
                               g["lag_w"], g["lag_obs"])
    assert ell.shape == (300,) and ell.dtype == np.float64
    for m in range(300):
        t = g["dz"] * float(int(g["w"][m]) - g["obs"]) / g["sigma_cm"]
        a = t * t
        for i in range(ms):
            u = (g["theta"][m, i] - g["theta_obs"][i]) / g["sigma"][i]
            a = a + u * u
        for j in range(mw):                                          # by ascending offset, after the sensors
            tj = g["dz"] * float(int(g["lag_w"][m, j]) - int(g["lag_obs"][j])) / g["sigma_cm"]
            a = a + tj * tj
        assert ell[m] == -0.5 * a
    assert np.all(ell <= filter_member_loglik(g["w"], g["theta"], g["obs"], g["theta_obs"], g["dz"], g["sigma_cm"],
                                              g["sigma"]))


def test_without_lagged_arguments_the_bits_are_those_of_the_sensor_rows():
    g = _inputs()
    w = np.asarray(g["w"], dtype=np.int64)
    t = np.float64(g["dz"]) * (w - g["obs"]).astype(np.float64) / np.float64(g["sigma_cm"])
    a = t * t
    for i in range(2):
        u = (g["theta"][:, i] - g["theta_obs"][i]) / g["sigma"][i]
        a = a + u * u
    before = -0.5 * a
    args = (g["w"], g["theta"], g["obs"], g["theta_obs"], g["dz"], g["sigma_cm"], g["sigma"])
    assert filter_member_loglik(*args).tobytes() == before.tobytes()
    assert filter_member_loglik(*args, None, None).tobytes() == before.tobytes()
    assert filter_member_loglik(*args, lag_w=np.zeros((300, 0)), lag_obs_idx=[]).tobytes() == before.tobytes()
    with pytest.raises(ValueError, match="3 lagged columns, 2 observed indices"):
        filter_member_loglik(*args, g["lag_w"], g["lag_obs"][:2])


def test_one_member_is_the_joint_gaussian_log_density():
    dz, sigma_cm = 5.0, 7.0
    ell = filter_member_loglik([43], np.zeros((1, 0)), 40, [], dz, sigma_cm, [], [[41, 38]], [40, 39])
    want = -0.5 * ((dz * 3 / sigma_cm) ** 2 + (dz * 1 / sigma_cm) ** 2 + (dz * -1 / sigma_cm) ** 2)
    assert abs(ell[0] - want) <= 4 * np.finfo(float).eps * abs(want)


# ---- 2. the offsets ----------------------------------------------------------------------------------------------------
def test_the_validator_is_the_enkf_windows_rule_under_the_filters_name():
    assert window_of(None, 48) == () and window_of([], 0) == () and window_of((), 48) == ()
    assert window_of([36, np.int64(12), 24], 48, 2) == (12, 24, 36) == enkf_window_settings([36, 12, 24], 48, 2)
    for bad, what in (([0], "Filter Window_Offsets: 0 lies outside [1, 48)"),
                      ([48], "Filter Window_Offsets: 48 lies outside [1, 48)"),
                      ([12, 24, 12], "Filter Window_Offsets = [12, 12, 24] repeats an offset"),
                      (list(range(1, 10)), "Filter Window_Offsets: 9 offsets, at most 8"),
                      ([True], "Filter Window_Offsets: True is not an integer"),
                      ([12.0], "Filter Window_Offsets: 12.0 is not an integer"),
                      ("12", "Filter Window_Offsets = '12' must be a list of integers")):
        with pytest.raises(ValueError, match=re.escape(what)):
            window_of(bad, 48)
    with pytest.raises(ValueError, match=re.escape("Filter Window_Offsets: 6 offsets and 3 soil-moisture sensors, at most "
                                                   "8 together")):
        window_of([1, 2, 3, 4, 5, 6], 48, n_sensors=3)
    with pytest.raises(ValueError, match="Filter Window_Offsets need the particle filter"):
        window_of([12], 0)
    with pytest.raises(ValueError, match="EnKF Window_Offsets need the EnKF"):      # the EnKF's words did not move
        enkf_window_settings([12], 0)


# ---- 3. the summary ----------------------------------------------------------------------------------------------------
def test_the_windows_summary_reads_a_hand_made_table():
    t = np.full((2, 5, 3, WINDOW_WIDTH), np.nan)                      # two points, slots 0..4, three offsets
    for p in range(2):
        t[p, 1, :, 0] = [1, 0, 1]                                     # slot 1: offsets 0 and 2 took part
        t[p, 1, 0, 1:] = [100.0, 90.0 + p, 4.0]
        t[p, 1, 2, 1:] = [105.0, 99.0 + p, 5.0]
        t[p, 3, :, 0] = [0, 1, 0]                                     # slot 3: offset 1
        t[p, 3, 1, 1:] = [110.0, 111.0 + p, 6.0]
    s = filter_window_summary(t, 48, (12, 24, 36), z0_cm=2.5)
    assert s["rows"].tolist() == [48, 144] and s["offsets"].tolist() == [12, 24, 36]
    assert s["observed"].shape == (2, 2, 3) and s["observed"][0].tolist() == [[True, False, True], [False, True, False]]
    assert s["n_obs"] == 3 and s["n_rows"] == 2
    assert s["obs_cm"][1, 0, 0] == 102.5 and s["prior_mean_cm"][1, 0, 2] == 102.5 and s["prior_std_cm"][0, 1, 1] == 6.0
    assert s["innovation_cm"][1, 0, 0] == 9.0 and np.isnan(s["obs_cm"][0, 0, 1])
    none = filter_window_summary(np.full((5, 3, WINDOW_WIDTH), np.nan), 48, (12, 24, 36))
    assert none["rows"].size == 0 and none["n_obs"] == 0 and none["n_rows"] == 0


# ---- 4. the CLI's key --------------------------------------------------------------------------------------------------
def test_the_key_parses_to_an_ascending_tuple():
    assert "Window_Offsets" in FILTER_KEYS
    assert filter_window_settings(_ens(Window_Offsets=[36, 12, 24])) == (12, 24, 36)
    assert filter_window_settings(_ens(Window_Offsets=[5], Stride=24, Soil_Moisture=SM3)) == (5,)
    assert filter_settings(_ens(Window_Offsets=[12])) == (48, 10.0, None)
    for ens in ({"Members": 8}, _ens(), _ens(Window_Offsets=[]), _ens(Window_Offsets=None),
                {"Members": 8, "EnKF": {"Sigma_cm": 10.0, "Window_Offsets": [12]}}):
        assert filter_window_settings(ens) is None
    pts = [{"Soil_Properties": {"n": 1.6}}, {"Soil_Properties": {"n": 2.4}}]
    assert filter_window_settings({**_ens(Window_Offsets=[12], Sharded=True), "Points": pts}) == (12,)   # a sweep ignores Sharded


REJECTED = [
    (_ens(Window_Offsets=12), "Filter Window_Offsets = 12 must be a list of integers"),
    (_ens(Window_Offsets=[0]), "Filter Window_Offsets: 0 lies outside [1, 48)"),
    (_ens(Window_Offsets=[12, 48]), "Filter Window_Offsets: 48 lies outside [1, 48)"),
    (_ens(Window_Offsets=[24], Stride=24), "Filter Window_Offsets: 24 lies outside [1, 24)"),
    (_ens(Window_Offsets=[12, 24, 12]), "Filter Window_Offsets = [12, 12, 24] repeats an offset"),
    (_ens(Window_Offsets=[12.0]), "Filter Window_Offsets: 12.0 is not an integer"),
    (_ens(Window_Offsets=list(range(1, 10))), "Filter Window_Offsets: 9 offsets, at most 8"),
    (_ens(Window_Offsets=[1, 2, 3, 4, 5, 6], Soil_Moisture=SM3),
     "Filter Window_Offsets: 6 offsets and 3 soil-moisture sensors, at most 8 together"),
    (_ens(Window_Offsets=[12], Stride=0), "Filter.Window_Offsets needs an active filter (Filter.Stride > 0)"),
    (_ens(Window_Offsets=[], Stride=0), "Filter.Window_Offsets needs an active filter (Filter.Stride > 0)"),
    (_ens(Window_Offsets=[12], Sharded=True), "Filter.Window_Offsets is not available with \"Sharded\": true"),
    ({"Members": 8, "Window_Offsets": [12]}, "Window_Offsets belongs inside the \"Filter\" or the \"EnKF\" block"),
    ({"Members": 8, "Window_Offsets": [12], "Filter": {"Sigma_cm": 10.0}},
     "Window_Offsets belongs inside the \"Filter\" or the \"EnKF\" block"),
]


@pytest.mark.parametrize("ens, message", REJECTED)
def test_window_settings_rejects(ens, message):
    with pytest.raises(ValueError) as err:
        filter_window_settings(ens)
    assert message in str(err.value) and str(err.value).startswith(" Ensemble: ")


@pytest.mark.parametrize("ens, message", REJECTED)
def test_a_bad_window_ends_the_command_with_status_1_before_any_gpu_call(tmp_path, capsys, monkeypatch, ens, message):
    from hydromodel_amd import ensemble
    from hydromodel_amd.synthetic import default_parameters

    def no_gpu(*a, **k):
        raise AssertionError("a GPU handle was created")
    monkeypatch.setattr(ensemble, "EnsembleStepper", no_gpu)
    params = default_parameters()
    params["Data_Filename"] = str(tmp_path / "missing.csv")          # never reached: the block is refused first
    params["Ensemble"] = ens
    (tmp_path / "p.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as stop:
        run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "p.json")])
    assert stop.value.code == 1
    out = capsys.readouterr().out
    assert message in out and "missing.csv" not in out


def test_a_bad_window_ends_a_multi_gpu_command_before_any_rank_starts(tmp_path, capsys, monkeypatch):
    from hydromodel_amd import multigpu
    from hydromodel_amd.synthetic import default_parameters

    def no_ranks(*a, **k):
        raise AssertionError("ranks were started")
    monkeypatch.setattr(multigpu, "launch_ranks", no_ranks)
    params = default_parameters()
    params["Ensemble"] = dict(_ens(Window_Offsets=[48]), Points=[{}, {}], GPUs=2)
    (tmp_path / "p.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as stop:
        run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "p.json")])
    assert stop.value.code == 1 and "48 lies outside [1, 48)" in capsys.readouterr().out


def test_the_simulation_refuses_a_window_with_a_shard_or_without_the_filter():
    from hydromodel_amd.ensemble import EnsembleSimulation
    with pytest.raises(ValueError, match="filter_shard and filter_window_offsets exclude each other"):
        EnsembleSimulation(None, None, 8, filter_stride=48, filter_sigma_cm=5.0, filter_shard=([0, 8], 0, None),
                           filter_window_offsets=(12,))


# ---- 5. the ABI --------------------------------------------------------------------------------------------------------
def test_the_symbols_are_in_the_header_and_in_the_prototypes():
    from hydromodel_amd import _lib
    header = (REPO / "include" / "hydrocol.h").read_text()
    source = (REPO / "hydromodel_amd" / "_lib.py").read_text()
    for name in SYMBOLS:
        assert re.search(rf"^int {name}\(hc_handle \*h, ", header, re.M), name
        assert f'"{name}"' in source, name
    protos = next(v for v in vars(_lib).values() if isinstance(v, dict) and "hc_set_filter" in v)
    for name in SYMBOLS:
        assert name in protos and len(protos[name][0]) == len(protos[name.replace("filter", "enkf")][0])
