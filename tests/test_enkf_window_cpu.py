"""The well's record inside the EnKF's window on the host (no GPU): the C-ABI entries, the "Window_Offsets" validator and
its refusals before any GPU call, and the summary of the window's table (include/hydrocol.h hc_set_enkf_window)."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

from hydromodel_amd.cli import ENKF_KEYS, enkf_method_settings, enkf_settings, enkf_window_settings, run_cli
from hydromodel_amd.stepper import WINDOW_WIDTH, enkf_window_summary
from hydromodel_amd.stepper import enkf_window_settings as window_of

REPO = Path(__file__).resolve().parent.parent
NEW_ENTRIES = ("hc_set_enkf_window", "hc_get_enkf_window_stats", "hc_set_enkf_window_stats", "hc_get_enkf_window_capture",
               "hc_set_enkf_window_capture", "hc_get_enkf_width", "hc_get_enkf_window_width", "hc_get_enkf_window_y",
               "hc_get_enkf_window_eps", "hc_get_enkf_window_gain")


def test_header_declares_and_the_binding_lists_the_new_entries():
    text = (REPO / "include" / "hydrocol.h").read_text()
    from hydromodel_amd import _lib as L
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in L.EXPORTS, name
    assert "Window_Offsets" in ENKF_KEYS


def _ens(**enkf):
    return {"Members": 8, "EnKF": {"Sigma_cm": 10.0, **enkf}}


SM3 = {"Filename": "sm.csv", "Depths_cm": [30, 60, 120], "Sigma": 0.02}


@pytest.mark.parametrize("ens, want", [
    ({"Members": 8}, None),
    (_ens(), None),
    (_ens(Window_Offsets=[]), None),
    (_ens(Window_Offsets=None), None),
    (_ens(Window_Offsets=[12, 24, 36]), (12, 24, 36)),
    (_ens(Window_Offsets=[36, 12, 24]), (12, 24, 36)),
    (_ens(Window_Offsets=(1, 47)), (1, 47)),
    (_ens(Window_Offsets=[48, 144, 96], Stride=192), (48, 96, 144)),
    (_ens(Window_Offsets=list(range(1, 9))), tuple(range(1, 9))),
    (_ens(Window_Offsets=[1, 2, 3, 4, 5], Soil_Moisture=SM3), (1, 2, 3, 4, 5)),
    (dict(_ens(Window_Offsets=[12], Method="sqrt"), Points=[{}, {}]), (12,)),
])
def test_window_settings_accepts_and_returns_the_offsets_ascending(ens, want):
    got = enkf_window_settings(ens)
    assert got == want and (got is None or all(type(o) is int for o in got))
    assert enkf_settings(ens, 1)[0] in (0, 48, 192)                   # the other validators take the key
    enkf_method_settings(ens)


REJECTED = [
    (_ens(Window_Offsets=12), "EnKF Window_Offsets = 12 must be a list of integers"),
    (_ens(Window_Offsets="12,24"), "EnKF Window_Offsets = '12,24' must be a list of integers"),
    (_ens(Window_Offsets={"a": 1}), "must be a list of integers"),
    (_ens(Window_Offsets=[0]), "EnKF Window_Offsets: 0 lies outside [1, 48)"),
    (_ens(Window_Offsets=[-3, 12]), "EnKF Window_Offsets: -3 lies outside [1, 48)"),
    (_ens(Window_Offsets=[12, 48]), "EnKF Window_Offsets: 48 lies outside [1, 48)"),
    (_ens(Window_Offsets=[12, 60]), "EnKF Window_Offsets: 60 lies outside [1, 48)"),
    (_ens(Window_Offsets=[24], Stride=24), "EnKF Window_Offsets: 24 lies outside [1, 24)"),
    (_ens(Window_Offsets=[12, 24, 12]), "EnKF Window_Offsets = [12, 12, 24] repeats an offset"),
    (_ens(Window_Offsets=[True]), "EnKF Window_Offsets: True is not an integer"),
    (_ens(Window_Offsets=[12, False]), "EnKF Window_Offsets: False is not an integer"),
    (_ens(Window_Offsets=[12.0]), "EnKF Window_Offsets: 12.0 is not an integer"),
    (_ens(Window_Offsets=[12, 24.5]), "EnKF Window_Offsets: 24.5 is not an integer"),
    (_ens(Window_Offsets=["12"]), "EnKF Window_Offsets: '12' is not an integer"),
    (_ens(Window_Offsets=list(range(1, 10))), "EnKF Window_Offsets: 9 offsets, at most 8"),
    (_ens(Window_Offsets=[1, 2, 3, 4, 5, 6], Soil_Moisture=SM3),
     "EnKF Window_Offsets: 6 offsets and 3 soil-moisture sensors, at most 8 together"),
    (_ens(Window_Offsets=[12], Stride=0), "EnKF.Window_Offsets needs an active EnKF (EnKF.Stride > 0)"),
    (_ens(Window_Offsets=[], Stride=0), "EnKF.Window_Offsets needs an active EnKF (EnKF.Stride > 0)"),
]


@pytest.mark.parametrize("ens, message", REJECTED)
def test_window_settings_rejects(ens, message):
    with pytest.raises(ValueError) as err:
        enkf_window_settings(ens)
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


def test_the_python_side_validator_is_the_same_rule():
    assert window_of(None, 48) == () and window_of([], 0) == () and window_of((), 48) == ()
    assert window_of([np.int64(5), 3], 48) == (3, 5)
    for bad in ([12], (1,)):
        with pytest.raises(ValueError, match="need the EnKF"):
            window_of(bad, 0)
    with pytest.raises(ValueError, match="at most 8 together"):
        window_of([1, 2], 48, n_sensors=7)
    with pytest.raises(ValueError, match="not an integer"):
        window_of([np.float64(3.0)], 48)


def test_the_windows_summary_reads_the_table():
    t = np.full((2, 5, 3, WINDOW_WIDTH), np.nan)                      # two points, slots 0..4, three offsets
    for p in range(2):
        t[p, 1, :, 0] = [1, 0, 1]                                     # slot 1: offsets 0 and 2 took part
        t[p, 1, 0, 1:] = [100.0, 90.0 + p, 4.0]
        t[p, 1, 2, 1:] = [105.0, 99.0 + p, 5.0]
        t[p, 3, :, 0] = [0, 1, 0]                                     # slot 3: offset 1
        t[p, 3, 1, 1:] = [110.0, 111.0 + p, 6.0]
    s = enkf_window_summary(t, 48, (12, 24, 36), z0_cm=2.5)
    assert s["rows"].tolist() == [48, 144] and s["offsets"].tolist() == [12, 24, 36]
    assert s["observed"].shape == (2, 2, 3) and s["observed"][0].tolist() == [[True, False, True], [False, True, False]]
    assert s["n_obs"] == 3 and s["n_rows"] == 2
    assert s["obs_cm"][1, 0, 0] == 102.5 and s["prior_mean_cm"][1, 0, 2] == 102.5 and s["prior_std_cm"][0, 1, 1] == 6.0
    assert s["innovation_cm"][1, 0, 0] == 9.0 and s["innovation_cm"][0, 1, 1] == -1.0
    assert np.isnan(s["obs_cm"][0, 0, 1]) and np.isnan(s["innovation_cm"][0, 1, 0])
    one = enkf_window_summary(t[0], 48, (12, 24, 36))
    assert one["observed"].shape == (2, 3) and one["n_obs"] == 3 and one["obs_cm"][0, 0] == 100.0
    none = enkf_window_summary(np.full((5, 3, WINDOW_WIDTH), np.nan), 48, (12, 24, 36))
    assert none["rows"].size == 0 and none["n_obs"] == 0 and none["n_rows"] == 0
