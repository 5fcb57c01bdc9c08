"""Soil-moisture sensors in the particle filter, the parts that need no GPU: the CLI's "Filter": {"Soil_Moisture": ...}
block (the EnKF's parser under another name), the NumPy restatement of the per-member log-likelihood, the fixed summation
order, and the sensors' summary."""
import json
import re

import numpy as np
import pytest

from hydromodel_amd.cli import FILTER_KEYS, filter_settings, run_cli, soil_moisture_settings
from hydromodel_amd.stepper import (SM_WIDTH, enkf_sm_summary, filter_member_loglik, filter_sm_summary, filter_summary,
                                    filter_tile_sum)

SM = {"Filename": "sm.csv", "Depths_cm": [30, 60, 120], "Sigma": 0.02}


def _ens(sm=SM, owner="Filter", **block):
    return {"Members": 8, owner: {"Sigma_cm": 10.0, "Soil_Moisture": sm, **block}}


# ---- 1. the CLI's block ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sm", [SM, {**SM, "Sigma": [0.02, 0.03, 0.01]}, {**SM, "Depths_cm": [5]}])
def test_filter_block_parses_to_the_enkfs_tuple(sm):
    got = soil_moisture_settings(_ens(sm), 1, "Filter")
    assert got is not None and got == soil_moisture_settings(_ens(sm, "EnKF"), 1)
    assert got[0] == "sm.csv" and len(got[1]) == len(got[2]) == len(sm["Depths_cm"])
    assert "Soil_Moisture" in FILTER_KEYS and filter_settings(_ens(sm), 1) == (48, 10.0, None)


def test_no_block_is_none_under_either_owner():
    for ens in ({"Members": 8}, {"Members": 8, "Filter": {"Sigma_cm": 1.0}}, _ens(owner="EnKF")):
        assert soil_moisture_settings(ens, 1, "Filter") is None
    assert soil_moisture_settings(_ens(), 1) is None              # the EnKF's parser does not see the filter's block


def test_a_sweep_takes_the_block_on_several_gpus_with_or_without_sharded():
    pts = [{"Soil_Properties": {"n": 1.6}}, {"Soil_Properties": {"n": 2.4}}]
    for extra in ({}, {"Sharded": True}):
        ens = {**_ens(**extra), "Points": pts}
        assert soil_moisture_settings(ens, 2, "Filter")[1] == (30.0, 60.0, 120.0)


@pytest.mark.parametrize("ens, gpus, message", [
    (_ens({**SM, "Units": "vwc"}), 1, "Filter.Soil_Moisture has unknown keys ['Units']"),
    (_ens({k: v for k, v in SM.items() if k != "Sigma"}), 1, "Filter.Soil_Moisture.Sigma (the sensors' error, m^3/m^3) is "
                                                              "required"),
    (_ens({**SM, "Depths_cm": list(range(10, 100, 10))}), 1, "Filter.Soil_Moisture.Depths_cm has 9 depths, at most 8"),
    (_ens({**SM, "Sigma": [0.02, 0.03]}), 1, "Filter.Soil_Moisture.Sigma = [0.02, 0.03] must be"),
    (_ens({**SM, "Filename": ""}), 1, "Filter.Soil_Moisture.Filename = '' must name the sensor CSV"),
    (_ens("sm.csv"), 1, "Filter.Soil_Moisture = 'sm.csv' must be an object"),
    (_ens(Sharded=True), 2, "Filter.Soil_Moisture is not available with \"Sharded\": true"),
    (_ens(Sharded=True), 1, "the sharded filter gathers the members' water-table indices only"),
    (_ens(Stride=0), 1, "Filter.Soil_Moisture needs an active filter (Filter.Stride > 0)"),
    (_ens(), 2, "Filter with one parameter point runs on one GPU"),
    ({"Members": 8, "Soil_Moisture": SM, "Filter": {"Sigma_cm": 10.0}}, 1,
     "Soil_Moisture belongs inside the \"EnKF\" block"),
    ({"Members": 8, "Filter": {"Sigma_cm": 10.0, "Soil_moisture": SM}}, 1, "Filter has unknown keys ['Soil_moisture']"),
])
def test_filter_block_rejects(ens, gpus, message):
    with pytest.raises(ValueError, match=re.escape(message)):
        soil_moisture_settings(ens, gpus, "Filter")


def test_cli_refuses_a_sharded_record_before_any_gpu_work(tmp_path, capsys):
    """The parameter file names no data file that exists and no GPU is asked for: the refusal comes first."""
    from hydromodel_amd.synthetic import default_parameters
    params = default_parameters()
    params["Data_Filename"] = str(tmp_path / "missing.csv")
    params["Ensemble"] = {"Members": 64, "Days": 1, "Filter": {"Sigma_cm": 10.0, "Sharded": True, "Soil_Moisture": SM}}
    (tmp_path / "p.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as status:
        run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "p.json")])
    assert status.value.code == 1
    assert "Filter.Soil_Moisture is not available with \"Sharded\": true" in capsys.readouterr().out


# ---- 2. the per-member log-likelihood ----------------------------------------------------------------------------------
def test_one_member_one_sensor_is_the_gaussian_log_density():
    dz, sigma_cm, s_th = 5.0, 7.0, 0.02
    w, o, th, th_o = 43, 40, 0.231, 0.25
    ell = filter_member_loglik([w], [[th]], o, [th_o], dz, sigma_cm, [s_th])
    assert ell.shape == (1,)
    # log N(z_o | z_w, sigma_cm) + log N(theta_o | theta, s) with the normalisation taken off
    want = -0.5 * ((dz * (w - o) / sigma_cm) ** 2 + ((th - th_o) / s_th) ** 2)
    assert abs(ell[0] - want) <= 4 * np.finfo(float).eps * abs(want)
    joint = ell[0] - np.log(sigma_cm) - np.log(s_th) - np.log(2.0 * np.pi)
    density = (np.exp(-0.5 * (15.0 / sigma_cm) ** 2) / (sigma_cm * np.sqrt(2 * np.pi))
               * np.exp(-0.5 * ((th - th_o) / s_th) ** 2) / (s_th * np.sqrt(2 * np.pi)))
    assert abs(joint - np.log(density)) <= 1e-13 * abs(joint)


def test_a_sensor_of_huge_error_adds_exactly_nothing():
    rng = np.random.default_rng(5)
    N, dz, sigma_cm, o = 300, 5.0, 7.5, 40
    w = rng.integers(20, 70, size=N)
    theta = rng.uniform(0.05, 0.45, size=(N, 2))
    ell = filter_member_loglik(w, theta, o, [0.2, 0.3], dz, sigma_cm, [1e200, 1e200])
    t = dz * (np.arange(101) - o).astype(np.float64) / sigma_cm
    l_b = -0.5 * (t * t)                                          # the bin path's l_b
    assert ell.tobytes() == l_b[w].tobytes()
    assert not np.array_equal(filter_member_loglik(w, theta, o, [0.2, 0.3], dz, sigma_cm, [0.02, 1e200]), ell)


def test_sensor_terms_are_added_in_record_order():
    w, theta = np.array([41, 44]), np.array([[0.2, 0.3, 0.1], [0.25, 0.31, 0.4]])
    obs, sg = np.array([0.22, 0.28, 0.15]), np.array([0.02, 0.03, 0.05])
    ell = filter_member_loglik(w, theta, 40, obs, 5.0, 6.0, sg)
    for m in range(2):
        t = 5.0 * float(w[m] - 40) / 6.0
        a = t * t
        for i in range(3):
            u = (theta[m, i] - obs[i]) / sg[i]
            a += u * u
        assert ell[m] == -0.5 * a


def test_the_fixed_summation_order():
    rng = np.random.default_rng(1)
    for n in (1, 3, 4, 5, 255, 256, 1023, 1024, 1025, 2500):
        x = rng.uniform(0.0, 1.0, size=n)
        got = filter_tile_sum(x)
        assert abs(got - float(np.sum(x.astype(np.longdouble)))) <= n * 2.0 ** -53 * got
        pad = np.zeros(-(-n // 1024) * 1024)
        pad[:n] = x
        total = 0.0
        for tile in pad.reshape(-1, 256, 4):
            th = [((0.0 + a) + b + c) + d for a, b, c, d in tile]
            o = 128
            while o:
                th[:o] = [th[i] + th[i + o] for i in range(o)]
                o //= 2
            total += th[0]
        assert got == total
    cols = rng.uniform(size=(1500, 3))
    assert filter_tile_sum(cols).tolist() == [filter_tile_sum(cols[:, j]) for j in range(3)]


# ---- 3. the summary ----------------------------------------------------------------------------------------------------
def _table(P=None):
    lead = () if P is None else (P,)
    t = np.full(lead + (5, 2, SM_WIDTH), np.nan)
    # slots 1 and 3 are sensor rows; on slot 3 sensor 1 has no value
    t[..., 1, 0, :] = [1.0, 0.25, 0.24, 0.02, 0.245, 0.01]
    t[..., 1, 1, :] = [1.0, 0.30, 0.33, 0.03, 0.31, 0.02]
    t[..., 3, 0, :] = [1.0, 0.20, 0.22, 0.02, 0.21, 0.01]
    t[..., 3, 1, 0] = 0.0
    return t


@pytest.mark.parametrize("P", [None, 3])
def test_filter_sm_summary_shapes_nan_handling_and_rmse(P):
    s = filter_sm_summary(_table(P), 24, [0.02, 0.03])
    lead = () if P is None else (P,)
    assert s["rows"].tolist() == [24, 72] and s["stride"] == 24
    for k in ("observed", "obs", "prior_mean", "prior_std", "post_mean", "post_std"):
        assert s[k].shape == lead + (2, 2), k
    assert s["observed"].reshape(-1, 2, 2)[0].tolist() == [[True, True], [True, False]]
    assert np.isnan(s["obs"][..., 1, 1]).all() and np.isnan(s["post_mean"][..., 1, 1]).all()
    assert s["n_obs"].reshape(-1, 2)[0].tolist() == [2, 1]
    rmse = np.array([np.sqrt((0.01 ** 2 + 0.02 ** 2) / 2), 0.03])              # over the observed rows only
    assert np.allclose(s["rmse"].reshape(-1, 2)[0], rmse, rtol=1e-12)
    assert np.allclose(np.reshape(s["rmse_all"], -1)[0], np.sqrt((0.01 ** 2 + 0.02 ** 2 + 0.03 ** 2) / 3), rtol=1e-12)
    same = enkf_sm_summary(_table(P), 24, [0.02, 0.03])                         # one code path, two names
    assert all(np.array_equal(np.asarray(s[k]), np.asarray(same[k]), equal_nan=True) for k in same)


def test_a_sensor_never_observed_has_a_nan_rmse():
    t = _table()
    t[1, 1, :] = [0.0] + [np.nan] * 5
    s = filter_sm_summary(t, 24, [0.02, 0.03])
    assert np.isnan(s["rmse"][1]) and s["n_obs"].tolist() == [2, 0] and np.isfinite(s["rmse_all"])


class _Fake:
    """EnsembleSimulation.filter_summary without a handle: the tables come as arguments."""
    from hydromodel_amd.ensemble import _Run
    filter_summary, filter_sm_summary = _Run.filter_summary, _Run.filter_sm_summary
    filter_stride, filter_sigma_cm = 24, 10.0

    def __init__(self, record):
        self.filter_soil_moisture = record


def test_filter_summary_gains_sm_keys_only_with_a_record():
    ft = np.zeros((5, 4))
    ft[:, 1:] = np.nan
    ft[1] = [8, 6.5, -3.0, 5]
    ft[3] = [8, 7.0, -2.5, 6]
    plain = _Fake(None).filter_summary(ft)
    assert set(plain) == set(filter_summary(ft, 24, 10.0)) and not any(k.startswith("sm_") for k in plain)
    with_record = _Fake({"sigma": np.array([0.02, 0.03])}).filter_summary(ft, _table())
    sm = filter_sm_summary(_table(), 24, [0.02, 0.03])
    assert set(with_record) - set(plain) == {"sm_" + k for k in sm}
    assert with_record["sm_rows"].tolist() == [24, 72] and with_record["loglik"] == -5.5
