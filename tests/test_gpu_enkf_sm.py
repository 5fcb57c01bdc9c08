"""Soil-moisture sensors in the ensemble Kalman filter on the GPU (include/hydrocol.h hc_set_enkf_soil_moisture): the
observation operator against hc_model_nodes; Y, eps, the gain, the analysis states and the diagnostics against a float64
NumPy restatement from the forecast states; an all-NaN record against the well-only run; sensors of huge error against the
well-only run; invariance under launch length, point order and the dealing of a sweep's points to handles and ranks; a
twin experiment; resume; the CLI's "EnKF": {"Soil_Moisture": ...} block."""
import json
import re

import numpy as np
import pytest

from helpers import digest, golden
from helpers import cli_params as _cli_params, run_cli_ranks as _run_ranks
from test_enkf_sm_cpu import analysis_restated
from test_gpu_enkf import _eps_restated, _find_wtd, _fresh, _philox, _spread, _stepper, _y_of, M32

pytestmark = pytest.mark.gpu


def _eps_sensor(seed, gid, row, i):
    """Sensor i's eps: counter (0xFFFFFFF0 + i, row, gid_lo, gid_hi), the same Box-Muller step as the well's."""
    r = _philox((0xFFFFFFF0 + i, row, gid & M32, gid >> 32), (seed & M32, seed >> 32))
    a, b = (r[1] << 32) | r[0], (r[3] << 32) | r[2]
    u1 = ((a >> 11) + 0.5) / 9007199254740992.0
    u2 = ((b >> 11) + 0.5) / 9007199254740992.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def _record(T, nodes, row_values, rows=(48,)):
    """[T][n] NaN but on ``rows``, where sensor i reads row_values[i] (NaN: absent)."""
    v = np.full((T, len(nodes)), np.nan)
    for r in rows:
        v[r] = row_values
    return v


def _theta_at(st, psi):
    """hc_model_nodes' theta of the states ``psi`` [N][D] (the handle's state is replaced)."""
    st.set_state(psi)
    return st.model_nodes()["theta"]


SENSORS = {1: [12], 3: [6, 20, 45]}          # nodes (D = 101: 5 cm apart); deeper columns take the same nodes
VALUES = {1: [0.21], 3: [0.27, np.nan, 0.18, 0.24]}


@pytest.mark.parametrize("noise", ["philox", "numpy"])
@pytest.mark.parametrize("well, P, mpp, loc, n_s", [
    (1, 1, 100, 0.0, 1), (1, 3, 100, 60.0, 3), (300, 1, 100, 0.0, 3), (300, 2, 100, 50.0, 1),
    (1, 1, 2500, 0.0, 3), (1, 2, 2500, 80.0, 1),              # not a multiple of 64 or of a 256-member tile
])
def test_analysis_against_numpy(well, P, mpp, loc, n_s, noise):
    N = P * mpp
    st, cols, forcing = _stepper(well, N, P, noise)
    D, dz, sigma, seed = cols.dim_d, cols.dz, 5.0, 11
    nodes = SENSORS[n_s] if n_s == 1 else [6, 20, 33, 45]            # 3 sensors present of 4
    vals = VALUES[n_s]
    s_sig = np.array([0.02, 0.03, 0.015, 0.025][:len(nodes)])
    obs = int(forcing.wtd_obs[48])
    psat = float(cols.soil.psi_sat)
    try:
        st.set_enkf(48, sigma, loc, seed)
        st.set_enkf_soil_moisture(nodes, _record(st.T, nodes, vals), s_sig)
        kw = {"fresh_noise": _fresh(st, 1, 47, 1)} if noise == "numpy" else {}
        st.step_rows(1, 47, **kw)
        kw = {"fresh_noise": _fresh(st, 48, 1, 2)} if noise == "numpy" else {}
        out = st.step_rows(48, 1, want_wtd=True, want_psi=True, **kw)
        Y, K, eps_w, eps_s = st.enkf_sm_y(), st.enkf_sm_gain(), st.enkf_eps(), st.enkf_sm_eps()
        y_hook = st.enkf_y()
        post = st.get_state()
        table, smt = st.enkf_table(), st.enkf_sm_table()
        present = [i for i, v in enumerate(vals) if not np.isnan(v)]
        theta_f = _theta_at(st, out["psi"][0])[:, [nodes[i] for i in present]]
        theta_post = _theta_at(st, post)[:, [nodes[i] for i in present]]
    finally:
        st.close()
    W = 1 + len(present)
    assert Y.shape == (N, W) and K.shape == (P, D, W) and eps_s.shape == (N, len(nodes))
    w, forecast = out["wtd"][0].astype(np.int64), out["psi"][0]
    y_np = _y_of(forecast, w, psat, dz)
    assert np.all(np.abs(Y[:, 0] - y_np) <= 1e-12 * (1.0 + np.abs(y_np))) and np.array_equal(Y[:, 0], y_hook)
    assert np.array_equal(Y[:, 1:], theta_f)                                        # the operator: model_nodes' bits
    eps_np = np.array([_eps_restated(seed, m, 48) for m in range(N)])
    assert np.all(np.abs(eps_w - eps_np) <= 1e-13 * (1.0 + np.abs(eps_np)))
    es_np = np.array([[_eps_sensor(seed, m, 48, i) for i in range(len(nodes))] for m in range(N)])
    assert np.all(np.abs(eps_s - es_np) <= 1e-13 * (1.0 + np.abs(es_np)))
    o = np.concatenate([[obs * dz], np.asarray(vals)[present]])
    R = np.concatenate([[sigma], s_sig[present]]) ** 2
    zeta_nodes = np.array([nodes[i] for i in present]) * dz
    E = np.concatenate([eps_w[:, None], eps_s[:, present]], axis=1)
    res = analysis_restated(forecast, Y, E, o, R, zeta_nodes, dz, loc, mpp)
    assert np.all(np.abs(K - res["K"]) <= 1e-10 * np.abs(res["K"]).max() + 1e-300)
    assert np.abs(K[..., 1:]).max() > 0.0
    assert np.all(np.abs(post - res["post"]) <= 1e-9 * (1.0 + np.abs(res["post"])))
    assert not np.array_equal(post, forecast)
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        t = table[p, 1]
        assert t[0] == mpp and t[7] == 0
        assert abs(t[1] - res["ybar"][p, 0]) <= 1e-12 * abs(res["ybar"][p, 0])
        assert abs(t[4] - res["loglik"][p]) <= 1e-10 * max(1.0, abs(res["loglik"][p]))
        y_post = _y_of(post[sl], _find_wtd(post[sl], psat), psat, dz)
        assert abs(t[5] - y_post.mean()) <= 1e-9 * (1.0 + abs(y_post.mean()))
        assert abs(t[6] - y_post.std(ddof=1)) <= 1e-9 * (1.0 + y_post.std(ddof=1))
        s = smt[p, 1]
        for i in range(len(nodes)):
            if np.isnan(vals[i]):
                assert s[i, 0] == 0.0 and np.isnan(s[i, 1:]).all()
                continue
            k = present.index(i)
            th, tp = theta_f[sl, k], theta_post[sl, k]
            assert s[i, 0] == 1.0 and s[i, 1] == vals[i]
            assert abs(s[i, 2] - th.mean()) <= 1e-12 and abs(s[i, 3] - th.std(ddof=1)) <= 1e-10
            assert abs(s[i, 4] - tp.mean()) <= 1e-12 and abs(s[i, 5] - tp.std(ddof=1)) <= 1e-10
        assert np.isnan(smt[p, 2:]).all() and np.isnan(smt[p, 0]).all()


def _run(well, N, rows, record=None, sigma_s=0.02, seed=5, stride=48, hist=True):
    st, cols, _ = _stepper(well, N, seed=seed)
    try:
        if hist:
            st.set_wtd_hist(48)
        st.set_enkf(stride, 2.0 * cols.dz, 0.0, 3)
        if record is not None:
            nodes, values = record
            st.set_enkf_soil_moisture(nodes, values, sigma_s)
        st.step_rows(1, rows)
        return dict(psi=st.get_state(), moments=st.moments(), hist=st.wtd_hist_table() if hist else None,
                    table=st.enkf_table(), sm=st.enkf_sm_table() if record is not None else None, cols=cols, T=st.T)
    finally:
        st.close()


def test_an_all_nan_record_is_the_well_only_run():
    N, rows = 96, 150
    ref = _run(300, N, rows)
    got = _run(300, N, rows, record=([10, 40], np.full((ref["T"], 2), np.nan)))
    for k in ("psi", "moments", "hist", "table"):
        a, b = np.asarray(ref[k]), np.asarray(got[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert np.isnan(got["sm"]).all()


def test_sensors_of_huge_error_give_the_well_only_analysis():
    """sigma_i = 1e6 after ONE analysis.  The sensors' columns of the gain are K_di ~ c_{d,theta_i} / sigma_i^2 and their
    innovations ~ sigma_i eps_i, so their share of the increment is at most sum_i sd(psi_d) sd(theta_i) |eps_i| / sigma_i
    (|corr| <= 1), and their effect on the well's column is smaller still, O(sd(theta)^2 / sigma_i^2).  The well-only run
    solves an m' = 1 system, this one an m' = 4 system: 1e-9 relative on top covers that rounding.  The tolerance per node is
    2 sum_i sd(psi_d) sd(theta_i) max_k |eps_ki| / sigma_i + 1e-9 (1 + |psi|)."""
    N, well, big = 200, 1, 1.0e6
    ref = _run(well, N, 48, hist=False)
    nodes = [6, 20, 45]
    st, cols, forcing = _stepper(well, N, seed=5)
    try:
        st.set_enkf(48, 2.0 * cols.dz, 0.0, 3)
        st.set_enkf_soil_moisture(nodes, _record(st.T, nodes, [0.2, 0.25, 0.3]), big)
        st.step_rows(1, 47)
        out = st.step_rows(48, 1, want_psi=True)
        Y, eps_s, post = st.enkf_sm_y(), st.enkf_sm_eps(), st.get_state()
    finally:
        st.close()
    forecast = out["psi"][0]
    bound = 2.0 * forecast.std(axis=0, ddof=1) * sum(Y[:, 1 + i].std(ddof=1) * np.abs(eps_s[:, i]).max() / big
                                                   for i in range(3))
    diff = np.abs(post - ref["psi"])
    assert np.all(diff <= bound[None, :] + 1e-9 * (1.0 + np.abs(ref["psi"])))
    assert not np.array_equal(post, forecast)


NS, MPP, SEED = (1.6, 2.0, 2.4), 70, 31


def _point_handle(ids, rows_per_launch=0):
    from hydromodel_amd.stepper import EnsembleStepper
    from test_gpu_enkf import digest_point_like
    pts = [digest_point_like(NS[k]) for k in ids]
    psi_all = _spread(golden("g1_tables_1.npz")["initial_cond"], 3 * MPP, seed=4)
    st = EnsembleStepper([c for _, c, _ in pts], pts[0][2], len(ids) * MPP)
    try:
        st.set_generic_exponents(True)
        st.set_state(np.concatenate([psi_all[k * MPP:(k + 1) * MPP] for k in ids]))
        st.set_noise_philox(SEED, ids[0] * MPP)
        if len(ids) > 1:
            st.set_point_member_bases(np.array(ids, dtype=np.int64) * MPP)
        st.set_rows_per_launch(rows_per_launch)
        st.set_wtd_hist(48)
        st.set_enkf(24, 2.0 * st.cols.dz, 40.0, 9)
        v = _record(st.T, [8, 30], [0.22, 0.26], rows=(24, 72, 120))
        v[48] = [0.2, np.nan]                                   # one sensor; 96, 144: the well alone (m' = 1)
        st.set_enkf_soil_moisture([8, 30], v, [0.02, 0.03])
        st.step_rows(1, 150)
        n = len(ids)
        return dict(psi=st.get_state().reshape(n, MPP, -1), table=st.enkf_table(), sm=st.enkf_sm_table(),
                    moments=np.asarray(st.moments()).reshape(n, 3, -1), hist=st.wtd_hist_table().reshape(n, -1))
    finally:
        st.close()


def test_results_do_not_depend_on_launch_length_point_order_or_handles():
    whole = _point_handle([0, 1, 2])
    assert (whole["table"][:, 1:7, 0] == MPP).all()
    assert (whole["sm"][:, [1, 3, 5], :, 0] == 1.0).all() and (whole["sm"][:, 2, :, 0] == [1.0, 0.0]).all()
    assert np.isnan(whole["sm"][:, [4, 6]]).all()
    runs = {"rows 1": (_point_handle([0, 1, 2], 1), [0, 1, 2]), "rows 7": (_point_handle([0, 1, 2], 7), [0, 1, 2]),
            "reversed": (_point_handle([2, 1, 0]), [2, 1, 0]), "split a": (_point_handle([0, 2]), [0, 2]),
            "split b": (_point_handle([1]), [1])}
    for tag, (part, ids) in runs.items():
        for j, k in enumerate(ids):
            for key in ("psi", "table", "sm", "moments", "hist"):
                a, b = whole[key][k], part[key][j]
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (tag, k, key)


def _twin(rows, sensors):
    """well 1, 256 members, +-60 cm offsets, truth at +35 cm (another seed) as the well and, with ``sensors``, its theta
    at the sensor nodes plus noise every 48th row: forecast RMSE of the mean theta at those nodes against the truth's
    (profile statistics, the forecast), mean CRPS of the water table."""
    from hydromodel_amd.stepper import wtd_distribution
    from hydromodel_amd.synthetic import synthetic_soil_moisture
    import copy
    N, nodes, s_sig = 256, [6, 20, 45], 0.01
    psi0 = golden("g1_tables_1.npz")["initial_cond"]
    shifts = np.random.default_rng(12).uniform(-60.0, 60.0, size=N)
    truth, cols, forcing = _stepper(1, 1, seed=999, spread=False)
    try:
        truth.set_state(psi0 + 35.0)
        out = truth.step_rows(1, rows, want_wtd=True, want_psi=True)
        w_truth = out["wtd"][:, 0]
        arows = np.arange(48, rows + 1, 48)
        theta_truth = np.array([_theta_at(truth, out["psi"][r - 1])[0, nodes] for r in arows])
    finally:
        truth.close()
    twin = copy.copy(forcing)
    obs = np.array(forcing.wtd_obs, dtype=np.int32)
    obs[1:rows + 1] = np.where(obs[1:rows + 1] >= 0, w_truth, -1)
    obs[rows + 1:] = -1
    twin.wtd_obs = obs
    values = synthetic_soil_moisture(theta_truth, s_sig, seed=21, rows=arows, n_rows=forcing.dim_t)
    res = {}
    for tag in ("open", "well", "well+sensors"):
        st, _, _ = _stepper(1, N, seed=4, forcing=twin)
        try:
            st.set_state(psi0[None, :] + shifts[:, None])
            st.set_wtd_hist(48)
            st.set_profile_stats(48)
            if tag != "open":
                st.set_enkf(48, 2.0 * cols.dz, 0.0, 17)
            if tag == "well+sensors" and sensors:
                st.set_enkf_soil_moisture(nodes, values, s_sig)
            st.step_rows(1, rows)
            hist, prof = st.wtd_hist_table()[0], st.profile_stats()
        finally:
            st.close()
        mean_theta = np.asarray(prof["theta_vol_mean"]).reshape(-1, cols.dim_d)[1:len(arows) + 1][:, nodes]
        res[tag] = dict(crps=float(wtd_distribution(hist, obs, (0.5,), cols.dz, cols.z, 0, 48)["crps_mean_cm"]),
                        rmse=float(np.sqrt(np.mean((mean_theta - theta_truth) ** 2))))
    return res


def test_twin_experiment_sensors_lower_the_theta_rmse(capsys):
    res = _twin(10 * 48, sensors=True)
    with capsys.disabled():
        print("\n twin experiment, 256 members, 10 days, +-60 cm spread, 3 sensors (6, 20, 45), sigma 0.01: " +
              "; ".join(f"{k}: theta RMSE {v['rmse']:.5f}, CRPS {v['crps']:.4f} cm" for k, v in res.items()))
    assert res["well+sensors"]["rmse"] < res["well"]["rmse"]


def test_dump_and_restore_continue_a_sensor_run_bit_for_bit(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    from hydromodel_amd.stepper import soil_moisture_record
    _, cols, forcing = digest(1)
    psi0 = _spread(golden("g1_tables_1.npz")["initial_cond"], 96)
    v = _record(forcing.dim_t, [0, 1], [0.22, 0.26], rows=(48, 96, 144, 192, 240))
    rec = soil_moisture_record(cols.z, [cols.z[0] + 30.0, cols.z[0] + 100.0], v, 0.02)
    kw = dict(seed=6, psi0=psi0, wtd_hist_stride=48, enkf_stride=48, enkf_sigma_cm=2.0 * cols.dz,
              enkf_localisation_cm=50.0, enkf_soil_moisture=rec)
    whole = EnsembleSimulation(cols, forcing, 96, **kw)
    try:
        whole.advance(100)
        path = whole.dump(tmp_path / "ck.h5")
        whole.advance(140)
        want = [whole.stepper.get_state(), whole.enkf_table(), whole.enkf_sm_table(), whole.moments()]
        summary = whole.enkf_summary()
    finally:
        whole.close()
    with pytest.raises(ValueError, match="soil-moisture record"):
        EnsembleSimulation.restore(path, cols, forcing)
    back = EnsembleSimulation.restore(path, cols, forcing, enkf_soil_moisture=rec)
    try:
        back.advance(140)
        got = [back.stepper.get_state(), back.enkf_table(), back.enkf_sm_table(), back.moments()]
    finally:
        back.close()
    for a, b in zip(want, got):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert summary["sm_rows"].tolist() == [48, 96, 144, 192, 240] and summary["sm_rmse"].shape == (2,)
    assert np.isfinite(summary["sm_rmse"]).all() and np.isfinite(summary["sm_mean_innovation"]).all()


def test_refusals_and_what_turns_the_record_off():
    from hydromodel_amd import _lib as L
    st, cols, _ = _stepper(1, 8)
    T = st.T
    try:
        with pytest.raises(L.HcError, match="the EnKF is off"):
            st.set_enkf_soil_moisture([3], np.full((T, 1), np.nan), 0.02)
        st.set_enkf(48, 5.0, 0.0, 1)
        for nodes, vals, sig in (([cols.dim_d], np.nan, 0.02), ([3], 1.5, 0.02), ([3], -0.1, 0.02), ([3], np.nan, 0.0),
                                 ([3], np.nan, np.inf), (list(range(9)), np.nan, 0.02)):
            with pytest.raises(L.HcError):
                st.set_enkf_soil_moisture(nodes, np.full((T, len(nodes)), vals), sig)
        st.set_enkf_soil_moisture([3], np.full((T, 1), 0.2), 0.02)
        assert st.enkf_sm_table().shape == (1, (T - 1) // 48 + 1, 1, 6)
        st.set_enkf(48, 5.0, 0.0, 1)                             # hc_set_enkf removes the record
        with pytest.raises(L.HcError, match="no soil-moisture record"):
            L.check(st.lib.hc_get_enkf_sm_stats(st.h, L.dptr(np.zeros(1)), -1))
        st.set_enkf_soil_moisture([3], np.full((T, 1), 0.2), 0.02)
        st.set_noise_philox(2, 0)                                # a new noise source turns the EnKF off, and the record
        with pytest.raises(L.HcError):
            L.check(st.lib.hc_get_enkf_sm_stats(st.h, L.dptr(np.zeros(1)), -1))
    finally:
        st.close()


SM_KEYS = {"enkf_sm_depths_cm", "enkf_sm_nodes", "enkf_sm_sigma", "enkf_sm_observed", "enkf_sm_obs",
           "enkf_sm_prior_mean", "enkf_sm_prior_std", "enkf_sm_post_mean", "enkf_sm_post_std"}


def _sensor_csv(tmp_path, n_depths, every=24):
    from hydromodel_amd.synthetic import synthetic_forcing, write_soil_moisture_csv
    _, datenum, _, _ = synthetic_forcing(1)
    v = np.full((datenum.size, n_depths), np.nan)
    rng = np.random.default_rng(3)
    v[::every] = rng.uniform(0.15, 0.3, size=v[::every].shape)
    v[48::96, -1] = np.nan
    return str(write_soil_moisture_csv(tmp_path / "sm.csv", v, datenum))


def test_cli_soil_moisture_block_writes_the_datasets(tmp_path, monkeypatch, capsys):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    params = _cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    sm = {"Filename": _sensor_csv(tmp_path, 2), "Depths_cm": [30, 120], "Sigma": [0.02, 0.03]}
    files, logs = {}, {}
    pts = [{"Soil_Properties": {"n": 1.6}}, {"Soil_Properties": {"n": 2.4}}]
    for tag, extra in (("well", {"EnKF": {"Stride": 24, "Sigma_cm": 10.0}}),
                       ("ens", {"EnKF": {"Stride": 24, "Sigma_cm": 10.0, "Soil_Moisture": sm}}),
                       ("sweep", {"Points": pts, "EnKF": {"Sigma_cm": 10.0, "Soil_Moisture": sm}})):
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 64, "Seed": 3, "Days": 2, **extra}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = loadResults(tmp_path / f"Run_{tag}_ensemble.h5")
        logs[tag] = capsys.readouterr().out
    well, ens, sweep = files["well"], files["ens"], files["sweep"]
    assert "soil-moisture" not in logs["well"] and set(ens) - set(well) == SM_KEYS
    assert ens["enkf_rows"].tolist() == [24, 48, 72, 96]
    assert ens["enkf_sm_nodes"].tolist() == [6, 24] and ens["enkf_sm_depths_cm"].tolist() == [30.0, 120.0]
    assert ens["enkf_sm_observed"].tolist() == [[1, 1], [1, 0], [1, 1], [1, 1]]
    for k in SM_KEYS - {"enkf_sm_depths_cm", "enkf_sm_nodes", "enkf_sm_sigma"}:
        assert ens[k].shape == (4, 2), k
    assert np.isnan(ens["enkf_sm_prior_mean"][1, 1]) and np.isfinite(ens["enkf_sm_post_std"][0]).all()
    rmse = np.sqrt(np.nanmean((ens["enkf_sm_obs"] - ens["enkf_sm_prior_mean"]) ** 2))
    line = re.search(r"\[Ensemble x64\] soil-moisture forecast RMSE = ([0-9.]+) over 4 rows", logs["ens"])
    assert line and abs(float(line.group(1)) - rmse) <= 1e-5
    assert sweep["enkf_sm_obs"].shape == (2, 2, 2) and sweep["enkf_rows"].tolist() == [48, 96]
    assert "[Sweep 2 points x64] soil-moisture forecast RMSE: best point " in logs["sweep"]


def test_a_sensor_sweep_on_two_ranks_writes_what_one_rank_writes(tmp_path):
    params = _cli_params(tmp_path)
    sm = {"Filename": _sensor_csv(tmp_path, 3), "Depths_cm": [20, 60, 150], "Sigma": 0.02}
    params["Ensemble"] = {"Members": 40, "Seed": 5, "Days": 2, "Distribution": {"Stride": 48},
                          "Points": [{"Soil_Properties": {"n": n}} for n in (1.6, 2.0, 2.2, 2.4)],
                          "EnKF": {"Stride": 24, "Sigma_cm": 8.0, "Soil_Moisture": sm}}
    one, log1 = _run_ranks(tmp_path, "one", params, 1)
    two, log2 = _run_ranks(tmp_path, "two", params, 2)
    for k in sorted(SM_KEYS) + ["enkf_loglik_rows", "enkf_post_mean_cm", "moments", "wtd_hist"]:
        a, b = np.asarray(one[k]), np.asarray(two[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert one["enkf_sm_obs"].shape == (4, 4, 3)
    line = [s for s in log1.splitlines() if "soil-moisture forecast RMSE" in s]
    assert len(line) == 1 and line == [s for s in log2.splitlines() if "soil-moisture forecast RMSE" in s]
