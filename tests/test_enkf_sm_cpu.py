"""Soil-moisture sensors in the EnKF on the host (no GPU): the C-ABI entries, the CLI's "Soil_Moisture" validator and its
refusals before any GPU call, the sensor CSV, the depth -> node rule, a NumPy restatement of the batch analysis (used by
the GPU tests too), the sensors' summary and the [P] assembly of their float64 table over two ranks
(include/hydrocol.h hc_set_enkf_soil_moisture)."""
import json
import os
import re
import socket
from pathlib import Path

import numpy as np
import pytest
import torch.multiprocessing as mp

from hydromodel_amd import multigpu
from hydromodel_amd.cli import enkf_settings, read_soil_moisture_csv, run_cli, soil_moisture_settings
from hydromodel_amd.stepper import (SM_WIDTH, enkf_sm_summary, gaspari_cohn, place_points, sensor_nodes,
                                    soil_moisture_record)

REPO = Path(__file__).resolve().parent.parent
NEW_ENTRIES = ("hc_set_enkf_soil_moisture", "hc_get_enkf_sm_stats", "hc_set_enkf_sm_stats", "hc_get_enkf_sm_width",
               "hc_get_enkf_sm_y", "hc_get_enkf_sm_gain", "hc_get_enkf_sm_eps")


def analysis_restated(psi, Y, E, o, R, zeta_nodes, dz, loc, mpp):
    """The batch analysis per point in float64 (include/hydrocol.h hc_set_enkf_soil_moisture): two-pass means and
    anomalies over the point's members, C_YY and C_psiY / (N_p - 1), the Gaspari-Cohn taper on both (zeta = ybar for the
    well, the sensors' depths ``zeta_nodes`` from the top node), K = (rho o C_psiY)(rho o C_YY + R)^-1 by a Cholesky
    factor, psi + K (o + sqrt(R) E - Y), and the joint log-density of ``o`` under N(Ybar, C_YY + R), untapered.
    psi [N][D], Y / E [N][m'], o / R [m']."""
    N, D = psi.shape
    W = Y.shape[1]
    P = N // mpp
    z = np.arange(D) * dz
    K, ybar, loglik = np.zeros((P, D, W)), np.zeros((P, W)), np.zeros(P)
    post = psi.copy()
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        yb = Y[sl].mean(axis=0)
        A = Y[sl] - yb
        n1 = mpp - 1
        cyy = A.T @ A / n1 if mpp > 1 else np.zeros((W, W))
        cpy = (psi[sl] - psi[sl].mean(axis=0)).T @ A / n1 if mpp > 1 else np.zeros((D, W))
        zeta = np.concatenate([[yb[0]], np.asarray(zeta_nodes, dtype=np.float64)])
        if loc > 0:
            rho_yy = gaspari_cohn(np.abs(zeta[:, None] - zeta[None, :]) / loc)
            rho_py = gaspari_cohn(np.abs(z[:, None] - zeta[None, :]) / loc)
        else:
            rho_yy, rho_py = np.ones((W, W)), np.ones((D, W))
        L = np.linalg.cholesky(rho_yy * cyy + np.diag(R))
        # K^T = S^-1 (rho o C_psiY)^T: forward, then backward substitution
        u = np.linalg.solve(L, (rho_py * cpy).T)
        K[p] = np.linalg.solve(L.T, u).T
        innov = (o[None, :] + np.sqrt(R)[None, :] * E[sl]) - Y[sl]
        post[sl] = psi[sl] + innov @ K[p].T
        Lu = np.linalg.cholesky(cyy + np.diag(R))
        w = np.linalg.solve(Lu, o - yb)
        loglik[p] = -0.5 * (W * np.log(2.0 * np.pi) + 2.0 * np.log(np.diag(Lu)).sum() + w @ w)
        ybar[p] = yb
    return {"K": K, "post": post, "ybar": ybar, "loglik": loglik}


def test_header_declares_and_the_binding_lists_the_sensor_entries():
    text = (REPO / "include" / "hydrocol.h").read_text()
    from hydromodel_amd import _lib as L
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in L.EXPORTS, name


def _ens(sm, **enkf):
    return {"Members": 8, "EnKF": {"Sigma_cm": 10.0, **enkf, "Soil_Moisture": sm}}


SM = {"Filename": "sm.csv", "Depths_cm": [30, 60, 120], "Sigma": 0.02}


@pytest.mark.parametrize("sm, want", [
    (SM, ("sm.csv", (30.0, 60.0, 120.0), (0.02, 0.02, 0.02))),
    (dict(SM, Sigma=[0.01, 0.02, 0.5]), ("sm.csv", (30.0, 60.0, 120.0), (0.01, 0.02, 0.5))),
    (dict(SM, Depths_cm=[10.5], Sigma=[3]), ("sm.csv", (10.5,), (3.0,))),
    (dict(SM, Depths_cm=list(range(8))), ("sm.csv", tuple(float(d) for d in range(8)), (0.02,) * 8)),
])
def test_soil_moisture_settings_accepts(sm, want):
    assert soil_moisture_settings(_ens(sm), 1) == want
    assert enkf_settings(_ens(sm), 1) == (48, 10.0, 0.0, None)                   # the EnKF's 4-tuple stays
    assert soil_moisture_settings({"Members": 8, "EnKF": {"Sigma_cm": 1.0}}) is None
    assert soil_moisture_settings({"Members": 8}) is None


def test_a_sweep_with_sensors_runs_on_several_ranks():
    ens = dict(_ens(SM), Points=[{}, {}])
    assert soil_moisture_settings(ens, 2)[1] == (30.0, 60.0, 120.0)


@pytest.mark.parametrize("ens, gpus, message", [
    (_ens(dict(SM, Sigma=0.0)), 1, "Soil_Moisture.Sigma = 0.0 must be a finite number > 0 or one per depth (3)"),
    (_ens(dict(SM, Sigma=-1)), 1, "Soil_Moisture.Sigma = -1 must be a finite number > 0"),
    (_ens(dict(SM, Sigma=float("nan"))), 1, "Soil_Moisture.Sigma = nan must be a finite number > 0"),
    (_ens(dict(SM, Sigma=[0.1, 0.2])), 1, "Soil_Moisture.Sigma = [0.1, 0.2] must be a finite number > 0 or one per depth"),
    (_ens(dict(SM, Sigma=[0.1, True, 0.2])), 1, "must be a finite number > 0 or one per depth"),
    (_ens(dict(SM, Sigma="0.02")), 1, "Soil_Moisture.Sigma = '0.02' must be a finite number > 0"),
    (_ens({k: v for k, v in SM.items() if k != "Sigma"}), 1, "Soil_Moisture.Sigma (the sensors' error, m^3/m^3) is required"),
    (_ens(dict(SM, Depths_cm=list(range(9)))), 1, "Soil_Moisture.Depths_cm has 9 depths, at most 8"),
    (_ens(dict(SM, Depths_cm=[])), 1, "Soil_Moisture.Depths_cm = [] must be a non-empty list"),
    (_ens(dict(SM, Depths_cm=[10, float("inf")])), 1, "must be a non-empty list of finite depths"),
    (_ens(dict(SM, Depths_cm=30)), 1, "Soil_Moisture.Depths_cm = 30 must be a non-empty list"),
    (_ens(dict(SM, Filename=None)), 1, "Soil_Moisture.Filename = None must name the sensor CSV"),
    (_ens(dict(SM, Bogus=1)), 1, "Soil_Moisture has unknown keys ['Bogus']"),
    (_ens(["sm.csv"]), 1, "EnKF.Soil_Moisture = ['sm.csv'] must be an object"),
    (_ens(SM, Stride=0), 1, "EnKF.Soil_Moisture needs an active EnKF (EnKF.Stride > 0)"),
    ({"Members": 8, "Soil_Moisture": SM}, 1, "Soil_Moisture belongs inside the \"EnKF\" block"),
    (dict(_ens(SM), Filter={"Sigma_cm": 1.0}), 1, '"Filter" and "EnKF" exclude each other'),
    (_ens(SM), 2, "EnKF with one parameter point runs on one GPU (2 requested)"),
    ({"Members": 8, "EnKF": {"Soil_Moisture": SM}}, 1, "EnKF.Sigma_cm (the observation error of the well, cm) is required"),
])
def test_soil_moisture_settings_rejects(ens, gpus, message):
    with pytest.raises(ValueError) as err:
        soil_moisture_settings(ens, gpus)
    assert message in str(err.value)


def test_the_enkf_validator_knows_the_key_and_still_names_unknown_ones():
    assert enkf_settings(_ens(SM), 1)[0] == 48
    with pytest.raises(ValueError, match=re.escape("EnKF has unknown keys ['Soil_moisture']")):
        enkf_settings({"Members": 8, "EnKF": {"Sigma_cm": 1.0, "Soil_moisture": SM}}, 1)


@pytest.mark.parametrize("ens, message", [
    (_ens(dict(SM, Depths_cm=list(range(9)))), "Soil_Moisture.Depths_cm has 9 depths, at most 8"),
    (_ens(dict(SM, Sigma=0)), "Soil_Moisture.Sigma = 0 must be a finite number > 0"),
    (_ens(SM, Stride=0), "EnKF.Soil_Moisture needs an active EnKF"),
    (dict(_ens(SM), Filter={"Sigma_cm": 1.0}), '"Filter" and "EnKF" exclude each other'),
    (dict(_ens(SM), GPUs=2), "EnKF with one parameter point runs on one GPU (2 requested)"),
])
def test_a_bad_soil_moisture_block_ends_the_command_with_status_1_before_any_gpu_call(tmp_path, capsys, ens, message):
    from hydromodel_amd.synthetic import default_parameters
    params = default_parameters()
    params["Data_Filename"] = str(tmp_path / "missing.csv")          # never reached: the block is refused first
    params["Ensemble"] = ens
    (tmp_path / "p.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as stop:
        run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "p.json")])
    assert stop.value.code == 1
    out = capsys.readouterr().out
    assert message in out and "missing.csv" not in out


def _cli_run(tmp_path, capsys, sm_csv, depths=(30, 60)):
    """The CLI up to the sensor record: forcing, site and sensor files exist; the run must stop with status 1 before the
    ensemble touches a GPU (this test needs none)."""
    from hydromodel_amd.synthetic import default_parameters, write_forcing_csv, write_site_information, synthetic_well
    params = default_parameters()
    params["Site_Information"] = str(write_site_information(tmp_path / "site.json", {10: synthetic_well(200)}))
    params["Data_Filename"] = str(write_forcing_csv(tmp_path / "forcing.csv", 1))
    params["Ensemble"] = _ens(dict(SM, Filename=str(sm_csv), Depths_cm=list(depths)))
    (tmp_path / "p.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as stop:
        run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "p.json")])
    return stop.value.code, capsys.readouterr().out


def _csv_values(T, n, seed=1):
    v = np.random.default_rng(seed).uniform(0.1, 0.4, size=(T, n))
    v[::3, 0] = np.nan
    return v


def test_the_sensor_csv_round_trips_and_misaligned_or_bad_files_are_refused(tmp_path):
    from hydromodel_amd.synthetic import synthetic_forcing, write_soil_moisture_csv
    _, datenum, _, _ = synthetic_forcing(1)
    T = datenum.size
    v = _csv_values(T, 2)
    path = write_soil_moisture_csv(tmp_path / "sm.csv", v, datenum)
    assert path.read_text().splitlines()[0].startswith("1,733682.0,,")          # an empty field: no observation
    got = read_soil_moisture_csv(path, datenum, 2)
    assert np.array_equal(np.isnan(got), np.isnan(v)) and np.array_equal(got[~np.isnan(got)], v[~np.isnan(v)])
    shifted = datenum.copy()
    shifted[100] += 1.0 / 48.0
    write_soil_moisture_csv(tmp_path / "shift.csv", v, shifted)
    with pytest.raises(ValueError, match="row 101 has Datenum"):
        read_soil_moisture_csv(tmp_path / "shift.csv", datenum, 2)
    write_soil_moisture_csv(tmp_path / "short.csv", v[:-1], datenum[:-1])
    with pytest.raises(ValueError, match=f"has {T - 1} rows, the forcing {T}"):
        read_soil_moisture_csv(tmp_path / "short.csv", datenum, 2)
    with pytest.raises(ValueError, match="row 1 has 4 fields, expected 5"):
        read_soil_moisture_csv(path, datenum, 3)
    bad = v.copy()
    bad[7, 1] = 1.25
    write_soil_moisture_csv(tmp_path / "bad.csv", bad, datenum)
    with pytest.raises(ValueError, match=r"row 8 value 2 = 1.25 lies outside \[0, 1\]"):
        read_soil_moisture_csv(tmp_path / "bad.csv", datenum, 2)
    bad[7, 1] = -0.01
    write_soil_moisture_csv(tmp_path / "neg.csv", bad, datenum)
    with pytest.raises(ValueError, match="lies outside"):
        read_soil_moisture_csv(tmp_path / "neg.csv", datenum, 2)


@pytest.mark.parametrize("case", ["misaligned", "out of range", "depth", "missing"])
def test_a_bad_sensor_file_or_depth_ends_the_command_with_status_1_before_any_gpu_call(tmp_path, capsys, monkeypatch,
                                                                                       case):
    from hydromodel_amd import ensemble
    from hydromodel_amd.synthetic import synthetic_forcing, write_soil_moisture_csv

    def no_gpu(*a, **k):
        raise AssertionError("a GPU handle was created")
    monkeypatch.setattr(ensemble, "EnsembleStepper", no_gpu)
    _, datenum, _, _ = synthetic_forcing(1)
    v = _csv_values(datenum.size, 2)
    depths = (30, 60)
    if case == "misaligned":
        datenum = datenum + 0.5
    if case == "out of range":
        v[5, 0] = 2.0
    if case == "depth":
        depths = (30, 5000)
    path = tmp_path / ("nowhere.csv" if case == "missing" else "sm.csv")
    if case != "missing":
        write_soil_moisture_csv(path, v, datenum)
    code, out = _cli_run(tmp_path, capsys, path, depths)
    assert code == 1
    want = {"misaligned": "row 1 has Datenum", "out of range": "lies outside [0, 1]",
            "depth": "sensor depth 5000.0 cm lies outside the column [0.0, 995.0] cm",
            "missing": "the sensor file"}[case]
    assert want in out


def test_depth_to_node_follows_the_reference_rule():
    """src/simulation.py:255: z_grid[z_grid >= k][0] -- the first node at or below the depth."""
    z = np.linspace(0.0, 500.0, 101)                                 # dz = 5
    for d in (0.0, 0.1, 4.999, 5.0, 5.0001, 30.0, 62.5, 499.9, 500.0):
        want = z[z >= d][0]
        assert z[sensor_nodes(z, [d])[0]] == want, d
    zo = np.linspace(20.0, 520.0, 101)                               # a column whose top node is not at 0
    assert sensor_nodes(zo, [20.0, 21.0, 520.0]).tolist() == [0, 1, 100]
    for d in (-0.1, 19.99, 520.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lies outside the column"):
            sensor_nodes(zo, [d])
    rec = soil_moisture_record(z, [30, 62.5], np.zeros((4, 2)), 0.02)
    assert rec["nodes"].tolist() == [6, 13] and rec["sigma"].tolist() == [0.02, 0.02] and rec["values"].shape == (4, 2)


def test_the_restated_analysis_is_the_kalman_update_and_the_gaussian_density():
    from scipy.stats import multivariate_normal
    rng = np.random.default_rng(5)
    mpp, P, D, W, dz = 40, 2, 30, 4, 5.0
    psi = rng.standard_normal((P * mpp, D)) * 30.0 - 200.0
    Y = np.column_stack([rng.uniform(50, 80, P * mpp), rng.uniform(0.1, 0.3, (P * mpp, W - 1))])
    Y[:, 1] += 0.001 * psi[:, 4]                                       # correlated with the states
    E = rng.standard_normal((P * mpp, W))
    o = np.array([66.0, 0.2, 0.22, 0.18])
    R = np.array([25.0, 4e-4, 1e-4, 9e-4])
    for loc in (0.0, 40.0):
        res = analysis_restated(psi, Y, E, o, R, [10.0, 45.0, 90.0], dz, loc, mpp)
        for p in range(P):
            sl = slice(p * mpp, (p + 1) * mpp)
            cyy = np.cov(Y[sl].T)
            cpy = np.array([[np.cov(psi[sl, d], Y[sl, i])[0, 1] for i in range(W)] for d in range(D)])
            zeta = np.array([Y[sl, 0].mean(), 10.0, 45.0, 90.0])
            rho_yy = gaspari_cohn(np.abs(zeta[:, None] - zeta[None, :]) / loc) if loc else 1.0
            rho_py = gaspari_cohn(np.abs(np.arange(D)[:, None] * dz - zeta[None, :]) / loc) if loc else 1.0
            K = (rho_py * cpy) @ np.linalg.inv(rho_yy * cyy + np.diag(R))      # the direct inverse
            assert np.allclose(res["K"][p], K, rtol=1e-10, atol=1e-12 * np.abs(K).max())
            post = psi[sl] + ((o + np.sqrt(R) * E[sl]) - Y[sl]) @ K.T
            assert np.allclose(res["post"][sl], post, rtol=1e-12, atol=1e-9)
            want = multivariate_normal(mean=Y[sl].mean(axis=0), cov=cyy + np.diag(R)).logpdf(o)
            assert abs(res["loglik"][p] - want) <= 1e-10 * abs(want)
    # one observation: the scalar EnKF of hc_set_enkf (K = c / (v + sigma^2) and its increment)
    one = analysis_restated(psi, Y[:, :1], E[:, :1], o[:1], R[:1], [], dz, 0.0, mpp)
    sl = slice(0, mpp)
    v = Y[sl, 0].var(ddof=1)
    c = ((psi[sl] - psi[sl].mean(axis=0)) * (Y[sl, 0] - Y[sl, 0].mean())[:, None]).sum(axis=0) / (mpp - 1)
    assert np.allclose(one["K"][0, :, 0], c / (v + R[0]), rtol=1e-12)
    d = o[0] - Y[sl, 0].mean()
    assert abs(one["loglik"][0] - (-0.5 * np.log(2 * np.pi * (v + R[0])) - 0.5 * d * d / (v + R[0]))) < 1e-12


def test_enkf_sm_summary_forms_the_forecast_rmse_per_sensor():
    stride, n_arow, n = 48, 6, 2
    t = np.full((n_arow, n, SM_WIDTH), np.nan)
    t[1] = [[1, 0.30, 0.25, 0.01, 0.28, 0.005], [1, 0.20, 0.22, 0.02, 0.21, 0.01]]
    t[2, 0] = [1, 0.31, 0.28, 0.01, 0.30, 0.005]
    t[2, 1, 0] = 0.0                                                    # not observed on that row
    t[4] = [[1, 0.29, 0.29, 0.01, 0.29, 0.005], [1, 0.24, 0.20, 0.02, 0.23, 0.01]]
    s = enkf_sm_summary(t, stride, [0.02, 0.03])
    assert s["rows"].tolist() == [48, 96, 192] and s["observed"].tolist() == [[True, True], [True, False], [True, True]]
    assert np.allclose(s["rmse"], [np.sqrt((0.05 ** 2 + 0.03 ** 2 + 0.0) / 3), np.sqrt((0.02 ** 2 + 0.04 ** 2) / 2)])
    assert np.allclose(s["mean_innovation"], [(0.05 + 0.03) / 3, (-0.02 + 0.04) / 2]) and s["n_obs"].tolist() == [3, 2]
    assert np.isclose(s["rmse_all"], np.sqrt((0.05 ** 2 + 0.03 ** 2 + 0.02 ** 2 + 0.04 ** 2) / 5))
    two = enkf_sm_summary(np.stack([t, t]), stride, 0.02)
    assert two["rmse"].shape == (2, 2) and two["rmse_all"].shape == (2,)
    empty = enkf_sm_summary(np.full((n_arow, n, SM_WIDTH), np.nan), stride, 0.02)
    assert empty["rows"].size == 0 and np.isnan(empty["rmse"]).all()


def _sm_table(P, n_arow, n, seed):
    rng = np.random.default_rng(seed)
    t = np.full((P, n_arow, n, SM_WIDTH), np.nan)
    t[:, 1:4] = rng.uniform(0.0, 0.5, size=(P, 3, n, SM_WIDTH))
    t[:, 1:4, :, 0] = 1.0
    t[0, 2, 1] = [0.0] + [np.nan] * (SM_WIDTH - 1)
    t[0, 1, 0, 3] = -0.0
    t[-1, -1, 0, 5] = np.frombuffer(np.array([0x7FF8_0000_DEAD_BEEF], dtype=np.uint64).tobytes(), dtype=np.float64)[0]
    return t


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _place_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), HYDROCOL_DIST_BACKEND="gloo")
    ranks = multigpu.Ranks(expect=world)
    whole = _sm_table(5, 6, 3, 7)
    mine = [k for k in range(5) if k % world == rank]             # round-robin, as deal_points
    total = place_points(whole[mine], mine, 5, ranks)
    np.save(os.path.join(out_dir, f"r{rank}.npy"), total)
    ranks.close()


def test_gloo_world2_assembly_of_the_sensor_table_keeps_every_bit(tmp_path):
    mp.spawn(_place_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    whole = _sm_table(5, 6, 3, 7)
    for r in range(2):
        got = np.load(tmp_path / f"r{r}.npy")
        assert got.dtype == np.float64 and got.shape == whole.shape
        assert np.array_equal(got.view(np.int64), whole.view(np.int64))     # NaN payloads and -0.0 included
        assert np.signbit(got[0, 1, 0, 3]) and np.isnan(got[0, 0, 0, 1])
