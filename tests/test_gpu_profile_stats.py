"""Ensemble profile statistics reduced on the GPU (include/hydrocol.h hc_set_profile_stats): the library's int64 tables
against a host restatement from hc_get_state / hc_model_nodes / diag_out, against numpy over psi_rows_out, their
invariance under launch length, member split, depth and parameter points, no side effects on the run, resume, and the
CLI's "Ensemble": {"Profiles": ...} block.  Reference surface: Simulation.run's outputs, simulation.py:658-671."""
import json

import numpy as np
import pytest

from helpers import WELLS, cli_params, digest, digest_point, golden, run_cli_ranks

pytestmark = pytest.mark.gpu

ROWS = 96                                                   # two days


def _stepper(well, N, stride, noise="philox", points=None, seed=7, offset=0, bases=None):
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(well)
    ic = golden(f"g1_tables_{well}.npz")["initial_cond"]
    st = EnsembleStepper(points or cols, forcing, N)
    st.set_state(ic)
    if noise == "numpy":
        st.set_noise_host(np.random.default_rng(seed + offset).standard_normal((N, cols.dim_d)))
    else:
        st.set_noise_philox(seed, offset)
        if bases is not None:
            st.set_point_member_bases(np.asarray(bases))
    st.set_profile_stats(stride)
    st.profile_snapshot(0)
    return st, cols, forcing


def _fresh(forcing, N, D, r0, n, rng):
    k = int((forcing.refresh[r0:r0 + n].astype(bool) & (forcing.wtd_obs[r0:r0 + n] >= 0)).sum())
    return rng.standard_normal((k, N, D))


@pytest.mark.parametrize("noise", ["philox", "numpy"])
def test_tables_equal_a_host_restatement_exactly(noise):
    """64 members, D = 300, two days, stride 1, one row per call: psi from hc_get_state, theta from hc_model_nodes, the
    fluxes from diag_out and the water table from wtd_out, quantised and summed with Python integers on the host."""
    from hydromodel_amd.stepper import (PROF_SCALE_FLUX, PROF_SCALE_PSI, PROF_SCALE_THETA, join_profile_table,
                                        profile_layout, profile_quantise, profile_words_of)
    N = 64
    st, cols, forcing = _stepper(300, N, 1, noise=noise)
    T, D = forcing.dim_t, cols.dim_d
    parts = {k: np.zeros(sh, dtype=np.int64) for k, (_, sh) in profile_layout(1, T, D, 1).items() if k != "words"}
    clamps = 0

    def add_profile(r):
        nonlocal clamps
        qp, b1 = profile_quantise(st.get_state(), PROF_SCALE_PSI)
        qt, b2 = profile_quantise(st.model_nodes()["theta"], PROF_SCALE_THETA)
        parts["prof"][0, r, :, 0] = profile_words_of(qp).sum(axis=0)
        parts["prof"][0, r, :, 1] = profile_words_of(qt).sum(axis=0)
        parts["pcnt"][0, r] = N
        clamps += b1 + b2

    rng = np.random.default_rng(1)
    # row 5 becomes a skip row (observation off the grid, simulation.py:582-588): it counts nobody
    wtd_obs = np.asarray(forcing.wtd_obs).copy()
    wtd_obs[5] = -1
    st.lib.hc_set_forcing_row(st.h, 5, float(forcing.precip[5]), float(forcing.atm[5]),
                              int(forcing.daylight[5]) | (int(forcing.wet_season[5]) << 1), -1)
    try:
        add_profile(0)
        for r in range(1, ROWS + 1):
            kw = {"fresh_noise": _fresh(forcing, N, D, r, 1, rng)} if noise == "numpy" else {}
            out = st.step_rows(r, 1, want_wtd=True, want_diag=True, **kw)
            obs = int(wtd_obs[r])
            if obs < 0:
                continue
            add_profile(r)
            for k in range(2):
                q, b = profile_quantise(out["diag"][0, :, k], PROF_SCALE_FLUX)
                parts["flux"][0, r, k] = profile_words_of(q).sum(axis=0)
                clamps += b
            parts["fcnt"][0, r] = N
            parts["aerr"][0, r] = int(np.abs(obs - out["wtd"][0].astype(np.int64)).sum())
        table = st.profile_table()
        assert clamps == 0 and st.profile_overflow() == 0
        assert np.array_equal(table, join_profile_table(parts))
        stats = st.profile_stats()
        solved = np.flatnonzero(wtd_obs[1:ROWS + 1] >= 0) + 1
        assert solved.size == ROWS - 1 and np.all(stats["row_count"][solved] == N)
        assert stats["row_count"][5] == 0 and stats["count"][5] == 0 and np.isnan(stats["theta_vol_mean"][5]).all()
        assert np.all(np.isfinite(stats["abs_error_mean"][solved]))
    finally:
        st.close()


def test_stats_agree_with_numpy_over_psi_rows_and_row_zero_is_the_initial_condition():
    from hydromodel_amd.stepper import PROF_SCALE_FLUX, PROF_SCALE_PSI
    N = 64
    st, cols, forcing = _stepper(300, N, 1)
    ic = golden("g1_tables_300.npz")["initial_cond"]
    try:
        out = st.step_rows(1, ROWS, want_psi=True, want_diag=True, want_wtd=True)
        s = st.profile_stats()
    finally:
        st.close()
    assert s["count"][0] == N and np.all(s["psi_press_std"][0] == 0.0)
    assert np.max(np.abs(s["psi_press_mean"][0] - ic)) <= 2.0 ** -(PROF_SCALE_PSI + 1)
    solved = [r for r in range(1, ROWS + 1) if forcing.wtd_obs[r] >= 0]
    assert len(solved) > 0
    for r in solved:
        psi, diag = out["psi"][r - 1], out["diag"][r - 1]
        assert np.max(np.abs(s["psi_press_mean"][r] - psi.mean(axis=0))) <= 2.0 ** -PROF_SCALE_PSI
        assert np.max(np.abs(s["psi_press_std"][r] - psi.std(axis=0))) <= 2.0 ** -PROF_SCALE_PSI
        for k, key in enumerate(("transpiration", "lateral_flow")):
            assert abs(s[key + "_mean"][r] - diag[:, k].mean()) <= 2.0 ** -PROF_SCALE_FLUX
            assert abs(s[key + "_std"][r] - diag[:, k].std()) <= 2.0 ** -PROF_SCALE_FLUX
        wtd_idx = out["wtd"][r - 1].astype(float)
        assert s["abs_error_mean"][r] == pytest.approx(cols.dz * np.abs(forcing.wtd_obs[r] - wtd_idx).mean(), rel=1e-14)
    assert np.all((s["theta_vol_mean"][solved] > 0) & (s["theta_vol_mean"][solved] <= 1))


def _run(well, N, stride, rpl=0, offset=0, points=None, bases=None, rows=ROWS):
    st, _, _ = _stepper(well, N, stride, offset=offset, points=points, bases=bases)
    try:
        if rpl:
            st.set_rows_per_launch(rpl)
        st.step_rows(1, rows)
        assert st.profile_overflow() == 0
        return st.profile_table()
    finally:
        st.close()


def test_tables_do_not_depend_on_the_launch_length():
    ref = _run(300, 64, 5)
    assert np.array_equal(_run(300, 64, 5, rpl=1), ref)
    assert np.array_equal(_run(300, 64, 5, rpl=17520), ref)


@pytest.mark.parametrize("well", [300, 1, 401, 581])        # 581: the split column (two wavefronts per member)
def test_one_handle_equals_two_handles_summed(well):
    whole = _run(well, 64, 4)
    halves = _run(well, 32, 4, rpl=7, offset=0) + _run(well, 32, 4, rpl=13, offset=32)
    assert np.array_equal(whole, halves)


def test_two_parameter_points_one_handle_equals_two_handles_summed():
    _, base, _ = digest(200)
    _, other, _ = digest_point("a003")
    pts = [base, other]
    whole = _run(200, 64, 6, points=pts, bases=[0, 1000])
    halves = (_run(200, 32, 6, rpl=5, points=pts, bases=[0, 1000]) +
              _run(200, 32, 6, rpl=11, points=pts, bases=[16, 1016]))
    assert np.array_equal(whole, halves)


@pytest.mark.parametrize("well", [300, 581])
def test_statistics_leave_the_run_alone(well):
    """States, wtd_out, moments and counters with statistics on equal those with statistics off, to the bit."""
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(well)
    ic = golden(f"g1_tables_{well}.npz")["initial_cond"]
    res = []
    for stride in (0, 1):
        st = EnsembleStepper(cols, forcing, 64)
        st.set_state(ic)
        st.set_noise_philox(3, 0)
        if stride:
            st.set_profile_stats(stride)
            st.profile_snapshot(0)
        out = st.step_rows(1, ROWS, want_wtd=True)
        res.append((st.get_state(), out["wtd"], st.moments(), st.counters()))
        st.close()
    (a_psi, a_w, a_m, a_c), (b_psi, b_w, b_m, b_c) = res
    assert np.array_equal(a_psi.view(np.int64), b_psi.view(np.int64))
    assert np.array_equal(a_w, b_w) and np.array_equal(a_m, b_m) and a_c == b_c


def test_resume_from_a_dump_gives_the_uninterrupted_tables(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(300)
    ic = golden("g1_tables_300.npz")["initial_cond"]
    full = EnsembleSimulation(cols, forcing, 64, seed=9, psi0=ic, profile_stride=3)
    full.advance(ROWS)
    want = full.profile_table()
    full.close()
    first = EnsembleSimulation(cols, forcing, 64, seed=9, psi0=ic, profile_stride=3)
    first.advance(50)
    path = first.dump(tmp_path / "ckpt.h5")
    first.close()
    resumed = EnsembleSimulation.restore(path, cols, forcing)
    resumed.advance(ROWS - 50)
    got = resumed.profile_table()
    stats = resumed.profile_stats()
    resumed.close()
    assert resumed.profile_stride == 3 and np.array_equal(got, want)
    assert stats["theta_vol_mean"].shape == ((forcing.dim_t - 1) // 3 + 1, cols.dim_d)


def test_cli_profiles_block_writes_the_new_datasets_and_leaves_the_rest_alone(tmp_path, monkeypatch):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    from hydromodel_amd.synthetic import default_parameters, write_forcing_csv, write_site_information
    params = default_parameters()
    params["Site_Information"] = str(write_site_information(tmp_path / "site.json", {10: WELLS[200]}))
    params["Data_Filename"] = str(write_forcing_csv(tmp_path / "forcing.csv", 1))
    monkeypatch.chdir(tmp_path)
    files = {}
    for tag, extra in (("plain", {}), ("prof", {"Profiles": 48})):
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 128, "Seed": 3, "Days": 2, **extra}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = loadResults(tmp_path / f"Run_{tag}_ensemble.h5")
    plain, prof = files["plain"], files["prof"]
    T, D = len(plain["moments"][0]), plain["initial_cond"].shape[-1]
    n_prow = (T - 1) // 48 + 1
    for key in ("theta_vol", "psi_press", "S_eff"):
        assert prof[key + "_mean"].shape == (n_prow, D) and prof[key + "_std"].shape == (n_prow, D)
    for key in ("transpiration_mean", "transpiration_std", "lateral_flow_mean", "lateral_flow_std", "abs_error_mean"):
        assert prof[key].shape == (T,)
    assert prof["profile_rows"].tolist() == list(range(0, T, 48)) and int(prof["profile_overflow"]) == 0
    assert prof["profile_count"][0] == 128 and np.all(np.isfinite(prof["theta_vol_mean"][:3]))
    assert np.isnan(prof["theta_vol_mean"][3]).all()          # day 3 is past the run: nobody counted
    new_keys = {k for k in prof} - {k for k in plain}
    assert new_keys == {"theta_vol_mean", "theta_vol_std", "psi_press_mean", "psi_press_std", "S_eff_mean", "S_eff_std",
                        "transpiration_mean", "transpiration_std", "lateral_flow_mean", "lateral_flow_std",
                        "abs_error_mean", "profile_rows", "profile_count", "profile_overflow"}
    for k in plain:                                          # (rows past the run are NaN in both)
        a, b = np.asarray(plain[k]), np.asarray(prof[k])
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), k


PROFILE_KEYS = ("theta_vol_mean", "theta_vol_std", "psi_press_mean", "psi_press_std", "S_eff_mean", "S_eff_std",
                "transpiration_mean", "transpiration_std", "lateral_flow_mean", "lateral_flow_std", "abs_error_mean")


@pytest.mark.parametrize("n_points", [1, 2])
def test_cli_sweep_profiles_keep_the_point_axis_and_leave_the_rest_alone(tmp_path, monkeypatch, n_points):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    params = cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    pts = [{"Soil_Properties": {"n": n}} for n in (1.6, 2.4)][:n_points]
    files = {}
    for tag, extra in (("plain", {}), ("prof", {"Profiles": 24, "Distribution": {"Stride": 48}})):
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 128, "Seed": 3, "Days": 2, "Points": pts, **extra}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = loadResults(tmp_path / f"Run_{tag}_ensemble.h5")
    plain, prof = files["plain"], files["prof"]
    P, T, D = n_points, plain["moments"].shape[-1], plain["initial_cond"].shape[-1]
    n_prow = (T - 1) // 24 + 1
    for key in ("theta_vol", "psi_press", "S_eff"):
        assert prof[key + "_mean"].shape == (P, n_prow, D) and prof[key + "_std"].shape == (P, n_prow, D)
    for key in ("transpiration_mean", "transpiration_std", "lateral_flow_mean", "lateral_flow_std", "abs_error_mean"):
        assert prof[key].shape == (P, T)
    assert prof["profile_rows"].tolist() == list(range(0, T, 24)) and int(prof["profile_overflow"]) == 0
    assert prof["profile_count"].shape == (P, n_prow)
    assert (prof["profile_count"][:, :5] == 128).all() and (prof["profile_count"][:, 5:] == 0).all()   # rows 0 ... 96
    assert np.all(np.isfinite(prof["theta_vol_mean"][:, :5])) and np.isnan(prof["theta_vol_mean"][:, 5:]).all()
    assert prof["wtd_hist"].shape == (P, (T - 1) // 48 + 1, D)
    for k in plain:                                          # every pre-existing dataset, byte for byte
        a, b = np.asarray(plain[k]), np.asarray(prof[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


@pytest.mark.parametrize("sweep", [False, True])
def test_two_ranks_sharing_the_card_write_the_profiles_one_rank_writes(tmp_path, sweep):
    params = cli_params(tmp_path)
    ens = {"Members": 250, "Seed": 5, "Days": 2, "Profiles": 24, "Distribution": {"Stride": 12}}
    if sweep:                                                # three points dealt to two ranks: 2 + 1
        ens.update(Members=32, Points=[{"Soil_Properties": {"n": n}} for n in (1.6, 2.0, 2.4)])
    params["Ensemble"] = ens
    one, log1 = run_cli_ranks(tmp_path, "one", params, 1)
    two, log2 = run_cli_ranks(tmp_path, "two", params, 2)
    assert set(PROFILE_KEYS) <= set(one) and set(one) == set(two)
    assert int(one["gpus"]) == 1 and int(two["gpus"]) == 2
    for k in one:
        if k == "gpus":
            continue
        a, b = np.asarray(one[k]), np.asarray(two[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    line = [s for s in log1.splitlines() if "CRPS" in s]
    assert len(line) == 1 and line == [s for s in log2.splitlines() if "CRPS" in s]
