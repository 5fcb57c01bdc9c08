"""Soil-moisture sensors in the particle filter on the GPU (include/hydrocol.h hc_set_filter_soil_moisture): theta against
hc_model_nodes, l_m against its NumPy restatement bit for bit, q_m against NumPy, the ancestry as an integer function of the
exported q_m, the gather; degenerate records against the well-only run; the increment, the ESS and the sensors' diagnostics
in the documented summation order; concentrated weights; invariance under launch length, point order and the dealing of a
sweep's points to handles; resume; the CLI's "Filter": {"Soil_Moisture": ...} block; the refusals."""
import json
import re
from fractions import Fraction

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the refusals below set a shard, whose buffer is torch's)

from helpers import WELLS, digest, forcing_frame, golden
from helpers import cli_params as _cli_params, run_cli_ranks as _run_ranks

pytestmark = pytest.mark.gpu
Q_ONE = 1 << 31
NODES = [6, 45]                 # 30 cm (above every well's water table: unsaturated) and 225 cm
VALUES = [0.24, 0.36]
SIGMAS = np.array([0.05, 0.08])


def _spread(psi0, N, seed=12, width=60.0):
    """[N][D]: the initial profile shifted by a per-member offset, uniform over +-width cm -- members whose water tables
    start in different bins, so that the weights differ and resampling has something to choose (the well's members
    otherwise share one bin for weeks)."""
    return np.asarray(psi0)[None, :] + np.random.default_rng(seed).uniform(-width, width, size=N)[:, None]


def _point_like(n, well=1):
    """a well with the soil's n changed: a parameter point of a sweep, or a column off the special exponents"""
    from hydromodel_amd.digest import ColumnTables, ForcingDigest
    from hydromodel_amd.synthetic import default_parameters
    params = default_parameters()
    params["Soil_Properties"]["n"] = n
    cols = ColumnTables(params, WELLS[well])
    return params, cols, ForcingDigest(params, forcing_frame(1), cols)


def _stepper(well, N, P=1, noise="philox", seed=7, spread=True, soil_n=None):
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(well) if soil_n is None else _point_like(soil_n, well)
    st = EnsembleStepper([cols] * P if P > 1 else cols, forcing, N)
    psi0 = golden(f"g1_tables_{well}.npz")["initial_cond"]
    st.set_state(_spread(psi0, N) if spread else psi0)
    if noise == "numpy":
        st.set_noise_host(np.random.default_rng(seed).standard_normal((N, cols.dim_d)))
    else:
        st.set_noise_philox(seed, 0)
    return st, cols, forcing


def _fresh(st, row_begin, n_rows, seed):
    return np.random.default_rng(seed).standard_normal((st.n_refresh(row_begin, n_rows), st.N, st.D))


def _record(T, row_values, rows=(48,)):
    """[T][n] NaN but on ``rows``, where sensor i reads row_values[i] (NaN: absent)."""
    v = np.full((T, len(row_values)), np.nan)
    for r in rows:
        v[r] = row_values
    return v


def _theta_at(st, psi, nodes):
    """hc_model_nodes' theta of the states ``psi`` [N][D] at ``nodes`` (the handle's state is replaced)."""
    st.set_state(psi)
    return st.model_nodes()["theta"][:, nodes]


def _q_numpy(ell, w, D):
    counted = (w < D) & np.isfinite(ell)
    s = ell[counted].max()
    e = np.where(counted, np.exp(np.where(counted, ell - s, 0.0)), 0.0)
    return np.floor(2.0 ** 31 * e).astype(np.int64), e, s, counted


def _row_48(well, P, mpp, noise, sigmas=SIGMAS, soil_n=None, values=VALUES):
    """One handle stepped to the assimilation at row 48 with two sensors: everything the checks below read."""
    N = P * mpp
    st, cols, forcing = _stepper(well, N, P, noise, soil_n=soil_n)
    sigma = 1.5 * cols.dz
    assert int(forcing.wtd_obs[48]) >= 0 and forcing.refresh[48]
    try:
        st.set_filter(48, sigma, 11)
        st.set_filter_soil_moisture(NODES, _record(st.T, values), sigmas)
        kw = {"fresh_noise": _fresh(st, 1, 47, 1)} if noise == "numpy" else {}
        st.step_rows(1, 47, **kw)
        base_pre = st.get_noise_base() if noise == "numpy" else st.filter_base()
        kw = {"fresh_noise": _fresh(st, 48, 1, 2)} if noise == "numpy" else {}
        out = st.step_rows(48, 1, want_wtd=True, want_psi=True, **kw)
        got = dict(anc=st.filter_ancestors(), qm=st.filter_member_weights(), r=st.filter_draw(), ell=st.filter_loglik(),
                   theta=st.filter_sm_theta(), width=st.filter_sm_width(), q_bins=st.filter_weights(),
                   table=st.filter_table(), smt=st.filter_sm_table(), psi_post=st.get_state(),
                   base_post=st.get_noise_base() if noise == "numpy" else st.filter_base(), base_pre=base_pre,
                   w=out["wtd"][0].astype(np.int64), forecast=out["psi"][0], sigma=sigma, cols=cols,
                   obs=int(forcing.wtd_obs[48]))
        got["theta_model"] = _theta_at(st, out["psi"][0], NODES)
    finally:
        st.close()
    return got


def _check_row_48(g, P, mpp):
    from hydromodel_amd.stepper import filter_ancestors_of, filter_member_loglik
    cols, N = g["cols"], P * mpp
    D, dz = cols.dim_d, cols.dz
    assert g["width"] == 2 and g["theta"].shape == (N, 2) and g["ell"].shape == (N,) and g["qm"].shape == (N,)
    assert g["theta"].tobytes() == g["theta_model"].tobytes()                # the operator: hc_model_nodes' bits
    ell = filter_member_loglik(g["w"], g["theta"], g["obs"], VALUES, dz, g["sigma"], SIGMAS)
    assert g["ell"].tobytes() == ell.tobytes()                               # the same IEEE operations in the same order
    assert not g["q_bins"].any()                                             # the bin table is zeroed on a sensor row
    two_in_a_bin = False
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        w, qm = g["w"][sl], g["qm"][sl]
        q_np, _, s, counted = _q_numpy(g["ell"][sl], w, D)
        assert counted.all()
        assert np.all(np.abs(qm - q_np) <= 1)                                # the device's exp against NumPy's
        assert np.all(qm[g["ell"][sl] == s] == Q_ONE)
        for b in np.unique(w):
            two_in_a_bin |= np.unique(qm[(w == b) & (qm > 0)]).size >= 2     # what one q per bin cannot give
        Q = int(qm.astype(object).sum())
        assert 0 <= int(g["r"][p]) < Q
        assert np.array_equal(g["anc"][sl], filter_ancestors_of(qm, int(g["r"][p])) + p * mpp)
        t = g["table"][p]
        assert t[1, 0] == mpp and t[1, 3] == np.unique(g["anc"][sl]).size
        assert np.isnan(t[2:, 1:]).all() and np.all(t[2:, 0] == 0)
        smt = g["smt"][p]
        assert smt[1, :, 0].tolist() == [1.0, 1.0] and smt[1, :, 1].tolist() == VALUES
        assert np.isfinite(smt[1]).all() and np.isnan(smt[0]).all() and np.isnan(smt[2:]).all()
    assert two_in_a_bin
    assert not np.array_equal(g["anc"], np.arange(N))
    assert np.array_equal(g["psi_post"], g["forecast"][g["anc"]])            # each slot's ancestor, bit for bit
    assert np.array_equal(g["base_post"], g["base_pre"][g["anc"]])


# ---- 4. weights, ancestry and gather -----------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["philox", "numpy"])
@pytest.mark.parametrize("well, P, mpp", [
    (1, 1, 100), (1, 3, 100), (300, 1, 100), (300, 3, 100), (581, 1, 100), (581, 3, 100),   # D = 101, 300, 581 (split)
    (1, 1, 2500),                                           # three tiles of the prefix scan
])
def test_member_weights_ancestry_and_gather_at_a_sensor_row(well, P, mpp, noise):
    """Members per point are not a multiple of 64; the states start spread, so theta at 30 cm differs within a bin."""
    _check_row_48(_row_48(well, P, mpp, noise), P, mpp)


# ---- 5. generic exponents ----------------------------------------------------------------------------------------------
def test_member_weights_with_generic_exponents():
    """n = 1.7: the cell model of enkf_theta without the special exponents."""
    _check_row_48(_row_48(300, 1, 100, "philox", soil_n=1.7), 1, 100)


# ---- 6. degenerate records ---------------------------------------------------------------------------------------------
def _run_256(values=None, sigmas=SIGMAS, rows=96, N=256, record_rows=(48, 96)):
    st, cols, forcing = _stepper(300, N)
    try:
        st.set_filter(48, 1.5 * cols.dz, 3)
        if values is not None:
            st.set_filter_soil_moisture(NODES, _record(st.T, values, record_rows), sigmas)
        st.step_rows(1, rows - 1)
        out = st.step_rows(rows, 1, want_wtd=True, want_psi=True)
        got = dict(psi=st.get_state(), table=st.filter_table(), anc=st.filter_ancestors(), q_bins=st.filter_weights(),
                   base=st.filter_base(), w=out["wtd"][0].astype(np.int64), forecast=out["psi"][0], cols=cols,
                   obs=int(forcing.wtd_obs[rows]), r=int(st.filter_draw()[0]))
        if values is not None:
            got.update(qm=st.filter_member_weights(), width=st.filter_sm_width(), smt=st.filter_sm_table()[0])
            if got["width"]:
                got.update(ell=st.filter_loglik(), theta=st.filter_sm_theta())
    finally:
        st.close()
    return got


@pytest.fixture(scope="module")
def well_only():
    return _run_256()


def test_an_all_nan_record_is_the_well_only_run(well_only):
    got = _run_256([np.nan, np.nan])
    for k in ("psi", "table", "anc", "q_bins", "base"):
        assert got[k].dtype == well_only[k].dtype and got[k].tobytes() == well_only[k].tobytes(), k
    assert got["width"] == 0 and np.isnan(got["smt"]).all()
    assert np.array_equal(got["qm"], well_only["q_bins"][0][got["w"]])       # the bin path's q of each member's bin


def test_sensors_of_huge_error_give_the_well_only_weights(well_only):
    got = _run_256(VALUES, np.array([1e200, 1e200]))
    assert got["width"] == 2 and not got["q_bins"].any()
    assert np.array_equal(got["w"], well_only["w"])
    assert np.array_equal(got["qm"], well_only["q_bins"][0][well_only["w"]])
    for k in ("psi", "anc", "base"):
        assert got[k].tobytes() == well_only[k].tobytes(), k
    a, b = got["table"][0], well_only["table"][0]
    assert np.array_equal(a[:, [0, 1, 3]], b[:, [0, 1, 3]], equal_nan=True)   # count, ESS, survivors
    shift = -2.0 * np.log(1e200) - 0.5 * 2 * np.log(2.0 * np.pi)
    for slot in (1, 2):
        assert abs((a[slot, 2] - b[slot, 2]) - shift) <= 1e-12 * abs(shift)
    assert got["smt"][1:3, :, 0].tolist() == [[1.0, 1.0]] * 2


def test_one_of_two_sensors_absent_on_the_row():
    from hydromodel_amd.stepper import filter_member_loglik
    got = _run_256([VALUES[0], np.nan], rows=48, record_rows=(48,))
    assert got["width"] == 1 and got["theta"].shape == (256, 1)
    s = got["smt"][1]
    assert s[:, 0].tolist() == [1.0, 0.0] and s[0, 1] == VALUES[0] and np.isnan(s[1, 1:]).all() and np.isfinite(s[0]).all()
    ell = filter_member_loglik(got["w"], got["theta"], got["obs"], VALUES[:1], got["cols"].dz, 1.5 * got["cols"].dz,
                               SIGMAS[:1])
    assert got["ell"].tobytes() == ell.tobytes()


# ---- 7. increment, ESS and diagnostics ---------------------------------------------------------------------------------
def test_increment_ess_and_sensor_diagnostics_against_numpy():
    from hydromodel_amd.stepper import filter_tile_sum
    N = 256
    got = _run_256(VALUES, rows=48, record_rows=(48,))
    cols, t, smt = got["cols"], got["table"][0, 1], got["smt"][1]
    q_np, e, s, counted = _q_numpy(got["ell"], got["w"], cols.dim_d)
    n = int(counted.sum())
    W = filter_tile_sum(e)                                                     # the documented order
    inc = s + np.log(W / n) - np.log(1.5 * cols.dz)
    for sg in SIGMAS:
        inc -= np.log(sg)
    inc -= 0.5 * 3.0 * np.log(2.0 * np.pi)
    bound = (N + 16) * 2.0 ** -53              # N_p positive terms, plus the ulps of exp and log
    print(f"\n increment {t[2]!r} against {inc!r}: {abs(t[2] - inc):.3e} (bound {bound * max(1.0, abs(inc)):.3e})")
    assert t[0] == n == N and abs(t[2] - inc) <= bound * max(1.0, abs(inc))
    qm = [int(v) for v in got["qm"]]
    ess = Fraction(sum(qm) ** 2, sum(v * v for v in qm))
    assert abs(t[1] - float(ess)) <= 4.5e-16 * float(ess)                      # within 2 ulp
    theta, post = got["theta"], got["theta"][got["anc"]]
    for i in range(2):
        for col, x in ((2, theta[:, i]), (4, post[:, i])):
            mean = filter_tile_sum(x) / N
            std = np.sqrt(filter_tile_sum((x - mean) * (x - mean)) / (N - 1))
            exact_mean = float(np.mean(x.astype(np.longdouble)))
            exact_std = float(np.sqrt(np.sum((x.astype(np.longdouble) - exact_mean) ** 2) / (N - 1)))
            assert smt[i, col] == mean and abs(mean - exact_mean) <= bound * max(1.0, abs(exact_mean))
            assert abs(smt[i, col + 1] - std) <= bound and abs(smt[i, col + 1] - exact_std) <= bound * max(1.0, exact_std)
    assert t[3] == np.unique(got["anc"]).size


def test_one_member_increment_is_the_joint_gaussian_log_density():
    got = _run_256(VALUES, rows=48, record_rows=(48,), N=1)
    cols, t, smt = got["cols"], got["table"][0, 1], got["smt"][1]
    sigma = 1.5 * cols.dz
    want = -0.5 * (cols.dz * (int(got["w"][0]) - got["obs"]) / sigma) ** 2 - np.log(sigma) - 0.5 * np.log(2.0 * np.pi)
    for i in range(2):
        want += -0.5 * ((got["theta"][0, i] - VALUES[i]) / SIGMAS[i]) ** 2 - np.log(SIGMAS[i]) - 0.5 * np.log(2.0 * np.pi)
    assert t[0] == 1 and t[1] == 1.0 and t[3] == 1 and got["anc"].tolist() == [0] and got["qm"].tolist() == [Q_ONE]
    assert abs(t[2] - want) <= 1e-12 * max(1.0, abs(want))
    assert smt[:, 3].tolist() == [0.0, 0.0] and smt[:, 5].tolist() == [0.0, 0.0]
    assert smt[:, 2].tolist() == got["theta"][0].tolist() == smt[:, 4].tolist()


# ---- 8. tiny errors ----------------------------------------------------------------------------------------------------
def test_weight_on_a_few_members_fills_long_slot_ranges():
    """sigma_i = 1e-4 at 30 cm: the members whose theta lies next to the reading share the 2 500 slots of their point."""
    P, mpp = 2, 2500
    g = _row_48(1, P, mpp, "philox", sigmas=np.array([1e-4, 0.08]))
    from hydromodel_amd.stepper import filter_ancestors_of
    longest = 0
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        anc = g["anc"][sl] - p * mpp
        assert np.array_equal(anc, filter_ancestors_of(g["qm"][sl], int(g["r"][p])))
        assert anc.min() >= 0 and anc.max() < mpp and np.all(np.diff(anc) >= 0)    # the slots partition [0, N_p)
        assert g["table"][p, 1, 3] == np.unique(anc).size
        longest = max(longest, int(np.bincount(anc, minlength=mpp).max()))
    assert longest > 64
    assert np.array_equal(g["psi_post"], g["forecast"][g["anc"]]) and np.array_equal(g["base_post"], g["base_pre"][g["anc"]])


# ---- 9. independence ---------------------------------------------------------------------------------------------------
SWEEP_N = (1.6, 1.7, 1.8, 2.0, 2.1, 2.2, 2.3, 2.4)
SWEEP_MPP, SWEEP_ROWS, SWEEP_STRIDE = 70, 120, 24


def _sweep_handle(ids, psi_all, rows_per_launch=0):
    """The handle that runs the sweep points ``ids``: global member ids point-major, each point keyed by its first global
    member, states from the whole sweep's ``psi_all``; five assimilations with two sensors."""
    from hydromodel_amd.stepper import EnsembleStepper
    pts = [_point_like(SWEEP_N[k]) for k in ids]
    st = EnsembleStepper([c for _, c, _ in pts], pts[0][2], len(ids) * SWEEP_MPP)
    try:
        st.set_generic_exponents(True)
        st.set_state(np.concatenate([psi_all[k * SWEEP_MPP:(k + 1) * SWEEP_MPP] for k in ids]))
        st.set_noise_philox(21, ids[0] * SWEEP_MPP)
        if len(ids) > 1:
            st.set_point_member_bases(np.array(ids, dtype=np.int64) * SWEEP_MPP)
        st.set_rows_per_launch(rows_per_launch)
        st.set_filter(SWEEP_STRIDE, 2.0 * st.cols.dz, 8)
        st.set_filter_soil_moisture(NODES, _record(st.T, VALUES, range(SWEEP_STRIDE, SWEEP_ROWS + 1, SWEEP_STRIDE)), SIGMAS)
        st.step_rows(1, SWEEP_ROWS)
        n = len(ids)
        return dict(psi=st.get_state().reshape(n, SWEEP_MPP, -1), table=st.filter_table(), smt=st.filter_sm_table(),
                    moments=np.asarray(st.moments()).reshape(n, 3, -1), base=st.filter_base().reshape(n, SWEEP_MPP, -1))
    finally:
        st.close()


def test_results_do_not_depend_on_launch_length_point_order_or_the_dealing_of_points(monkeypatch):
    psi_all = _spread(golden("g1_tables_1.npz")["initial_cond"], 8 * SWEEP_MPP, seed=4)
    everyone = list(range(8))
    monkeypatch.delenv("HYDROCOL_POINT_ORDER", raising=False)
    whole = _sweep_handle(everyone, psi_all)
    assert (whole["table"][:, 1:6, 0] == SWEEP_MPP).all() and np.isfinite(whole["smt"][:, 1:6]).all()
    assert np.any(whole["table"][:, 1:6, 3] < SWEEP_MPP)
    others = [_sweep_handle(everyone, psi_all, 48), _sweep_handle(everyone, psi_all, 480)]
    monkeypatch.setenv("HYDROCOL_POINT_ORDER", "fixed")
    others.append(_sweep_handle(everyone, psi_all))
    monkeypatch.delenv("HYDROCOL_POINT_ORDER", raising=False)
    for other in others:
        for k in whole:
            assert whole[k].dtype == other[k].dtype and whole[k].tobytes() == other[k].tobytes(), k
    for ids in ([0, 2, 4, 6], [1, 3, 5, 7]):                   # what two ranks of the sweep run
        part = _sweep_handle(ids, psi_all)
        for j, k in enumerate(ids):
            for key in whole:
                assert whole[key][k].tobytes() == part[key][j].tobytes(), (ids, k, key)


# ---- 10. checkpoint ----------------------------------------------------------------------------------------------------
def test_dump_and_restore_continue_a_run_with_a_record_bit_for_bit(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    from hydromodel_amd.stepper import soil_moisture_record
    _, cols, forcing = digest(1)
    psi0 = _spread(golden("g1_tables_1.npz")["initial_cond"], 96)
    values = _record(forcing.dim_t, VALUES, range(24, 145, 24))
    values[96, 1] = np.nan
    record = soil_moisture_record(cols.z, cols.z[NODES], values, SIGMAS)
    assert record["nodes"].tolist() == NODES
    kw = dict(seed=6, psi0=psi0, filter_stride=24, filter_sigma_cm=2.0 * cols.dz, filter_soil_moisture=record)

    def state(sim):
        return [sim.stepper.get_state(), sim.filter_table(), sim.filter_sm_table(), sim.moments(), sim.stepper.filter_base()]

    whole = EnsembleSimulation(cols, forcing, 96, **kw)
    try:
        whole.advance(72)
        path = whole.dump(tmp_path / "ck.h5")
        whole.advance(72)
        want, summary = state(whole), whole.filter_summary()
    finally:
        whole.close()
    with pytest.raises(ValueError, match="pass the same record as filter_soil_moisture"):
        EnsembleSimulation.restore(path, cols, forcing)
    back = EnsembleSimulation.restore(path, cols, forcing, filter_soil_moisture=record)
    try:
        assert back.next_row == 73 and back.filter_stride == 24 and back.stepper.filter_sm_n == 2
        back.advance(72)
        got = state(back)
    finally:
        back.close()
    for a, b in zip(want, got):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert summary["rows"].tolist() == summary["sm_rows"].tolist() == [24, 48, 72, 96, 120, 144]
    assert summary["sm_observed"][3].tolist() == [True, False] and np.isfinite(summary["loglik"])


# ---- 11. the CLI -------------------------------------------------------------------------------------------------------
SM_KEYS = {"filter_sm_depths_cm", "filter_sm_nodes", "filter_sm_sigma", "filter_sm_observed", "filter_sm_obs",
           "filter_sm_prior_mean", "filter_sm_prior_std", "filter_sm_post_mean", "filter_sm_post_std"}


def _sensor_csv(tmp_path, n_depths, every=24):
    from hydromodel_amd.synthetic import synthetic_forcing, write_soil_moisture_csv
    _, datenum, _, _ = synthetic_forcing(1)
    v = np.full((datenum.size, n_depths), np.nan)
    rng = np.random.default_rng(3)
    v[::every] = rng.uniform(0.15, 0.3, size=v[::every].shape)
    v[48::96, -1] = np.nan
    return str(write_soil_moisture_csv(tmp_path / "sm.csv", v, datenum))


def test_cli_filter_soil_moisture_block_writes_the_datasets(tmp_path, monkeypatch, capsys):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    params = _cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    sm = {"Filename": _sensor_csv(tmp_path, 2), "Depths_cm": [30, 120], "Sigma": [0.05, 0.06]}
    files, logs = {}, {}
    pts = [{"Soil_Properties": {"n": 1.6}}, {"Soil_Properties": {"n": 2.4}}]
    for tag, extra in (("well", {"Filter": {"Stride": 24, "Sigma_cm": 10.0}}),
                       ("ens", {"Filter": {"Stride": 24, "Sigma_cm": 10.0, "Soil_Moisture": sm}}),
                       ("sweep", {"Points": pts, "Filter": {"Sigma_cm": 10.0, "Soil_Moisture": sm}})):
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 64, "Seed": 3, "Days": 2, **extra}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = loadResults(tmp_path / f"Run_{tag}_ensemble.h5")
        logs[tag] = capsys.readouterr().out
    well, ens, sweep = files["well"], files["ens"], files["sweep"]
    assert "soil-moisture" not in logs["well"] and set(ens) - set(well) == SM_KEYS
    assert ens["filter_rows"].tolist() == [24, 48, 72, 96]
    assert ens["filter_sm_nodes"].tolist() == [6, 24] and ens["filter_sm_depths_cm"].tolist() == [30.0, 120.0]
    assert ens["filter_sm_sigma"].tolist() == [0.05, 0.06]
    assert ens["filter_sm_observed"].tolist() == [[1, 1], [1, 0], [1, 1], [1, 1]]
    for k in SM_KEYS - {"filter_sm_depths_cm", "filter_sm_nodes", "filter_sm_sigma"}:
        assert ens[k].shape == (4, 2), k
    assert np.isnan(ens["filter_sm_prior_mean"][1, 1]) and np.isfinite(ens["filter_sm_post_std"][0]).all()
    assert not np.array_equal(ens["filter_loglik_rows"], well["filter_loglik_rows"])    # the joint increment
    rmse = np.sqrt(np.nanmean((ens["filter_sm_obs"] - ens["filter_sm_prior_mean"]) ** 2))
    line = re.search(r"\[Ensemble x64\] soil-moisture forecast RMSE = ([0-9.]+) over 4 rows", logs["ens"])
    assert line and abs(float(line.group(1)) - rmse) <= 1e-5
    assert sweep["filter_sm_obs"].shape == (2, 2, 2) and sweep["filter_rows"].tolist() == [48, 96]
    assert "[Sweep 2 points x64] soil-moisture forecast RMSE: best point " in logs["sweep"]


def test_a_sensor_filtered_sweep_on_two_ranks_writes_what_one_rank_writes(tmp_path):
    params = _cli_params(tmp_path)
    sm = {"Filename": _sensor_csv(tmp_path, 3), "Depths_cm": [20, 60, 150], "Sigma": 0.05}
    params["Ensemble"] = {"Members": 40, "Seed": 5, "Days": 2,
                          "Points": [{"Soil_Properties": {"n": n}} for n in (1.6, 2.0, 2.2, 2.4)],
                          "Filter": {"Stride": 24, "Sigma_cm": 8.0, "Soil_Moisture": sm}}
    one, log1 = _run_ranks(tmp_path, "one", params, 1)
    two, log2 = _run_ranks(tmp_path, "two", params, 2)
    assert set(one) == set(two) and SM_KEYS <= set(one)
    for k in sorted(set(one) - {"gpus"}):
        a, b = np.asarray(one[k]), np.asarray(two[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert one["filter_sm_obs"].shape == (4, 4, 3)
    line = [s for s in log1.splitlines() if "soil-moisture forecast RMSE" in s]
    assert len(line) == 1 and line == [s for s in log2.splitlines() if "soil-moisture forecast RMSE" in s]


def test_cli_refuses_a_record_with_a_sharded_single_point_filter(tmp_path, monkeypatch, capsys):
    from hydromodel_amd import cli
    params = _cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    sm = {"Filename": _sensor_csv(tmp_path, 2), "Depths_cm": [30, 120], "Sigma": 0.05}
    params["Ensemble"] = {"Members": 64, "Days": 1, "Filter": {"Sigma_cm": 10.0, "Sharded": True, "Soil_Moisture": sm}}
    (tmp_path / "p.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as status:
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "p.json")])
    out = capsys.readouterr().out
    assert status.value.code == 1 and "the sharded filter gathers the members' water-table indices only" in out
    assert not (tmp_path / "Sim_01_ensemble.h5").exists() and "Saving" not in out


# ---- 12. refusals through the stepper ----------------------------------------------------------------------------------
def test_refusals():
    from hydromodel_amd._lib import HcError
    st, cols, _ = _stepper(1, 64)
    rec = _record(st.T, VALUES)
    try:
        with pytest.raises(HcError, match="the particle filter is off"):
            st.set_filter_soil_moisture(NODES, rec, SIGMAS)
        st.set_enkf(48, 5.0, 0.0, 1)
        with pytest.raises(HcError, match="the EnKF is on"):
            st.set_filter_soil_moisture(NODES, rec, SIGMAS)
        st.set_enkf(0)
        st.set_filter(48, 5.0, 1)
        with pytest.raises(HcError, match="9 sensors, at most 8"):
            st.set_filter_soil_moisture(list(range(9)), np.full((st.T, 9), np.nan), 0.02)
        with pytest.raises(HcError, match="sigma 0 of sensor 1 must be finite and > 0"):
            st.set_filter_soil_moisture(NODES, rec, [0.02, 0.0])
        st.set_filter_soil_moisture(NODES, rec, SIGMAS)
        assert st.filter_sm_n == 2 and st.filter_sm_table().shape == (1, (st.T - 1) // 48 + 1, 2, 6)
        with pytest.raises(HcError, match="the sharded filter gathers water-table indices only"):
            st.set_filter_shard([0, 64], 0, None)
        assert st.get_filter_shard() == (0, 0, 0)
        st.set_filter_soil_moisture(None)                       # the record removed: sharding is accepted again,
        st.set_filter_shard([0, 64], 0, None)
        with pytest.raises(HcError, match="the sharded filter gathers water-table indices only"):
            st.set_filter_soil_moisture(NODES, rec, SIGMAS)     # ... and refuses the record in its turn
        assert st.filter_sm_n == 0
        st.set_filter(48, 5.0, 1)                               # hc_set_filter removes sharding and record alike
        st.set_filter_soil_moisture(NODES, rec, SIGMAS)
        st.set_filter(0)
        assert st.filter_sm_n == 0 and st.filter_sm_width() == 0
    finally:
        st.close()
