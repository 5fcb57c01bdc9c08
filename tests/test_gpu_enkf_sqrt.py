"""The EnKF's square-root analysis and relaxation to prior spread on the GPU (include/hydrocol.h hc_set_enkf_method):
the reduced gain, the mean's increment, the spreads, the analysis states and the posterior diagnostics against the float64
NumPy restatement from the forecast states; defaults that change nothing; a square-root analysis that draws nothing;
invariance under launch length, point order and the dealing of a sweep's points to handles and ranks; edge cases; resume;
the CLI's "Method" / "Relaxation" keys; a twin experiment."""
import copy
import json

import numpy as np
import pytest

from helpers import digest, golden
from helpers import cli_params as _cli_params, run_cli_ranks as _run_ranks
from test_enkf_sm_cpu import analysis_restated
from test_enkf_sqrt_cpu import rtps_restated, sqrt_analysis_restated
from test_gpu_enkf import _find_wtd, _fresh, _spread, _stepper, _y_of, digest_point_like
from test_gpu_enkf_sm import _record, _sensor_csv, _theta_at

pytestmark = pytest.mark.gpu

VARIANTS = [("sqrt", 0.0), ("sqrt", 0.5), ("stochastic", 0.5)]


@pytest.mark.parametrize("method, alpha", VARIANTS)
@pytest.mark.parametrize("noise", ["philox", "numpy"])
@pytest.mark.parametrize("well, P, mpp, loc, n_s", [
    (1, 1, 100, 0.0, 1), (1, 3, 100, 60.0, 3), (300, 1, 100, 0.0, 3), (300, 2, 100, 50.0, 1),
    (1, 1, 2500, 0.0, 3), (1, 2, 2500, 80.0, 1),              # the grid of test_gpu_enkf_sm.test_analysis_against_numpy
    (1, 2, 100, 0.0, 0), (300, 1, 2500, 50.0, 0),             # ... and the well alone
])
def test_analysis_against_numpy(well, P, mpp, loc, n_s, noise, method, alpha):
    _check_analysis(well, P, mpp, loc, n_s, noise, method, alpha)


def _check_analysis(well, P, mpp, loc, n_s, noise, method, alpha, find_wtd=_find_wtd, y_of=_y_of,
                    sqrt_analysis=sqrt_analysis_restated, analysis=analysis_restated, rtps=rtps_restated,
                    mean_std=lambda x: (x.mean(), x.std(ddof=1)), std_columns=lambda x: x.std(axis=0, ddof=1)):
    """The restatements are arguments: a large ensemble passes forms without a loop over the members and with long sums."""
    N = P * mpp
    st, cols, forcing = _stepper(well, N, P, noise)
    D, dz, sigma, seed = cols.dim_d, cols.dz, 5.0, 11
    nodes = {0: [], 1: [12], 3: [6, 20, 33, 45]}[n_s]                 # 3 sensors present of 4
    vals = {0: [], 1: [0.21], 3: [0.27, np.nan, 0.18, 0.24]}[n_s]
    s_sig = np.array([0.02, 0.03, 0.015, 0.025][:len(nodes)])
    present = np.array([i for i, v in enumerate(vals) if not np.isnan(v)], dtype=np.int64)
    at = np.array(nodes, dtype=np.int64)[present]                     # the nodes of the sensors present
    obs = int(forcing.wtd_obs[48])
    psat = float(cols.soil.psi_sat)
    try:
        st.set_enkf(48, sigma, loc, seed)
        if nodes:
            st.set_enkf_soil_moisture(nodes, _record(st.T, nodes, vals), s_sig)
        st.set_enkf_method(method, alpha)
        assert st.get_enkf_method() == (method, alpha)
        kw = {"fresh_noise": _fresh(st, 1, 47, 1)} if noise == "numpy" else {}
        st.step_rows(1, 47, **kw)
        kw = {"fresh_noise": _fresh(st, 48, 1, 2)} if noise == "numpy" else {}
        out = st.step_rows(48, 1, want_wtd=True, want_psi=True, **kw)
        Y = st.enkf_sm_y() if nodes else st.enkf_y()[:, None]
        K = st.enkf_sm_gain() if nodes else st.enkf_gain()[:, :, None]
        if method == "sqrt":
            Kr, dbar = st.enkf_sqrt_gain(), st.enkf_sqrt_shift()
        else:
            eps_w = st.enkf_eps()
            eps_s = st.enkf_sm_eps() if nodes else np.zeros((N, 0))
        if alpha:
            sb, sa, f = st.enkf_relaxation_factors()
        post = st.get_state()
        table = st.enkf_table()
        smt = st.enkf_sm_table() if nodes else None
        theta_post = _theta_at(st, post)[:, at]
    finally:
        st.close()
    W = 1 + len(present)
    forecast = out["psi"][0]
    assert Y.shape == (N, W) and K.shape == (P, D, W)
    o = np.concatenate([[obs * dz], np.asarray(vals, dtype=np.float64)[present]])
    R = np.concatenate([[sigma], s_sig[present]]) ** 2
    zeta_nodes = at * dz

    def close(got, want, tag):                                        # LAB_NOTES.md 13: 1e-10 of the array's largest entry
        err = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
        print(f" {tag}: {err:.1e}", end="")
        assert got.shape == want.shape and err <= 1e-10, (tag, err)

    if method == "sqrt":
        res = sqrt_analysis(forecast, Y, o, R, zeta_nodes, dz, loc, mpp)
        close(K, res["K"], "K")
        close(Kr, res["Kr"], "Kr")
        close(dbar, res["dbar"], "dbar")
        assert np.abs(Kr).max() > 0.0
        if W == 1:                                                    # Kr = K / (1 + sqrt(sigma^2 / s))
            assert np.all(np.abs(Kr) <= np.abs(K))
    else:
        E = np.concatenate([eps_w[:, None], eps_s[:, present]], axis=1)
        res = analysis(forecast, Y, E, o, R, zeta_nodes, dz, loc, mpp)
        close(K, res["K"], "K")
    want = res["post"]
    if alpha:
        sb_np, sa_np, f_np, want = rtps(forecast, res["post"], alpha, mpp)
        close(sb, sb_np, "sigma_b")
        close(sa, sa_np, "sigma_a")
        assert np.all(np.abs(f - f_np) <= 1e-9 * np.abs(f_np)) and np.isfinite(f).all()
        # what the relaxation is for: every node's spread is (1 - alpha) sigma_a + alpha sigma_b
        for p in range(P):
            sl = slice(p * mpp, (p + 1) * mpp)
            blend = (1.0 - alpha) * sa[p] + alpha * sb[p]
            assert np.abs(std_columns(post[sl]) - blend).max() <= 1e-9 * sb[p].max()
    err = float(np.max(np.abs(post - want) / (1.0 + np.abs(want))))
    print(f" states: {err:.1e}")
    assert err <= 1e-9
    assert not np.array_equal(post, forecast)
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        t = table[p, 1]
        assert t[0] == mpp and t[7] == 0
        assert abs(t[1] - res["ybar"][p, 0]) <= 1e-12 * abs(res["ybar"][p, 0])
        y_post = y_of(post[sl], find_wtd(post[sl], psat), psat, dz)          # the posterior describes the FINAL states
        yb_post, sd_post = mean_std(y_post)
        assert abs(t[5] - yb_post) <= 1e-9 * (1.0 + abs(yb_post))
        assert abs(t[6] - sd_post) <= 1e-9 * (1.0 + sd_post)
        for k, i in enumerate(present):
            tp = theta_post[sl, k]
            s = smt[p, 1, i]
            tp_mean, tp_sd = mean_std(tp)
            assert s[0] == 1.0 and abs(s[4] - tp_mean) <= 1e-12 and abs(s[5] - tp_sd) <= 1e-10


def _run(well, N, rows, scheme=None, seed=3, sensors=True, P=1):
    st, cols, _ = _stepper(well, N, P, seed=5)
    try:
        st.set_wtd_hist(48)
        st.set_enkf(48, 2.0 * cols.dz, 40.0, seed)
        nodes = [6, 20, 45]
        if sensors:
            st.set_enkf_soil_moisture(nodes, _record(st.T, nodes, [0.22, 0.26, 0.2], rows=(48, 144)), 0.02)
        if scheme is not None:
            st.set_enkf_method(*scheme)
        st.step_rows(1, rows)
        got = dict(psi=st.get_state(), moments=np.asarray(st.moments()), hist=st.wtd_hist_table(), table=st.enkf_table(),
                   gain=st.enkf_gain(), y=st.enkf_y())
        if sensors:
            got["sm"] = st.enkf_sm_table()
        if scheme is None or scheme[0] == "stochastic":
            got["eps"] = st.enkf_eps()
        return got
    finally:
        st.close()


def _same(a, b, keys=None):
    for k in keys or a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


def test_the_default_scheme_is_the_run_without_the_call():
    ref = _run(300, 96, 150)
    got = _run(300, 96, 150, scheme=("stochastic", 0.0))
    assert set(ref) == set(got) and "eps" in got
    _same(ref, got)


def test_the_square_root_analysis_does_not_depend_on_the_enkf_seed():
    for scheme in (("sqrt", 0.0), ("sqrt", 0.5)):
        a, b = _run(1, 96, 150, scheme, seed=3), _run(1, 96, 150, scheme, seed=77)
        _same(a, b)
    a, b = _run(1, 96, 150, ("stochastic", 0.5), seed=3), _run(1, 96, 150, ("stochastic", 0.5), seed=77)
    assert not np.array_equal(a["psi"], b["psi"])                     # (the perturbed observations do)


NS, MPP, SEED = (1.6, 2.0, 2.4), 70, 31


def _point_handle(ids, rows_per_launch=0):
    """test_gpu_enkf_sm._point_handle with three sensors, the square-root scheme and alpha = 0.5"""
    from hydromodel_amd.stepper import EnsembleStepper
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
        v = _record(st.T, [8, 30, 50], [0.22, 0.26, 0.3], rows=(24, 72, 120))
        v[48] = [0.2, np.nan, np.nan]                           # one sensor; 96, 144: the well alone (m' = 1)
        st.set_enkf_soil_moisture([8, 30, 50], v, [0.02, 0.03, 0.02])
        st.set_enkf_method("sqrt", 0.5)
        st.step_rows(1, 150)
        n = len(ids)
        sb, sa, f = st.enkf_relaxation_factors()
        return dict(psi=st.get_state().reshape(n, MPP, -1), table=st.enkf_table(), sm=st.enkf_sm_table(),
                    moments=np.asarray(st.moments()).reshape(n, 3, -1), hist=st.wtd_hist_table().reshape(n, -1),
                    kr=st.enkf_sqrt_gain(), dbar=st.enkf_sqrt_shift(), sb=sb, sa=sa, f=f)
    finally:
        st.close()


def test_results_do_not_depend_on_launch_length_point_order_or_handles():
    whole = _point_handle([0, 1, 2])
    assert (whole["table"][:, 1:7, 0] == MPP).all() and (whole["sm"][:, [1, 3, 5], :, 0] == 1.0).all()
    assert (whole["f"] >= 1.0).any() and np.isfinite(whole["psi"]).all()
    runs = {"rows 1": (_point_handle([0, 1, 2], 1), [0, 1, 2]), "rows 7": (_point_handle([0, 1, 2], 7), [0, 1, 2]),
            "reversed": (_point_handle([2, 1, 0]), [2, 1, 0]), "split a": (_point_handle([0, 2]), [0, 2]),
            "split b": (_point_handle([1]), [1])}
    for tag, (part, ids) in runs.items():
        for j, k in enumerate(ids):
            for key in whole:
                a, b = whole[key][k], part[key][j]
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (tag, k, key)


METHOD_KEYS = {"enkf_method", "enkf_relaxation"}


def test_a_square_root_sweep_on_two_ranks_writes_what_one_rank_writes(tmp_path):
    params = _cli_params(tmp_path)
    sm = {"Filename": _sensor_csv(tmp_path, 3), "Depths_cm": [20, 60, 150], "Sigma": 0.02}
    params["Ensemble"] = {"Members": 40, "Seed": 5, "Days": 2, "Distribution": {"Stride": 48},
                          "Points": [{"Soil_Properties": {"n": n}} for n in (1.6, 2.0, 2.2, 2.4)],
                          "EnKF": {"Stride": 24, "Sigma_cm": 8.0, "Soil_Moisture": sm, "Method": "sqrt", "Relaxation": 0.5}}
    one, _ = _run_ranks(tmp_path, "one", params, 1)
    two, _ = _run_ranks(tmp_path, "two", params, 2)
    for k in sorted(k for k in one if k.startswith("enkf_")) + ["moments", "wtd_hist"]:
        a, b = np.asarray(one[k]), np.asarray(two[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert int(one["enkf_method"]) == 1 and float(one["enkf_relaxation"]) == 0.5 and one["enkf_sm_obs"].shape == (4, 4, 3)


def test_one_member_per_point_keeps_its_state():
    st, cols, _ = _stepper(1, 2, 2)
    try:
        st.set_enkf(48, 7.0, 0.0, 1)
        st.set_enkf_soil_moisture([12], _record(st.T, [12], [0.2]), 0.02)
        st.set_enkf_method("sqrt", 0.5)
        st.step_rows(1, 47)
        out = st.step_rows(48, 1, want_psi=True)
        sb, sa, f = st.enkf_relaxation_factors()
        assert np.array_equal(st.get_state(), out["psi"][0])
        assert not st.enkf_sqrt_gain().any() and not st.enkf_sqrt_shift().any()
        assert not sb.any() and not sa.any() and (f == 1.0).all()
        t = st.enkf_table()
        assert (t[:, 1, 0] == 1).all() and (t[:, 1, 7] == 0).all() and np.isfinite(t[:, 1]).all()
    finally:
        st.close()


@pytest.mark.parametrize("method", ["sqrt", "stochastic"])
def test_nodes_where_every_member_agrees_are_untouched(method):
    """sigma_a = 0: the 64 members of the second point start from one state and take the same noise (caller noise), so
    they hold the same psi on every node of the analysis row, as a saturated tail does; the first point is spread."""
    mpp, N = 64, 128
    st, cols, _ = _stepper(1, N, 2, "numpy")
    D = cols.dim_d
    try:
        psi = st.get_state()
        psi[mpp:] = psi[mpp]
        st.set_state(psi)
        base = np.random.default_rng(8).standard_normal((N, D))
        base[mpp:] = base[mpp]
        st.set_noise_host(base)
        st.set_enkf(48, 5.0, 0.0, 1)
        st.set_enkf_method(method, 0.5)
        fresh = _fresh(st, 1, 48, 3)
        fresh[:, mpp:] = fresh[:, mpp:mpp + 1]
        out = st.step_rows(1, 48, want_psi=True, fresh_noise=fresh)
        forecast, post = out["psi"][-1], st.get_state()
        sb, sa, f = st.enkf_relaxation_factors()
        t = st.enkf_table()
    finally:
        st.close()
    assert (forecast[mpp:] == forecast[mpp]).all()                    # every member agrees, on every node
    assert not sa[1].any() and (f[1] == 1.0).all()                   # sigma_a = 0 exactly (sigma_b: the rounding of a
    assert sb[1].max() <= 1e-12 * np.abs(forecast[mpp]).max()         # plain sum of 64 equal values)
    assert np.array_equal(post[mpp:], forecast[mpp:]) and np.isfinite(post).all()
    assert sb[0].min() > 0.0 and not np.array_equal(post[:mpp], forecast[:mpp])
    assert (t[:, 1, 0] == mpp).all() and np.isfinite(t[:, 1]).all() and (t[:, 1, 7] == 0).all()


@pytest.mark.parametrize("well", [401, 581])
def test_deep_columns_stay_finite_over_ten_days(well):
    st, cols, _ = _stepper(well, 64)
    try:
        st.set_enkf(48, 5.0, 0.0, 2)
        st.set_enkf_method("sqrt", 0.5)
        st.step_rows(1, 480)
        psi, t, Kr = st.get_state(), st.enkf_table()[0], st.enkf_sqrt_gain()
        sb, sa, f = st.enkf_relaxation_factors()
    finally:
        st.close()
    assert cols.dim_d == well and np.isfinite(psi).all()
    done = t[t[:, 0] > 0]
    assert done.shape[0] >= 9 and np.isfinite(done).all() and np.all(done[:, 7] == 0)
    assert np.abs(Kr).max() > 0.0 and np.isfinite(f).all() and np.isfinite(sb).all() and np.isfinite(sa).all()


def test_refusals_hooks_and_what_resets_the_method():
    from hydromodel_amd import _lib as L
    st, cols, _ = _stepper(1, 16)
    buf = np.zeros(16 * cols.dim_d * 4)
    try:
        with pytest.raises(L.HcError, match="the EnKF is off"):
            st.set_enkf_method("sqrt", 0.5)
        st.set_enkf(48, 5.0, 0.0, 1)
        assert st.get_enkf_method() == ("stochastic", 0.0)
        for method, alpha in ((2, 0.0), (-1, 0.0), (1, -0.1), (1, 1.5), (0, float("nan")), (0, float("inf"))):
            with pytest.raises(L.HcError, match="hc_set_enkf_method"):
                L.check(st.lib.hc_set_enkf_method(st.h, method, alpha))
        for bad in (("etkf", 0.0), ("sqrt", 2.0), ("sqrt", float("nan"))):
            with pytest.raises(ValueError):
                st.set_enkf_method(*bad)
        st.step_rows(1, 48)                                          # a stochastic analysis without relaxation
        assert st.enkf_eps().shape == (16,)
        for hook in (st.enkf_sqrt_gain, st.enkf_sqrt_shift, st.enkf_relaxation_factors):
            with pytest.raises(L.HcError):
                hook()
        st.set_enkf_method("sqrt", 0.5)
        assert st.get_enkf_method() == ("sqrt", 0.5)
        st.step_rows(49, 48)
        assert st.enkf_sqrt_gain().shape == (1, cols.dim_d, 1) and st.enkf_gain().shape == (1, cols.dim_d)
        with pytest.raises(L.HcError, match="hc_get_enkf_eps"):      # nothing was drawn
            st.enkf_eps()
        assert st.lib.hc_get_enkf_sm_eps(st.h, L.dptr(buf)) != 0
        st.set_enkf(48, 5.0, 0.0, 1)                                 # hc_set_enkf resets the method
        assert st.get_enkf_method() == ("stochastic", 0.0) and (st.enkf_method, st.enkf_relaxation) == ("stochastic", 0.0)
        with pytest.raises(L.HcError):
            st.enkf_sqrt_gain()
        st.set_enkf_method("sqrt", 1.0)
        st.set_noise_philox(2, 0)                                    # a new noise source turns the EnKF off
        assert st.get_enkf_method() == ("stochastic", 0.0)
        with pytest.raises(L.HcError, match="the EnKF is off"):
            st.set_enkf_method("sqrt", 0.0)
    finally:
        st.close()


def test_dump_and_restore_continue_a_square_root_run_bit_for_bit(tmp_path):
    from hydromodel_amd import hdf5io
    from hydromodel_amd.ensemble import EnsembleSimulation
    from hydromodel_amd.stepper import soil_moisture_record
    _, cols, forcing = digest(1)
    psi0 = _spread(golden("g1_tables_1.npz")["initial_cond"], 96)
    v = _record(forcing.dim_t, [0, 1], [0.22, 0.26], rows=(48, 96, 144, 192, 240))
    rec = soil_moisture_record(cols.z, [cols.z[0] + 30.0, cols.z[0] + 100.0], v, 0.02)
    kw = dict(seed=6, psi0=psi0, wtd_hist_stride=48, enkf_stride=48, enkf_sigma_cm=2.0 * cols.dz,
              enkf_localisation_cm=50.0, enkf_soil_moisture=rec)
    plain = EnsembleSimulation(cols, forcing, 96, **kw)
    try:
        plain.advance(60)
        keys_plain = set(hdf5io.read(plain.dump(tmp_path / "plain.h5")))
        assert plain.enkf_summary()["method"] == "stochastic" and plain.enkf_summary()["relaxation"] == 0.0
    finally:
        plain.close()
    whole = EnsembleSimulation(cols, forcing, 96, enkf_method="sqrt", enkf_relaxation=0.5, **kw)
    try:
        whole.advance(100)
        path = whole.dump(tmp_path / "ck.h5")
        whole.advance(140)
        want = [whole.stepper.get_state(), whole.enkf_table(), whole.enkf_sm_table(), whole.moments()]
        summary = whole.enkf_summary()
    finally:
        whole.close()
    assert set(hdf5io.read(path)) - keys_plain == METHOD_KEYS and not keys_plain & METHOD_KEYS
    assert summary["method"] == "sqrt" and summary["relaxation"] == 0.5
    back = EnsembleSimulation.restore(path, cols, forcing, enkf_soil_moisture=rec)
    try:
        assert (back.enkf_method, back.enkf_relaxation) == ("sqrt", 0.5)
        assert back.stepper.get_enkf_method() == ("sqrt", 0.5)
        back.advance(140)
        got = [back.stepper.get_state(), back.enkf_table(), back.enkf_sm_table(), back.moments()]
    finally:
        back.close()
    for a, b in zip(want, got):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    with pytest.raises(ValueError, match="need the EnKF"):
        EnsembleSimulation(cols, forcing, 8, seed=6, psi0=psi0[:8], enkf_method="sqrt")


def test_cli_method_keys_write_the_datasets(tmp_path, monkeypatch, capsys):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    params = _cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    files = {}
    for tag, extra in (("plain", {}), ("sqrt", {"Method": "sqrt", "Relaxation": 0.5}), ("relax", {"Relaxation": 0.25})):
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 64, "Seed": 3, "Days": 2, "EnKF": {"Stride": 24, "Sigma_cm": 10.0, **extra}}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = loadResults(tmp_path / f"Run_{tag}_ensemble.h5")
        assert "EnKF log-likelihood = " in capsys.readouterr().out
    plain, root, relax = files["plain"], files["sqrt"], files["relax"]
    assert not METHOD_KEYS & set(plain) and set(root) - set(plain) == METHOD_KEYS == set(relax) - set(plain)
    assert int(root["enkf_method"]) == 1 and float(root["enkf_relaxation"]) == 0.5
    assert int(relax["enkf_method"]) == 0 and float(relax["enkf_relaxation"]) == 0.25
    assert root["enkf_rows"].tolist() == [24, 48, 72, 96] and np.isfinite(root["enkf_post_std_cm"]).all()
    # the first analysis sees the same forecast: the same prior; the relaxed posterior is the wider one
    assert root["enkf_prior_std_cm"][0] == plain["enkf_prior_std_cm"][0] == relax["enkf_prior_std_cm"][0]
    assert not np.array_equal(root["enkf_post_mean_cm"], plain["enkf_post_mean_cm"])


def _twin(rows):
    """The set-up of test_gpu_enkf.test_twin_experiment_enkf_lowers_the_crps (well 1, 256 members, +-60 cm, truth at
    +35 cm under another seed): mean CRPS of the forecast for the open loop and the EnKF's schemes; for the relaxed one,
    per analysis row, the hooks' sigma_b, sigma_a and the per-node psi std before / after the relaxation."""
    from hydromodel_amd.stepper import wtd_distribution
    N = 256
    psi0 = golden("g1_tables_1.npz")["initial_cond"]
    shifts = np.random.default_rng(12).uniform(-60.0, 60.0, size=N)
    truth, cols, forcing = _stepper(1, 1, seed=999, spread=False)
    try:
        truth.set_state(psi0 + 35.0)
        w_truth = truth.step_rows(1, rows, want_wtd=True)["wtd"][:, 0]
    finally:
        truth.close()
    twin = copy.copy(forcing)
    obs = np.array(forcing.wtd_obs, dtype=np.int32)
    obs[1:rows + 1] = np.where(obs[1:rows + 1] >= 0, w_truth, -1)
    obs[rows + 1:] = -1
    twin.wtd_obs = obs
    crps, spreads = {}, []
    for tag, scheme in (("open", None), ("stochastic", ("stochastic", 0.0)), ("sqrt", ("sqrt", 0.0)),
                        ("sqrt+rtps", ("sqrt", 0.5))):
        st, _, _ = _stepper(1, N, seed=4, forcing=twin)
        try:
            st.set_state(psi0[None, :] + shifts[:, None])
            st.set_wtd_hist(48)
            if scheme is not None:
                st.set_enkf(48, 2.0 * cols.dz, 0.0, 17)
                st.set_enkf_method(*scheme)
            if tag == "sqrt+rtps":
                for day in range(rows // 48):                         # one analysis per call: the hooks of each
                    st.step_rows(1 + 48 * day, 48)
                    if obs[48 * (day + 1)] >= 0:
                        sb, sa, f = st.enkf_relaxation_factors()
                        spreads.append((sb[0], sa[0], st.get_state().std(axis=0, ddof=1)))
            else:
                st.step_rows(1, rows)
            hist = st.wtd_hist_table()[0]
        finally:
            st.close()
        crps[tag] = float(wtd_distribution(hist, obs, (0.5,), cols.dz, cols.z, 0, 48)["crps_mean_cm"])
    return crps, spreads


def test_twin_experiment_every_scheme_lowers_the_crps(capsys):
    crps, spreads = _twin(10 * 48)
    with capsys.disabled():
        print("\n twin experiment, 256 members, 10 days, +-60 cm spread: mean CRPS " +
              ", ".join(f"{k} {v:.4f} cm" for k, v in crps.items()))
    for tag in ("stochastic", "sqrt", "sqrt+rtps"):
        assert crps[tag] < crps["open"], tag
    assert len(spreads) >= 9
    for sb, sa, std_relaxed in spreads:                               # by construction: (1 - a) sigma_a + a sigma_b >= sigma_a
        wider = sb >= sa
        assert wider.any() and np.all(std_relaxed[wider] >= sa[wider] * (1.0 - 1e-12))
