"""The members' forcing state in the EnKF's analysis on the GPU (include/hydrocol.h hc_set_enkf_forcing): the gain, the
analysed g and the diagnostics against ``stepper.enkf_forcing_analysis_of`` from the forecast read back through the hooks; a
psi analysis that is not disturbed; the neutral analysis; the analysed g as what the next rows integrate with; the same
bits under re-arrangement; the refusals of the C layer; resume; the CLI's ``Forcing_Perturbation.EnKF`` key."""
import json

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: a shard's buffer is torch's, one HIP runtime serves both)

from helpers import digest, golden
from helpers import cli_params as _cli_params, run_cli_ranks as _run_ranks
from test_gpu_enkf import _fresh, _spread, _stepper, digest_point_like
from test_gpu_enkf_noise import NODES, PRESENT, S_SIG, VALS, _prepare, _same
from test_gpu_enkf_sm import _record

pytestmark = pytest.mark.gpu

SP, SD, TAU, FSEED = 0.3, 0.1, 3.0, 2024


def _start(well, N, P, noise, wide, loc, method, alpha, alpha_g, sd=SD, stride=48, noise_field=None, key=True, sigma=5.0):
    """A handle in the order a run sets it up: the perturbation, the EnKF, the noise field, the forcing analysis."""
    st, cols, forcing = _stepper(well, N, P, noise)
    try:
        st.set_forcing_perturbation(SP, sd, TAU, FSEED)
        _prepare(st, wide, loc, method, alpha, sigma=sigma, stride=stride)
        if noise_field is not None:
            st.set_enkf_noise_field(True, noise_field)
        if key:
            st.set_enkf_forcing(True, alpha_g)
    except Exception:
        st.close()
        raise
    return st, cols, forcing


def _to_row_48(st, noise):
    kw = {"fresh_noise": _fresh(st, 1, 47, 1)} if noise == "numpy" else {}
    st.step_rows(1, 47, **kw)
    kw = {"fresh_noise": _fresh(st, 48, 1, 2)} if noise == "numpy" else {}
    return st.step_rows(48, 1, want_psi=True, **kw)["psi"][0]


def _forecast(well, N, P, noise, wide, loc, method, alpha, sd, noise_field):
    """(g [2][N] at day 1, psi) as the analysis of row 48 finds them: the same run with its analyses on every 96th row."""
    st, _, _ = _start(well, N, P, noise, False, loc, method, alpha, 0.0, sd, stride=96, noise_field=noise_field)
    try:
        psi = _to_row_48(st, noise)
        g, day = st.forcing_state()
        assert day == 1
        return g, psi
    finally:
        st.close()


# 100 / 257 / 2 500 members a point: less than a tile of 256, a tile and one member, ten tiles with a ragged last one
CASES = [
    # well, P, mpp, noise, wide, loc, method, alpha (psi), alpha_g, noise field's relaxation or None, sigma_demand
    (1, 1, 100, "numpy", False, 0.0, "stochastic", 0.0, 0.0, None, SD),
    (1, 3, 257, "philox", True, 60.0, "stochastic", 0.5, 0.25, None, SD),
    (300, 1, 257, "philox", True, 0.0, "sqrt", 0.0, 0.5, None, SD),
    (300, 3, 100, "numpy", False, 50.0, "sqrt", 0.5, 0.0, None, SD),
    (1, 1, 2500, "philox", False, 80.0, "sqrt", 0.5, 0.25, 0.5, SD),
    (1, 3, 2500, "numpy", True, 0.0, "stochastic", 0.0, 0.5, None, 0.0),
    (300, 1, 2500, "numpy", True, 50.0, "sqrt", 0.0, 0.0, None, SD),
    (300, 1, 2500, "philox", False, 0.0, "stochastic", 0.5, 0.5, None, SD),
]


@pytest.mark.parametrize("well, P, mpp, noise, wide, loc, method, alpha, alpha_g, nz, sd", CASES)
def test_analysis_against_the_restatement(well, P, mpp, noise, wide, loc, method, alpha, alpha_g, nz, sd):
    from hydromodel_amd.stepper import enkf_forcing_analysis_of, split_enkf_forcing_table
    N, sigma = P * mpp, 5.0
    g_f, psi_f = _forecast(well, N, P, noise, wide, loc, method, alpha, sd, nz)
    st, cols, forcing = _start(well, N, P, noise, wide, loc, method, alpha, alpha_g, sd, noise_field=nz)
    dz = cols.dz
    try:
        assert st.get_enkf_forcing() == (True, alpha_g)
        _same(_to_row_48(st, noise), psi_f, "forecast")               # the twin run is this run up to the analysis
        W = st.enkf_width()
        Y = np.concatenate([st.enkf_sm_y(), st.enkf_window_y()], axis=1) if wide else st.enkf_y()[:, None]
        Kg = st.enkf_forcing_gain()
        if method == "sqrt":
            Krg, shift = st.enkf_forcing_sqrt_gain(), st.enkf_forcing_sqrt_shift()
            E = None
        else:
            E = (np.concatenate([st.enkf_eps()[:, None], st.enkf_sm_eps()[:, PRESENT], st.enkf_window_eps()], axis=1)
                 if wide else st.enkf_eps()[:, None])
        g_a, day = st.forcing_state()
        stats, rej = split_enkf_forcing_table(st.enkf_forcing_table())
        psi_rejected = st.enkf_table()[:, 1, 7]
    finally:
        st.close()
    assert day == 1 and W == (4 if wide else 1) and Y.shape == (N, W) and Kg.shape == (P, W, 2)
    obs, sig, zeta = [float(forcing.wtd_obs[48]) * dz], [sigma], []
    if wide:
        lag = float(forcing.wtd_obs[36]) * dz
        obs += [VALS[0], VALS[2], lag]
        sig += [S_SIG[0], S_SIG[2], sigma]
        zeta = [NODES[0] * dz, NODES[2] * dz, lag]
    active = (True, sd > 0.0)
    assert not np.array_equal(g_a[0], g_f[0]) and np.isfinite(g_a).all() and (psi_rejected == 0).all()
    if sd > 0.0:
        assert not np.array_equal(g_a[1], g_f[1])
    else:
        _same(g_a[1], g_f[1], "a stream with sigma = 0 keeps every bit")
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        res = enkf_forcing_analysis_of(psi_f[sl], g_f[:, sl].T, Y[sl], obs, sig, None if E is None else E[sl], active=active,
                                       zeta=zeta, dz=dz, localisation_cm=loc, method=method, relaxation=alpha_g)

        def close(got, want, tag, bar=1e-10):                         # LAB_NOTES 13: of the array's largest entry
            err = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
            print(f" {tag}[{p}]: {err:.1e}", end="")
            assert got.shape == want.shape and err <= bar, (tag, p, err)

        close(Kg[p], res["K"], "K")
        assert np.abs(Kg[p]).max() > 0.0
        if method == "sqrt":
            close(Krg[p], res["Kr"], "Kr")
            close(shift[p], res["shift"], "shift")
        err = float(np.max(np.abs(g_a[:, sl].T - res["g"]) / np.maximum(1.0, np.abs(res["g"]))))
        print(f" g[{p}]: {err:.1e}", end="")
        assert err <= 1e-9, (p, err)
        assert not res["rejected"].any() and rej[p, 1] == 0
        for k, tag in enumerate(("prior mean", "prior std", "post mean", "post std")):
            assert np.abs(stats[p, 1, k] - res["stats"][k]).max() <= 1e-10, (tag, p)
        if sd == 0.0:
            _same(stats[p, 1, 2:, 1], stats[p, 1, :2, 1], "post = prior")
        if alpha_g:                                                   # what the relaxation is for
            blend = (1.0 - alpha_g) * res["sigma_a"] + alpha_g * res["sigma_b"]
            got = g_a[:, sl].std(axis=1, ddof=1)
            assert np.abs(got - blend)[np.array(active)].max() <= 1e-9 * res["sigma_b"].max()
        assert np.isnan(stats[p, 2:]).all() and np.isnan(rej[p, 2:]).all() and np.isnan(rej[p, 0])
    print()


def _long_run(key, rows=150, sigma=None, well=300, N=96, alpha_g=0.5, noise_field=None, analysed_rows=(48,)):
    """Three analyses (rows 48, 96, 144) of a host-noise run with perturbed forcing: the state and the hooks after each of
    ``analysed_rows`` and at the end."""
    st, cols, forcing = _stepper(well, N, 1, "numpy", seed=5)
    try:
        st.set_forcing_perturbation(SP, SD, TAU, FSEED)
        st.set_wtd_hist(48)
        st.set_enkf(48, 2.0 * cols.dz if sigma is None else sigma, 40.0, 3)
        st.set_enkf_soil_moisture(NODES, _record(st.T, NODES, [0.22, 0.26, 0.2], rows=(48, 144)),
                                  0.02 if sigma is None else sigma)
        if noise_field is not None:
            st.set_enkf_noise_field(True, noise_field)
        if key:
            st.set_enkf_forcing(True, alpha_g)
        fresh = _fresh(st, 1, rows, 9)
        got, row, used = {}, 1, 0
        for stop in list(analysed_rows) + [rows]:
            n = st.n_refresh(row, stop - row + 1)
            st.step_rows(row, stop - row + 1, fresh_noise=fresh[used:used + n])
            used += n
            row = stop + 1
            got[stop] = dict(psi=st.get_state(), table=st.enkf_table(), gain=st.enkf_sm_gain(), g=st.forcing_state()[0],
                             base=st.enkf_noise_base())
        got["end"] = dict(psi=st.get_state(), moments=np.asarray(st.moments()), hist=st.wtd_hist_table(),
                          g=got[rows]["g"], factors=st.forcing_factors(0, N, 0, 4))
        if key:
            got["forcing_table"] = st.enkf_forcing_table()
        return got
    finally:
        st.close()


@pytest.mark.parametrize("noise_field", [None, 0.5])
def test_the_psi_analysis_is_not_disturbed(noise_field):
    off, on = _long_run(False, noise_field=noise_field), _long_run(True, noise_field=noise_field)
    for k in ("psi", "table", "gain", "base"):                        # the first analysis: the same bits, z's too
        _same(off[48][k], on[48][k], k)
    assert not np.array_equal(off[48]["g"], on[48]["g"])              # ... but g changed,
    assert not np.array_equal(off["end"]["psi"], on["end"]["psi"])    # and so do the later states
    assert np.isfinite(on["end"]["psi"]).all() and np.isfinite(on["end"]["g"]).all()


def test_the_neutral_analysis_changes_nothing():
    off, on = _long_run(False, sigma=1e30), _long_run(True, sigma=1e30, alpha_g=0.0)
    for k in ("psi", "moments", "hist", "g", "factors"):
        _same(off["end"][k], on["end"][k], k)
    assert (on["forcing_table"][0, 1:4, 8] == 0).all()


def test_the_analysed_g_is_what_the_next_rows_integrate_with():
    """Two points of 70 members at D = 101.  After the analysis of row 48 the carried state is the analysed g at day 1.
    Rows 49 ... 96 of members of either point are then, bit for bit, those of a one-member handle that is given the
    member's analysed psi and analysed g at day 1 (the factor the step kernel applies is the device's exp of that g,
    which no accessor returns for a g that is not the stateless recursion's: so the one-member run takes g, not a scaled
    record), and the day-2 state is the recursion's step from the analysed g."""
    from hydromodel_amd.stepper import EnsembleStepper, forcing_coefficients
    phi, c = forcing_coefficients(TAU)
    mpp, ids = 70, (0, 2)
    pts = [digest_point_like((1.6, 2.0, 2.4)[k]) for k in ids]
    cols, forcing = [q[1] for q in pts], pts[0][2]
    psi_all = _spread(golden("g1_tables_1.npz")["initial_cond"], 3 * mpp, seed=4)
    psi0 = np.concatenate([psi_all[k * mpp:(k + 1) * mpp] for k in ids])
    bases = np.array(ids, dtype=np.int64) * mpp
    a = EnsembleStepper(cols, forcing, 2 * mpp)
    try:
        a.set_generic_exponents(True)
        a.set_state(psi0)
        a.set_noise_philox(31, 0)
        a.set_point_member_bases(bases)
        a.set_forcing_perturbation(SP, SD, TAU, FSEED)
        a.set_enkf(48, 2.0 * a.cols.dz, 40.0, 9)
        a.set_enkf_forcing(True, 0.25)
        a.step_rows(1, 47)
        g_f = a.forcing_state()[0]                                    # day 0 still: row 48 opens day 1
        a.step_rows(48, 1)
        psi_a, (g_a, day), scale = a.get_state(), a.forcing_state(), a.noise_scale()
        assert day == 1 and g_f.shape == g_a.shape
        out = a.step_rows(49, 47, want_psi=True, want_wtd=True)       # the rest of day 1
        _same(a.forcing_state()[0], g_a, "inside the day the carried state stays")
        a.set_enkf_forcing(False)                                     # row 96 opens day 2: its g is the recursion's, not analysed
        a.step_rows(96, 1)
        g_2, day = a.forcing_state()
        assert day == 2
        gid = lambda j: int(bases[j // mpp]) + j % mpp
        xi = np.stack([a.forcing_normals(gid(j), 1, 2) for j in range(2 * mpp)], axis=2)            # [2 days][2][N]
    finally:
        a.close()
    assert not np.array_equal(g_a, (phi * g_f) + (c * xi[0]))         # day 1's g is the analysed one, not the recursion's
    _same(g_2, (phi * g_a) + (c * xi[1]), "day 2 is the recursion's step from the analysed g")
    for j in (0, 69, 70, 139):
        b = EnsembleStepper(cols[j // mpp], forcing, 1)
        try:
            b.set_generic_exponents(True)
            b.set_state(psi_a[j])
            b.set_noise_philox(31, gid(j))
            b.set_noise_scale(scale[j:j + 1])
            b.set_forcing_perturbation(SP, SD, TAU, FSEED)
            b.set_forcing_state(g_a[:, j:j + 1], 1)
            want = b.step_rows(49, 47, want_psi=True, want_wtd=True)
            b.step_rows(96, 1)
            g_b, _ = b.forcing_state()
        finally:
            b.close()
        _same(out["psi"][:, j], want["psi"][:, 0], (j, "psi"))
        _same(out["wtd"][:, j], want["wtd"][:, 0], (j, "wtd"))
        _same(g_2[:, j], g_b[:, 0], (j, "g"))


NS, MPP, SEED = (1.6, 2.0, 2.4), 70, 31


def _point_handle(ids, rows_per_launch=0):
    """test_gpu_enkf_noise._point_handle with perturbed forcing and its analysis"""
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
        st.set_forcing_perturbation(SP, SD, TAU, FSEED)
        st.set_rows_per_launch(rows_per_launch)
        st.set_wtd_hist(48)
        st.set_enkf(24, 2.0 * st.cols.dz, 40.0, 9)
        st.set_enkf_soil_moisture([8], _record(st.T, [8], [0.22], rows=(24, 72, 120)), 0.02)
        st.set_enkf_method("stochastic", 0.25)
        st.set_enkf_forcing(True, 0.5)
        st.step_rows(1, 150)
        n = len(ids)
        g = st.forcing_state()[0].reshape(2, n, MPP)
        return dict(psi=st.get_state().reshape(n, MPP, -1), table=st.enkf_table(), forcing=st.enkf_forcing_table(),
                    g=np.ascontiguousarray(np.swapaxes(g, 0, 1)), gain=st.enkf_forcing_gain(),
                    moments=np.asarray(st.moments()).reshape(n, 3, -1), hist=st.wtd_hist_table().reshape(n, -1))
    finally:
        st.close()


def test_results_do_not_depend_on_launch_length_point_order_or_handles():
    whole = _point_handle([0, 1, 2])
    assert (whole["table"][:, 1:7, 0] == MPP).all() and np.isfinite(whole["forcing"][:, 1:7]).all()
    runs = {"rows 1": (_point_handle([0, 1, 2], 1), [0, 1, 2]), "rows 7": (_point_handle([0, 1, 2], 7), [0, 1, 2]),
            "rows 48": (_point_handle([0, 1, 2], 48), [0, 1, 2]), "reversed": (_point_handle([2, 1, 0]), [2, 1, 0]),
            "split a": (_point_handle([0, 2]), [0, 2]), "split b": (_point_handle([1]), [1])}
    for tag, (part, ids) in runs.items():
        for j, k in enumerate(ids):
            for key in whole:
                _same(whole[key][k], part[key][j], (tag, k, key))


def test_refusals_at_the_c_layer_and_what_turns_it_off():
    from hydromodel_amd import _lib as L
    st, cols, _ = _stepper(1, 256)

    def c_set(on, a):
        L.check(st.lib.hc_set_enkf_forcing(st.h, on, a))

    try:
        with pytest.raises(ValueError, match="needs the EnKF on"):
            st.set_enkf_forcing(True)
        with pytest.raises(L.HcError, match="the EnKF is off"):
            c_set(1, 0.0)
        st.set_enkf(48, 5.0, 0.0, 1)
        with pytest.raises(L.HcError, match="the forcing is not perturbed"):
            c_set(1, 0.0)
        st.set_forcing_perturbation(SP, SD, TAU, FSEED)
        for bad in (-0.1, 1.5, np.nan, np.inf):
            with pytest.raises(L.HcError, match="relaxation"):
                c_set(1, bad)
        with pytest.raises(L.HcError, match="bad argument"):
            c_set(2, 0.0)
        assert st.get_enkf_forcing() == (False, 0.0)
        with pytest.raises(L.HcError, match="the forcing analysis is off"):
            st.enkf_forcing_table()
        st.set_enkf_forcing(True, 0.25)
        assert st.get_enkf_forcing() == (True, 0.25) and st.enkf_forcing
        assert np.isnan(st.enkf_forcing_table()).all()
        with pytest.raises(L.HcError, match="no analysis since hc_set_enkf_forcing"):
            st.enkf_forcing_gain()
        with pytest.raises(L.HcError, match="the forcing analysis is on"):         # a shard after the key ...
            st.set_enkf_shard(256, 0)
        st.set_enkf_forcing(False)
        st.set_enkf_shard(256, 0)
        with pytest.raises(L.HcError, match="the analysis is sharded"):            # ... and the key after a shard
            c_set(1, 0.0)
        st.set_enkf_shard(0)
        st.set_enkf_forcing(True, 0.5)
        st.set_enkf(48, 5.0, 0.0, 1)                                  # setting the EnKF again turns it off
        assert st.get_enkf_forcing() == (False, 0.0) and not st.enkf_forcing
        st.set_enkf_forcing(True, 0.5)
        st.set_forcing_perturbation(SP, SD, TAU, FSEED)               # ... and so does setting the perturbation again
        assert st.get_enkf_forcing() == (False, 0.0) and not st.enkf_forcing
        st.set_enkf_forcing(True, 0.5)
        st.step_rows(1, 48)
        assert st.enkf_forcing_gain().shape == (1, 1, 2)
        with pytest.raises(L.HcError, match="no square-root analysis"):
            st.enkf_forcing_sqrt_gain()
    finally:
        st.close()


def test_dump_and_restore_continue_a_forcing_analysis_bit_for_bit(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(1)
    psi0 = _spread(golden("g1_tables_1.npz")["initial_cond"], 96)
    pert = {"precipitation_sigma": SP, "demand_sigma": SD, "correlation_days": TAU, "seed": FSEED, "enkf_relaxation": 0.5}
    kw = dict(seed=6, psi0=psi0, wtd_hist_stride=48, enkf_stride=48, enkf_sigma_cm=2.0 * cols.dz,
              enkf_localisation_cm=50.0, enkf_relaxation=0.25, forcing_perturbation=pert)
    whole = EnsembleSimulation(cols, forcing, 96, **kw)
    try:
        whole.advance(60)
        path = whole.dump(tmp_path / "ck.h5")
        whole.advance(90)
        want = [whole.stepper.get_state(), whole.enkf_table(), whole.enkf_forcing_table(), whole.moments(),
                whole.wtd_hist_table(), whole.stepper.forcing_state()[0]]
        summary = whole.enkf_summary()
    finally:
        whole.close()
    back = EnsembleSimulation.restore(path, cols, forcing)
    try:
        assert back.next_row == 61 and back.forcing_perturbation["enkf_relaxation"] == 0.5
        assert back.stepper.get_enkf_forcing() == (True, 0.5)
        assert np.isfinite(back.enkf_forcing_table()[1]).all() and np.isnan(back.enkf_forcing_table()[2]).all()
        back.advance(90)
        got = [back.stepper.get_state(), back.enkf_table(), back.enkf_forcing_table(), back.moments(),
               back.wtd_hist_table(), back.stepper.forcing_state()[0]]
    finally:
        back.close()
    for a, b in zip(want, got):
        _same(a, b)
    assert summary["rows"].tolist() == [48, 96, 144] and summary["forcing_relaxation"] == 0.5
    assert summary["forcing_post_std"].shape == (3, 2) and summary["forcing_rejected"].tolist() == [0] * 3
    assert summary["forcing_spread_ratio"].shape == (2,) and (summary["forcing_spread_ratio"] > 0.0).all()


FORCING_KEYS = {"enkf_forcing", "enkf_forcing_relaxation", "enkf_forcing_prior_mean", "enkf_forcing_prior_std",
                "enkf_forcing_post_mean", "enkf_forcing_post_std", "enkf_forcing_rejected"}
BLOCK = {"Precipitation_Sigma": SP, "Demand_Sigma": SD, "Correlation_Days": TAU}


def test_cli_key_writes_the_datasets_and_the_closing_line(tmp_path, monkeypatch, capsys):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    params = _cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    files, logs = {}, {}
    for tag, extra in (("off", {}), ("no", {"EnKF": False}), ("on", {"EnKF": True}), ("own", {"EnKF": {"Relaxation": 0.5}})):
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 64, "Seed": 3, "Days": 3, "EnKF": {"Stride": 48, "Sigma_cm": 10.0, "Relaxation": 0.25},
                              "Forcing_Perturbation": {**BLOCK, **extra}}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = loadResults(tmp_path / f"Run_{tag}_ensemble.h5")
        logs[tag] = capsys.readouterr().out
    off, no, on, own = (files[k] for k in ("off", "no", "on", "own"))
    assert "EnKF forcing" not in logs["off"] + logs["no"] and not any("enkf_forcing" in k for k in off)
    assert set(no) == set(off)
    for k in sorted(off):                                             # false is the run without the key
        _same(off[k], no[k], k)
    assert set(on) - set(off) == FORCING_KEYS and set(own) == set(on)
    assert int(on["enkf_forcing"]) == 1 and float(on["enkf_forcing_relaxation"]) == 0.25          # the EnKF block's
    assert float(own["enkf_forcing_relaxation"]) == 0.5
    assert on["enkf_rows"].tolist() == [48, 96, 144]
    for k in ("enkf_forcing_prior_mean", "enkf_forcing_prior_std", "enkf_forcing_post_mean", "enkf_forcing_post_std"):
        assert on[k].shape == (3, 2) and np.isfinite(on[k]).all(), k
    assert on["enkf_forcing_rejected"].tolist() == [0] * 3
    r = (on["enkf_forcing_post_std"] / on["enkf_forcing_prior_std"]).mean(axis=0)
    assert (f" [Ensemble x64] EnKF forcing: posterior spread {r[0]:.4f} / {r[1]:.4f} of prior (precipitation / demand) over "
            f"3 rows") in logs["on"]
    for k in ("enkf_prior_mean_cm", "enkf_prior_std_cm", "enkf_post_mean_cm", "enkf_post_std_cm"):
        assert on[k][0] == off[k][0] and own[k][0] == off[k][0], k   # the first analysis's psi diagnostics are the run's without
    assert not np.array_equal(on["enkf_prior_mean_cm"][1:], off["enkf_prior_mean_cm"][1:])        # ... the later ones are not


def test_a_sweep_on_two_ranks_writes_what_one_rank_writes(tmp_path):
    params = _cli_params(tmp_path)
    params["Ensemble"] = {"Members": 40, "Seed": 5, "Days": 2, "Distribution": {"Stride": 48},
                          "Points": [{"Soil_Properties": {"n": n}} for n in (1.6, 2.0, 2.2, 2.4)],
                          "EnKF": {"Stride": 24, "Sigma_cm": 8.0, "Relaxation": 0.25},
                          "Forcing_Perturbation": {**BLOCK, "EnKF": {"Relaxation": 0.5}}}
    one, log1 = _run_ranks(tmp_path, "one", params, 1)
    two, log2 = _run_ranks(tmp_path, "two", params, 2)
    assert FORCING_KEYS <= set(one) and set(one) == set(two)
    for k in sorted(k for k in one if k != "gpus"):
        _same(one[k], two[k], k)
    assert one["enkf_forcing_post_std"].shape == (4, 4, 2) and one["enkf_forcing_rejected"].shape == (4, 4)
    line = [s for s in log1.splitlines() if "EnKF forcing" in s]
    assert len(line) == 1 and line == [s for s in log2.splitlines() if "EnKF forcing" in s]
