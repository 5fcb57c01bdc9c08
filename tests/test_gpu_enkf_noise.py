"""The noise field in the EnKF's analysis on the GPU (include/hydrocol.h hc_set_enkf_noise_field): the gain, the analysed
base vectors and the diagnostics against ``stepper.enkf_noise_analysis_of`` from the forecast read back through the hooks;
a psi analysis that is not disturbed; the neutral analysis; the same bits under re-arrangement; the rejection rules; the
refusals of the noise path; resume; the CLI's ``Noise_Field`` key."""
import json

import numpy as np
import pytest

from helpers import digest, golden
from helpers import cli_params as _cli_params, run_cli_ranks as _run_ranks
from test_gpu_enkf import _fresh, _spread, _stepper, digest_point_like
from test_gpu_enkf_sm import _record

pytestmark = pytest.mark.gpu

NODES, VALS, S_SIG = [6, 20, 45], [0.27, np.nan, 0.24], np.array([0.02, 0.03, 0.025])     # two sensors present of three
PRESENT = [0, 2]


def _same(a, b, tag=None):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), tag


def _prepare(st, wide, loc, method, alpha, sigma=5.0, seed=11, stride=48):
    st.set_enkf(stride, sigma, loc, seed)
    if wide:                                         # m' = 4: two present sensors and one lagged row
        st.set_enkf_soil_moisture(NODES, _record(st.T, NODES, VALS), S_SIG)
        st.set_enkf_window([12])
    st.set_enkf_method(method, alpha)


def _forecast_base(well, N, P, noise, wide, loc, method, alpha):
    """The base vectors as the analysis of row 48 finds them: the same run with its analyses on every 96th row (so that
    a Philox run takes the same noise path), stepped through row 48."""
    st, _, _ = _stepper(well, N, P, noise)
    try:
        _prepare(st, False, loc, method, alpha, stride=96)
        st.set_enkf_noise_field(True, 0.0)
        kw = {"fresh_noise": _fresh(st, 1, 47, 1)} if noise == "numpy" else {}
        st.step_rows(1, 47, **kw)
        kw = {"fresh_noise": _fresh(st, 48, 1, 2)} if noise == "numpy" else {}
        out = st.step_rows(48, 1, want_psi=True, **kw)
        return st.enkf_noise_base(), out["psi"][0]
    finally:
        st.close()


# every value of the issue's list with every kernel it reaches: D = 101 / 300; 100 / 2 500 members; 1 / 3 points; host / Philox
# noise; m' = 1 / 4; taper off / on; both schemes; psi's relaxation 0 / 0.5 with the vectors' another one
CASES = [
    # well, P, mpp, noise, wide, loc, method, alpha (psi), alpha_z
    (1, 1, 100, "numpy", False, 0.0, "stochastic", 0.0, 0.0),
    (1, 3, 100, "philox", True, 60.0, "stochastic", 0.5, 0.25),
    (300, 1, 100, "philox", True, 0.0, "sqrt", 0.0, 0.5),
    (300, 3, 100, "numpy", False, 50.0, "sqrt", 0.5, 0.0),
    (1, 1, 2500, "philox", False, 80.0, "sqrt", 0.5, 0.25),
    (1, 3, 2500, "numpy", True, 0.0, "stochastic", 0.0, 0.5),
    (300, 1, 2500, "numpy", True, 50.0, "sqrt", 0.0, 0.0),
    (300, 1, 2500, "philox", False, 0.0, "stochastic", 0.5, 0.5),
]


@pytest.mark.parametrize("well, P, mpp, noise, wide, loc, method, alpha, alpha_z", CASES)
def test_analysis_against_the_restatement(well, P, mpp, noise, wide, loc, method, alpha, alpha_z):
    from hydromodel_amd.stepper import enkf_noise_analysis_of, split_enkf_noise_table
    N, sigma = P * mpp, 5.0
    z_f, psi_f = _forecast_base(well, N, P, noise, wide, loc, method, alpha)
    st, cols, forcing = _stepper(well, N, P, noise)
    D, dz = cols.dim_d, cols.dz
    try:
        _prepare(st, wide, loc, method, alpha)
        st.set_enkf_noise_field(True, alpha_z)
        assert st.get_enkf_noise_field() == (True, alpha_z)
        kw = {"fresh_noise": _fresh(st, 1, 47, 1)} if noise == "numpy" else {}
        st.step_rows(1, 47, **kw)
        kw = {"fresh_noise": _fresh(st, 48, 1, 2)} if noise == "numpy" else {}
        out = st.step_rows(48, 1, want_psi=True, **kw)
        _same(out["psi"][0], psi_f, "forecast")                       # the twin run is this run up to the analysis
        W = st.enkf_width()
        Y = np.concatenate([st.enkf_sm_y(), st.enkf_window_y()], axis=1) if wide else st.enkf_y()[:, None]
        Kz = st.enkf_noise_gain()
        if method == "sqrt":
            Krz, shift = st.enkf_noise_sqrt_gain(), st.enkf_noise_sqrt_shift()
            E = None
        else:
            E = (np.concatenate([st.enkf_eps()[:, None], st.enkf_sm_eps()[:, PRESENT], st.enkf_window_eps()], axis=1)
                 if wide else st.enkf_eps()[:, None])
        z_a = st.enkf_noise_base()
        stats, rej = split_enkf_noise_table(st.enkf_noise_table(), D)
        psi_rejected = st.enkf_table()[:, 1, 7]
    finally:
        st.close()
    assert W == (4 if wide else 1) and Y.shape == (N, W) and Kz.shape == (P, W, D)
    obs, sig, zeta = [float(forcing.wtd_obs[48]) * dz], [sigma], []
    if wide:
        lag = float(forcing.wtd_obs[36]) * dz
        obs += [VALS[0], VALS[2], lag]
        sig += [S_SIG[0], S_SIG[2], sigma]
        zeta = [NODES[0] * dz, NODES[2] * dz, lag]
    assert not np.array_equal(z_a, z_f) and np.isfinite(z_a).all() and (psi_rejected == 0).all()
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        res = enkf_noise_analysis_of(psi_f[sl], z_f[sl], Y[sl], obs, sig, None if E is None else E[sl], zeta=zeta, dz=dz,
                                     localisation_cm=loc, method=method, relaxation=alpha_z)

        def close(got, want, tag, bar=1e-10):                         # LAB_NOTES 13: of the array's largest entry
            err = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
            print(f" {tag}[{p}]: {err:.1e}", end="")
            assert got.shape == want.shape and err <= bar, (tag, p, err)

        close(Kz[p], res["K"], "K")
        assert np.abs(Kz[p]).max() > 0.0
        if method == "sqrt":
            close(Krz[p], res["Kr"], "Kr")
            close(shift[p], res["shift"], "shift")
        err = float(np.max(np.abs(z_a[sl] - res["z"]) / np.maximum(1.0, np.abs(res["z"]))))
        print(f" z[{p}]: {err:.1e}", end="")
        assert err <= 1e-9, (p, err)
        assert not res["rejected"].any() and rej[p, 1] == 0
        for k, tag in enumerate(("prior mean", "prior std", "post mean", "post std")):
            assert np.abs(stats[p, 1, k] - res["stats"][k]).max() <= 1e-10, (tag, p)
        if alpha_z:                                                   # what the relaxation is for
            blend = (1.0 - alpha_z) * res["sigma_a"] + alpha_z * res["sigma_b"]
            assert np.abs(z_a[sl].std(axis=0, ddof=1) - blend).max() <= 1e-9 * res["sigma_b"].max()
        assert np.isnan(stats[p, 2:]).all() and np.isnan(rej[p, 2:]).all() and np.isnan(rej[p, 0])
    print()


def _long_run(noise_field, noise="numpy", rows=150, sigma=None, well=300, N=96, alpha_z=0.5, base=None, fresh=None,
              sensors=True, analysed_rows=(48,)):
    """Three analyses (rows 48, 96, 144), the state and the hooks after each of ``analysed_rows`` and at the end."""
    st, cols, forcing = _stepper(well, N, 1, "philox" if noise == "philox" else "numpy", seed=5)
    try:
        if base is not None:
            st.set_noise_host(base)
        st.set_wtd_hist(48)
        st.set_enkf(48, 2.0 * cols.dz if sigma is None else sigma, 40.0, 3)
        if sensors:
            st.set_enkf_soil_moisture(NODES, _record(st.T, NODES, [0.22, 0.26, 0.2], rows=(48, 144)),
                                      0.02 if sigma is None else sigma)
        if noise_field:
            st.set_enkf_noise_field(True, alpha_z)
        if fresh is None and noise != "philox":
            fresh = _fresh(st, 1, rows, 9)
        got, row, used = {}, 1, 0
        for stop in list(analysed_rows) + [rows]:
            kw = {}
            if noise != "philox":
                n = st.n_refresh(row, stop - row + 1)
                kw["fresh_noise"] = fresh[used:used + n]
                used += n
            st.step_rows(row, stop - row + 1, **kw)
            row = stop + 1
            got[stop] = dict(psi=st.get_state(), table=st.enkf_table(), gain=st.enkf_sm_gain() if sensors else st.enkf_gain(),
                             base=st.enkf_noise_base() if (noise_field or noise != "philox") else None)
        got["end"] = dict(psi=st.get_state(), moments=np.asarray(st.moments()), hist=st.wtd_hist_table(),
                          base=got[rows]["base"])
        if noise_field:
            got["noise_table"] = st.enkf_noise_table()
        return got
    finally:
        st.close()


def test_the_psi_analysis_is_not_disturbed():
    off, on = _long_run(False), _long_run(True)
    for k in ("psi", "table", "gain"):                                # the first analysis: the same bits
        _same(off[48][k], on[48][k], k)
    assert not np.array_equal(off[48]["base"], on[48]["base"])        # ... but z changed,
    assert not np.array_equal(off["end"]["psi"], on["end"]["psi"])    # and so do the later states
    assert np.isfinite(on["end"]["psi"]).all() and np.isfinite(on["end"]["base"]).all()


def test_the_neutral_analysis_changes_nothing_host_noise():
    off, on = _long_run(False, sigma=1e30), _long_run(True, sigma=1e30, alpha_z=0.0)
    for k in ("psi", "moments", "hist", "base"):
        _same(off["end"][k], on["end"][k], k)
    assert (on["noise_table"][0, 1:4, -1] == 0).all()


def test_the_neutral_analysis_in_a_philox_run_is_the_host_noise_run_fed_its_normals():
    N, rows = 96, 150
    on = _long_run(True, noise="philox", sigma=1e30, alpha_z=0.0)
    ref, _, forcing = _stepper(300, N, seed=5)
    try:
        live = forcing.refresh.astype(bool) & (forcing.wtd_obs >= 0)
        draw = np.cumsum(live)
        base = np.stack([ref.philox_normals(m, 0) for m in range(N)])
        fresh = np.stack([np.stack([ref.philox_normals(m, int(draw[row])) for m in range(N)])
                          for row in range(1, rows + 1) if live[row]])
    finally:
        ref.close()
    want = _long_run(False, sigma=1e30, base=base, fresh=fresh)
    for k in ("psi", "moments", "hist", "base"):
        _same(want["end"][k], on["end"][k], k)


NS, MPP, SEED = (1.6, 2.0, 2.4), 70, 31


def _point_handle(ids, rows_per_launch=0):
    """test_gpu_enkf._point_handle with one sensor, relaxation and the noise field"""
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
        st.set_enkf_soil_moisture([8], _record(st.T, [8], [0.22], rows=(24, 72, 120)), 0.02)
        st.set_enkf_method("stochastic", 0.25)
        st.set_enkf_noise_field(True, 0.5)
        st.step_rows(1, 150)
        n = len(ids)
        return dict(psi=st.get_state().reshape(n, MPP, -1), table=st.enkf_table(), noise=st.enkf_noise_table(),
                    base=st.enkf_noise_base().reshape(n, MPP, -1), gain=st.enkf_noise_gain(),
                    moments=np.asarray(st.moments()).reshape(n, 3, -1), hist=st.wtd_hist_table().reshape(n, -1))
    finally:
        st.close()


def test_results_do_not_depend_on_launch_length_point_order_or_handles():
    whole = _point_handle([0, 1, 2])
    assert (whole["table"][:, 1:7, 0] == MPP).all() and np.isfinite(whole["noise"][:, 1:7]).all()
    runs = {"rows 1": (_point_handle([0, 1, 2], 1), [0, 1, 2]), "rows 7": (_point_handle([0, 1, 2], 7), [0, 1, 2]),
            "reversed": (_point_handle([2, 1, 0]), [2, 1, 0]), "split a": (_point_handle([0, 2]), [0, 2]),
            "split b": (_point_handle([1]), [1])}
    for tag, (part, ids) in runs.items():
        for j, k in enumerate(ids):
            for key in whole:
                _same(whole[key][k], part[key][j], (tag, k, key))


def test_a_member_whose_psi_analysis_is_rejected_keeps_its_vector():
    """sigma_cm = 1e200 is finite but its square is not: S has no Cholesky factor, the gain is NaN and the finiteness vote
    rejects every member's psi analysis -- no state is non-finite and nothing faults.  Every member then keeps its z to the
    bit and none is counted in noise_rejected."""
    N = 100
    z_f, _ = _forecast_base(1, N, 1, "numpy", False, 0.0, "stochastic", 0.0)
    st, cols, _ = _stepper(1, N, 1, "numpy")
    try:
        st.set_enkf(48, 1e200, 0.0, 11)
        st.set_enkf_noise_field(True, 0.5)
        st.step_rows(1, 47, fresh_noise=_fresh(st, 1, 47, 1))
        out = st.step_rows(48, 1, want_psi=True, fresh_noise=_fresh(st, 48, 1, 2))
        t, nt = st.enkf_table(), st.enkf_noise_table()
        _same(st.get_state(), out["psi"][0])
        _same(st.enkf_noise_base(), z_f)
    finally:
        st.close()
    assert t[0, 1, 7] == N and nt[0, 1, -1] == 0


def test_a_member_with_a_non_finite_base_entry_keeps_it_and_is_counted():
    """-inf in one member's base vector at the bottom node of the second of three points (a cell of no conductivity: the
    member's solves stay finite): the node's mean and gain are not finite, so no member of that point can take its update
    -- each keeps its vector and is counted, and its psi analysis stands; the other points are analysed as ever."""
    P, mpp = 3, 100
    N = P * mpp
    st, cols, _ = _stepper(1, N, P, "numpy")
    D = cols.dim_d
    try:
        base = st.get_noise_base()
        base[mpp + 17, D - 1] = -np.inf
        st.set_noise_host(base)
        st.set_enkf(48, 5.0, 0.0, 11)
        st.set_enkf_noise_field(True, 0.5)
        st.step_rows(1, 47, fresh_noise=_fresh(st, 1, 47, 1))
        before = st.get_noise_base()
        out = st.step_rows(48, 1, want_psi=True, want_stats=True, fresh_noise=_fresh(st, 48, 1, 2))
        after, t, nt = st.get_noise_base(), st.enkf_table(), st.enkf_noise_table()
        psi = st.get_state()
    finally:
        st.close()
    assert before[mpp + 17, D - 1] == -np.inf and after[mpp + 17, D - 1] == -np.inf
    ok = t[:, 1, 7] == 0
    assert ok[0] and ok[2]
    if ok[1] and out["failed"][0, mpp:2 * mpp].sum() == 0:            # (the member's own solve may have given up)
        assert nt[1, 1, -1] == mpp
        _same(after[mpp:2 * mpp], before[mpp:2 * mpp])
        assert not np.array_equal(psi[mpp:2 * mpp], out["psi"][0][mpp:2 * mpp])        # the psi update stands
    else:                                                             # its psi went non-finite: the whole point's psi
        assert nt[1, 1, -1] == 0                                      # analysis is rejected, and every vector is kept
        _same(after[mpp:2 * mpp], before[mpp:2 * mpp])
    for p in (0, 2):
        sl = slice(p * mpp, (p + 1) * mpp)
        assert nt[p, 1, -1] == 0 and not np.array_equal(after[sl], before[sl]) and np.isfinite(after[sl]).all()


def test_refusals_of_the_noise_path_and_the_filter_guard():
    from hydromodel_amd import _lib as L
    st, cols, _ = _stepper(1, 16)
    try:
        with pytest.raises(ValueError, match="needs the EnKF on"):
            st.set_enkf_noise_field(True)
        with pytest.raises(L.HcError, match="the EnKF is off"):
            L.check(st.lib.hc_set_enkf_noise_field(st.h, 1, 0.0))
        st.set_enkf(48, 5.0, 0.0, 1)
        st.set_enkf_method("sqrt", 0.25)
        for bad in (-0.1, 1.5, np.nan):
            with pytest.raises(L.HcError, match="relaxation"):
                L.check(st.lib.hc_set_enkf_noise_field(st.h, 1, bad))
        assert st.get_enkf_noise_field() == (False, 0.0)
        with pytest.raises(L.HcError, match="hc_get_enkf_noise_base"):
            st.enkf_noise_base()
        st.set_enkf_noise_field(True)                                 # the default is the block's relaxation
        assert st.get_enkf_noise_field() == (True, 0.25)
        with pytest.raises(L.HcError, match="noise field is on and the base vectors carry the damping"):
            st.set_noise_scale(np.full(16, 0.8))
        with pytest.raises(L.HcError, match="set it after the spin-up"):
            st.spinup(100.0, float(cols.z[0]))
        with pytest.raises(L.HcError, match="set it after the spin-up"):
            st.step_rows(0, 1, spinup=True, moments=False)
        with pytest.raises(L.HcError, match="a Philox run with the particle filter on"):   # the filter's guard, as before
            st.filter_base()
        with pytest.raises(L.HcError, match="no analysis since hc_set_enkf_noise_field"):
            st.enkf_noise_gain()
        assert st.enkf_noise_base().shape == (16, cols.dim_d)
        st.set_enkf_noise_field(False)
        assert st.get_enkf_noise_field() == (False, 0.0)
        st.set_noise_scale(np.full(16, 0.8))                          # accepted again
        st.set_enkf_noise_field(True, 0.5)
        st.set_enkf(48, 5.0, 0.0, 1)                                  # re-creating the EnKF turns it off
        assert st.get_enkf_noise_field() == (False, 0.0) and not st.enkf_noise_field
    finally:
        st.close()


def test_dump_and_restore_continue_a_noise_field_run_bit_for_bit(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(1)
    psi0 = _spread(golden("g1_tables_1.npz")["initial_cond"], 96)
    kw = dict(seed=6, psi0=psi0, wtd_hist_stride=48, enkf_stride=48, enkf_sigma_cm=2.0 * cols.dz,
              enkf_localisation_cm=50.0, enkf_relaxation=0.25, enkf_noise_field={"relaxation": 0.5})
    whole = EnsembleSimulation(cols, forcing, 96, **kw)
    try:
        whole.advance(100)
        path = whole.dump(tmp_path / "ck.h5")
        whole.advance(140)
        want = [whole.stepper.get_state(), whole.enkf_table(), whole.enkf_noise_table(), whole.moments(),
                whole.wtd_hist_table(), whole.stepper.enkf_noise_base()]
        summary = whole.enkf_summary()
    finally:
        whole.close()
    back = EnsembleSimulation.restore(path, cols, forcing)
    try:
        assert back.next_row == 101 and back.enkf_noise_relaxation == 0.5 and back.enkf_relaxation == 0.25
        assert back.stepper.get_enkf_noise_field() == (True, 0.5)
        back.advance(140)
        got = [back.stepper.get_state(), back.enkf_table(), back.enkf_noise_table(), back.moments(),
               back.wtd_hist_table(), back.stepper.enkf_noise_base()]
    finally:
        back.close()
    for a, b in zip(want, got):
        _same(a, b)
    D = cols.dim_d
    assert summary["rows"].tolist() == [48, 96, 144, 192, 240] and summary["noise_relaxation"] == 0.5
    assert summary["noise_post_std"].shape == (5, D) and summary["noise_rejected"].tolist() == [0] * 5
    assert 0.0 < summary["noise_spread_ratio"] <= 1.0


NOISE_KEYS = {"enkf_noise_field", "enkf_noise_relaxation", "enkf_noise_prior_mean", "enkf_noise_prior_std",
              "enkf_noise_post_mean", "enkf_noise_post_std", "enkf_noise_rejected"}


def test_cli_noise_field_key_writes_the_datasets(tmp_path, monkeypatch, capsys):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    params = _cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    files, logs = {}, {}
    block = {"Stride": 24, "Sigma_cm": 10.0, "Relaxation": 0.25}
    for tag, extra in (("off", {"Noise_Field": False}), ("on", {"Noise_Field": True}),
                       ("own", {"Noise_Field": {"Relaxation": 0.5}})):
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 64, "Seed": 3, "Days": 2, "EnKF": {**block, **extra}}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = loadResults(tmp_path / f"Run_{tag}_ensemble.h5")
        logs[tag] = capsys.readouterr().out
    off, on, own = files["off"], files["on"], files["own"]
    D = off["initial_cond"].shape[-1]
    assert "noise field" not in logs["off"] and not any("noise" in k for k in off)
    assert set(on) - set(off) == NOISE_KEYS and set(own) == set(on)
    assert int(on["enkf_noise_field"]) == 1 and float(on["enkf_noise_relaxation"]) == 0.25      # the block's
    assert float(own["enkf_noise_relaxation"]) == 0.5
    assert on["enkf_rows"].tolist() == [24, 48, 72, 96]
    for k in ("enkf_noise_prior_mean", "enkf_noise_prior_std", "enkf_noise_post_mean", "enkf_noise_post_std"):
        assert on[k].shape == (4, D) and np.isfinite(on[k]).all(), k
    assert on["enkf_noise_rejected"].tolist() == [0] * 4
    r = on["enkf_noise_post_std"] / on["enkf_noise_prior_std"]
    ratio = float(r[np.isfinite(r) & (on["enkf_noise_prior_std"] > 0)].mean())
    assert 0.0 < ratio <= 1.0
    assert f" [Ensemble x64] EnKF noise field: posterior spread {ratio:.4f} of prior over 4 rows" in logs["on"]
    # the first analysis's psi diagnostics are those of the run without the key
    for k in ("enkf_prior_mean_cm", "enkf_prior_std_cm", "enkf_post_mean_cm", "enkf_post_std_cm"):
        assert on[k][0] == off[k][0] and own[k][0] == off[k][0], k
    assert not np.array_equal(on["enkf_prior_mean_cm"][1:], off["enkf_prior_mean_cm"][1:])      # ... the later ones are not


def test_cli_refuses_the_noise_field_on_a_sharded_single_point(tmp_path, capsys):
    from hydromodel_amd import cli
    params = _cli_params(tmp_path)
    params["Ensemble"] = {"Members": 64, "Days": 1, "EnKF": {"Sigma_cm": 10.0, "Sharded": True, "Noise_Field": True}}
    (tmp_path / "p.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as stop:
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "p.json")])
    assert stop.value.code == 1
    assert "the partials the ranks exchange cover psi only" in capsys.readouterr().out


def test_a_noise_field_sweep_on_two_ranks_writes_what_one_rank_writes(tmp_path):
    params = _cli_params(tmp_path)
    params["Ensemble"] = {"Members": 40, "Seed": 5, "Days": 2, "Distribution": {"Stride": 48},
                          "Points": [{"Soil_Properties": {"n": n}} for n in (1.6, 2.0, 2.2, 2.4)],
                          "EnKF": {"Stride": 24, "Sigma_cm": 8.0, "Relaxation": 0.25, "Sharded": True,
                                   "Noise_Field": {"Relaxation": 0.5}}}
    one, log1 = _run_ranks(tmp_path, "one", params, 1)
    two, log2 = _run_ranks(tmp_path, "two", params, 2)
    assert NOISE_KEYS <= set(one) and set(one) == set(two)
    for k in sorted(k for k in one if k != "gpus"):
        _same(one[k], two[k], k)
    assert one["enkf_noise_post_std"].shape[:2] == (4, 4) and one["enkf_noise_rejected"].shape == (4, 4)
    line = [s for s in log1.splitlines() if "EnKF noise field" in s]
    assert len(line) == 1 and line == [s for s in log2.splitlines() if "EnKF noise field" in s]


def _twin(rows=10 * 48):
    """The set-up of test_gpu_enkf.test_twin_experiment_enkf_lowers_the_crps (well 1, 256 members, +-60 cm offsets, the
    truth at +35 cm with its own seed, sigma = 2 dz): the state-only EnKF against the EnKF with the noise field
    (relaxation 0.5).  The truth's base vector is its Philox draw 0."""
    import copy
    from hydromodel_amd.stepper import split_enkf_noise_table, wtd_distribution
    N = 256
    psi0 = golden("g1_tables_1.npz")["initial_cond"]
    shifts = np.random.default_rng(12).uniform(-60.0, 60.0, size=N)
    truth, cols, forcing = _stepper(1, 1, seed=999, spread=False)
    try:
        truth.set_state(psi0 + 35.0)
        z_truth = truth.philox_normals(0, 0)
        w_truth = truth.step_rows(1, rows, want_wtd=True)["wtd"][:, 0]
    finally:
        truth.close()
    twin = copy.copy(forcing)
    obs = np.array(forcing.wtd_obs, dtype=np.int32)
    obs[1:rows + 1] = np.where(obs[1:rows + 1] >= 0, w_truth, -1)
    obs[rows + 1:] = -1
    twin.wtd_obs = obs
    layered = np.flatnonzero(np.asarray(cols.noisec_node) >= 0)       # the nodes that belong to a layer
    res = {}
    for tag in ("state", "noise"):
        st, _, _ = _stepper(1, N, seed=4, forcing=twin)
        try:
            st.set_state(psi0[None, :] + shifts[:, None])
            st.set_wtd_hist(48)
            st.set_enkf(48, 2.0 * cols.dz, 0.0, 17)
            if tag == "noise":
                st.set_enkf_noise_field(True, 0.5)
            out = st.step_rows(1, rows, want_stats=True)
            hist = st.wtd_hist_table()[0]
            r = dict(crps=float(wtd_distribution(hist, obs, (0.5,), cols.dz, cols.z, 0, 48)["crps_mean_cm"]),
                     failed=float(out["failed"].sum()) / (N * rows / 48.0), psi=st.get_state())
            if tag == "noise":
                stats, rej = split_enkf_noise_table(st.enkf_noise_table()[0], cols.dim_d)
                done = np.flatnonzero(np.isfinite(rej))
                r.update(base=st.enkf_noise_base(), rejected=int(rej[done].sum()), analyses=done.size,
                         rmse_before=float(np.sqrt(np.mean((stats[done[0], 0] - z_truth)[layered] ** 2))),
                         rmse_after=float(np.sqrt(np.mean((stats[done[-1], 2] - z_truth)[layered] ** 2))),
                         ratio=float(np.mean(stats[done, 3][:, layered] / stats[done, 1][:, layered])))
            res[tag] = r
        finally:
            st.close()
    return res


def test_twin_experiment_with_the_noise_field(capsys):
    """Recorded, not gated on a number chosen in advance (LAB_NOTES.md 28): what holds by construction is asserted."""
    res = _twin()
    s, n = res["state"], res["noise"]
    with capsys.disabled():
        print(f"\n twin experiment, 256 members, 10 days: forecast CRPS state-only {s['crps']:.4f} cm, with the noise field "
              f"{n['crps']:.4f} cm; RMSE of the ensemble-mean z against the truth's {n['rmse_before']:.4f} -> "
              f"{n['rmse_after']:.4f}; failed BDF attempts per member-day {s['failed']:.4f} / {n['failed']:.4f}; spread "
              f"ratio {n['ratio']:.4f} over {n['analyses']} analyses, {n['rejected']} vectors refused")
    assert np.isfinite(s["psi"]).all() and np.isfinite(n["psi"]).all() and np.isfinite(n["base"]).all()
    assert np.isfinite(s["failed"]) and np.isfinite(n["failed"]) and s["failed"] >= 0.0 and n["failed"] >= 0.0
    assert 0.0 < n["ratio"] <= 1.0 and n["analyses"] == 10
