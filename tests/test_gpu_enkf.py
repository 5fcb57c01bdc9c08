"""The ensemble Kalman filter on the GPU (include/hydrocol.h hc_set_enkf): y, eps, the gain and the analysis states against
a float64 NumPy restatement from the forecast states; the neutral EnKF against a run without it; invariance under launch
length, point order and the dealing of a sweep's points to handles; one member; the TWO-layout and split-column depths
(D = 401, 581) for finiteness only -- the analysis is compared with NumPy at every slot count, D = 41 ... 640, in
test_gpu_enkf_depths.py; a twin experiment against the open run and the particle filter; resume; the CLI's "Ensemble":
{"EnKF": ...} block."""
import copy
import json

import numpy as np
import pytest

from helpers import digest, golden
from helpers import cli_params as _cli_params, run_cli_ranks as _run_ranks

pytestmark = pytest.mark.gpu
M32 = 0xFFFFFFFF


def _spread(psi0, N, seed=12, width=60.0):
    """[N][D]: the initial profile shifted by a per-member offset, uniform over +-width cm: water tables in many cells."""
    return np.asarray(psi0)[None, :] + np.random.default_rng(seed).uniform(-width, width, size=N)[:, None]


def _stepper(well, N, P=1, noise="philox", seed=7, forcing=None, spread=True):
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, f0 = digest(well)
    forcing = f0 if forcing is None else forcing
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


def _philox(ctr, key):
    """Philox4x32-10 with Python integers (Salmon et al. 2011; the device's philox4x32_10)."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def _eps_restated(seed, gid, row):
    """eps_k: counter (0xFFFFFFFE, row, gid_lo, gid_hi) under the seed, Box-Muller's cosine branch."""
    r = _philox((0xFFFFFFFE, row, gid & M32, gid >> 32), (seed & M32, seed >> 32))
    a, b = (r[1] << 32) | r[0], (r[3] << 32) | r[2]
    u1 = ((a >> 11) + 0.5) / 9007199254740992.0
    u2 = ((b >> 11) + 0.5) / 9007199254740992.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def _find_wtd(psi, psat):
    """The step kernel's index: below the deepest node with psi < psi_sat, clamped to D - 1; 0 when every node is
    saturated (utilities.py:57-99)."""
    D = psi.shape[-1]
    out = np.zeros(psi.shape[0], dtype=np.int64)
    for k, col in enumerate(psi):
        unsat = np.flatnonzero(~(col >= psat))
        out[k] = 0 if unsat.size == 0 else min(unsat[-1] + 1, D - 1)
    return out


def _y_of(psi, b, psat, dz):
    """The continuous water table (depths from the top node, z_i = i dz)."""
    y = b.astype(np.float64) * dz
    for k in range(psi.shape[0]):
        i = int(b[k])
        if i >= 1 and psi[k, i - 1] < psat <= psi[k, i]:
            y[k] = float(i - 1) * dz + dz * (psat - psi[k, i - 1]) / (psi[k, i] - psi[k, i - 1])
    return y


def _analysis_numpy(psi, y, eps, obs, dz, sigma, loc, mpp):
    """Per point, float64 two-pass: ybar, v, psibar, c_d, the taper and the gain; then psi + K (o_k - y_k)."""
    from hydromodel_amd.stepper import gaspari_cohn
    N, D = psi.shape
    z = np.arange(D) * dz
    K = np.zeros((N // mpp, D))
    for p in range(N // mpp):
        sl = slice(p * mpp, (p + 1) * mpp)
        yb = y[sl].mean()
        a = y[sl] - yb
        n1 = max(mpp - 1, 1)
        v = (a @ a) / n1 if mpp > 1 else 0.0
        c = ((psi[sl] - psi[sl].mean(axis=0)).T @ a) / n1 if mpp > 1 else np.zeros(D)
        rho = gaspari_cohn(np.abs(z - yb) / loc) if loc > 0 else 1.0
        K[p] = rho * c / (v + sigma * sigma)
    innov = (obs * dz + sigma * eps) - y
    return K, psi + np.repeat(K, mpp, axis=0) * innov[:, None]


@pytest.mark.parametrize("noise", ["philox", "numpy"])
@pytest.mark.parametrize("well, P, mpp, loc", [
    (1, 1, 100, 0.0), (1, 3, 100, 60.0), (300, 1, 100, 0.0),
    (1, 1, 2500, 0.0), (1, 2, 2500, 80.0),                 # not a multiple of 64 or of a 256-member tile
])
def test_analysis_against_numpy(well, P, mpp, loc, noise):
    _check_analysis(well, P, mpp, loc, noise)


def _check_analysis(well, P, mpp, loc, noise, find_wtd=_find_wtd, y_of=_y_of, analysis=_analysis_numpy, eps_members=None,
                    mean_std=lambda x: (x.mean(), x.std(ddof=1))):
    """``find_wtd``, ``y_of``, ``analysis``, ``mean_std``: the restatements (a large ensemble passes forms without a loop
    over the members and with long sums); ``eps_members``: the members whose draw is restated (None: every member)."""
    N = P * mpp
    st, cols, forcing = _stepper(well, N, P, noise)
    D, dz, sigma, seed = cols.dim_d, cols.dz, 5.0, 11
    obs = int(forcing.wtd_obs[48])
    assert obs >= 0
    psat = float(cols.soil.psi_sat)
    try:
        st.set_enkf(48, sigma, loc, seed)
        kw = {"fresh_noise": _fresh(st, 1, 47, 1)} if noise == "numpy" else {}
        st.step_rows(1, 47, **kw)
        kw = {"fresh_noise": _fresh(st, 48, 1, 2)} if noise == "numpy" else {}
        out = st.step_rows(48, 1, want_wtd=True, want_psi=True, **kw)
        y, eps, K = st.enkf_y(), st.enkf_eps(), st.enkf_gain()
        post = st.get_state()
        table = st.enkf_table()
    finally:
        st.close()
    w, forecast = out["wtd"][0].astype(np.int64), out["psi"][0]
    assert np.array_equal(find_wtd(forecast, psat), w)                       # b is the row's wtd_out
    y_np = y_of(forecast, w, psat, dz)
    assert np.all(np.abs(y - y_np) <= 1e-12 * (1.0 + np.abs(y_np)))
    assert np.unique(y).size > np.unique(w).size                            # spread below one cell: a continuous y
    members = np.arange(N) if eps_members is None else np.asarray(eps_members)
    eps_np = np.array([_eps_restated(seed, int(m), 48) for m in members])    # one handle: global id = m
    assert eps.shape == (N,) and np.isfinite(eps).all()
    assert np.all(np.abs(eps[members] - eps_np) <= 1e-13 * (1.0 + np.abs(eps_np)))
    K_np, post_np = analysis(forecast, y, eps, obs, dz, sigma, loc, mpp)
    assert np.all(np.abs(K - K_np) <= 1e-10 * np.abs(K_np).max() + 1e-300)
    assert np.abs(K).max() > 0.0
    assert np.all(np.abs(post - post_np) <= 1e-9 * (1.0 + np.abs(post_np)))
    assert not np.array_equal(post, forecast)
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        t = table[p, 1]
        yb, sd = mean_std(y[sl])
        v = sd * sd
        assert t[0] == mpp and t[7] == 0
        assert abs(t[1] - yb) <= 1e-12 * abs(yb) and abs(t[2] - sd) <= 1e-10 * sd
        assert abs(t[3] - (obs * dz - yb)) <= 1e-10 * (1.0 + abs(t[3]))
        s2 = v + sigma * sigma
        inc = -0.5 * np.log(2.0 * np.pi * s2) - 0.5 * (obs * dz - yb) ** 2 / s2
        assert abs(t[4] - inc) <= 1e-10 * max(1.0, abs(inc))
        y_post = y_of(post[sl], find_wtd(post[sl], psat), psat, dz)
        yb_post, sd_post = mean_std(y_post)
        assert abs(t[5] - yb_post) <= 1e-9 * (1.0 + abs(yb_post))
        assert abs(t[6] - sd_post) <= 1e-9 * (1.0 + sd_post)
        assert np.isnan(table[p, 2:, 1:]).all() and np.all(table[p, 2:, 0] == 0)


def test_neutral_enkf_changes_nothing():
    """sigma = 1e100: K ~ c / 1e200 and K (o - y) ~ 1e-100 cm vanish against psi, so the states, moments and histograms
    equal those of a run without the EnKF to the bit: ending launches on analysis rows changes nothing."""
    N, rows = 64, 150
    got = []
    for on in (True, False):
        st, _, _ = _stepper(300, N, seed=5)
        try:
            st.set_wtd_hist(48)
            if on:
                st.set_enkf(48, 1e100, 0.0, 3)
            st.step_rows(1, rows)
            got.append((st.get_state(), st.moments(), st.wtd_hist_table()))
            if on:
                t = st.enkf_table()[0]
                assert t[1:4, 0].tolist() == [N] * 3 and np.all(t[1:4, 7] == 0)
        finally:
            st.close()
    for a, b in zip(*got):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def digest_point_like(n):
    """well 1 (D = 101) with the soil's n changed: a parameter point of a sweep"""
    from hydromodel_amd.digest import ColumnTables, ForcingDigest
    from hydromodel_amd.synthetic import default_parameters
    from helpers import WELLS, forcing_frame
    params = default_parameters()
    params["Soil_Properties"]["n"] = n
    cols = ColumnTables(params, WELLS[1])
    return params, cols, ForcingDigest(params, forcing_frame(1), cols)


NS, MPP, SEED = (1.6, 2.0, 2.4), 70, 31


def _point_handle(ids, rows_per_launch=0):
    """The handle a rank runs for the sweep points ``ids``: global member ids point-major, each point keyed by its first
    global member, spread states of the whole sweep; per point: states, EnKF table, moments, histograms."""
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
        st.step_rows(1, 150)
        n = len(ids)
        return dict(psi=st.get_state().reshape(n, MPP, -1), table=st.enkf_table(),
                    moments=np.asarray(st.moments()).reshape(n, 3, -1), hist=st.wtd_hist_table().reshape(n, -1))
    finally:
        st.close()


def test_results_do_not_depend_on_launch_length_point_order_or_handles():
    whole = _point_handle([0, 1, 2])
    assert (whole["table"][:, 1:7, 0] == MPP).all()            # six analyses per point
    runs = {"rows 1": (_point_handle([0, 1, 2], 1), [0, 1, 2]), "rows 7": (_point_handle([0, 1, 2], 7), [0, 1, 2]),
            "reversed": (_point_handle([2, 1, 0]), [2, 1, 0]), "split a": (_point_handle([0, 2]), [0, 2]),
            "split b": (_point_handle([1]), [1])}
    for tag, (part, ids) in runs.items():
        for j, k in enumerate(ids):
            for key in ("psi", "table", "moments", "hist"):
                a, b = whole[key][k], part[key][j]
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (tag, k, key)


def test_one_member_keeps_its_state_and_the_increment_is_the_gaussian_log_density():
    st, cols, forcing = _stepper(1, 1)
    sigma = 7.0
    try:
        st.set_enkf(48, sigma, 0.0, 1)
        st.step_rows(1, 47)
        out = st.step_rows(48, 1, want_psi=True)
        y = st.enkf_y()
        assert np.array_equal(st.get_state().reshape(-1), out["psi"][0][0]) and np.all(st.enkf_gain() == 0.0)
        t = st.enkf_table()[0]
    finally:
        st.close()
    d = float(forcing.wtd_obs[48]) * cols.dz - y[0]
    want = -0.5 * np.log(2.0 * np.pi * sigma * sigma) - 0.5 * d * d / (sigma * sigma)
    assert t[1, 0] == 1 and t[1, 2] == 0.0 and t[1, 6] == 0.0 and t[1, 1] == y[0] and t[1, 5] == y[0]
    assert abs(t[1, 4] - want) <= 1e-13 * max(1.0, abs(want))


@pytest.mark.parametrize("well", [401, 581])
def test_deep_columns_stay_finite_over_ten_days(well):
    """The TWO-layout build (D = 401) and the split column (D = 581)."""
    st, cols, _ = _stepper(well, 64)
    try:
        st.set_enkf(48, 5.0, 0.0, 2)
        st.step_rows(1, 480)
        psi, t, K = st.get_state(), st.enkf_table()[0], st.enkf_gain()
    finally:
        st.close()
    assert cols.dim_d == well and np.isfinite(psi).all()
    done = t[t[:, 0] > 0]
    assert done.shape[0] >= 9 and np.isfinite(done).all() and np.all(done[:, 7] == 0)
    assert np.abs(K).max() > 0.0


def _twin(rows, spread):
    """well 1, 256 members: open run, particle filter and EnKF against a synthetic truth (+35 cm, another seed) as the
    well; mean CRPS of the forecast over the histogram rows, and failed BDF attempts per member-day."""
    from hydromodel_amd.stepper import wtd_distribution
    N = 256
    psi0 = golden("g1_tables_1.npz")["initial_cond"]
    shifts = np.random.default_rng(12).uniform(-60.0, 60.0, size=N) if spread else np.zeros(N)
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
    crps, failed = {}, {}
    for tag in ("open", "filter", "enkf"):
        st, _, _ = _stepper(1, N, seed=4, forcing=twin)
        try:
            st.set_state(psi0[None, :] + shifts[:, None])
            st.set_wtd_hist(48)
            if tag == "filter":
                st.set_filter(48, 2.0 * cols.dz, 17)
            if tag == "enkf":
                st.set_enkf(48, 2.0 * cols.dz, 0.0, 17)
            out = st.step_rows(1, rows, want_stats=True)
            hist = st.wtd_hist_table()[0]
        finally:
            st.close()
        crps[tag] = float(wtd_distribution(hist, obs, (0.5,), cols.dz, cols.z, 0, 48)["crps_mean_cm"])
        failed[tag] = float(out["failed"].sum()) / (N * rows / 48.0)
    return crps, failed


def test_twin_experiment_enkf_lowers_the_crps(capsys):
    crps, failed = _twin(10 * 48, spread=True)
    flat, _ = _twin(20 * 48, spread=False)
    with capsys.disabled():
        print(f"\n twin experiment, 256 members, 10 days, +-60 cm spread: mean CRPS open {crps['open']:.4f} cm, "
              f"particle filter {crps['filter']:.4f} cm, EnKF {crps['enkf']:.4f} cm; failed BDF attempts per member-day "
              f"open {failed['open']:.4f}, EnKF {failed['enkf']:.4f}")
        print(f" without an initial spread, 20 days: open {flat['open']:.4f} cm, particle filter {flat['filter']:.4f} cm, "
              f"EnKF {flat['enkf']:.4f} cm")
    assert crps["enkf"] < crps["open"]


def test_dump_and_restore_continue_an_enkf_run_bit_for_bit(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(1)
    psi0 = _spread(golden("g1_tables_1.npz")["initial_cond"], 96)
    kw = dict(seed=6, psi0=psi0, wtd_hist_stride=48, enkf_stride=48, enkf_sigma_cm=2.0 * cols.dz,
              enkf_localisation_cm=50.0)
    whole = EnsembleSimulation(cols, forcing, 96, **kw)
    try:
        whole.advance(100)
        path = whole.dump(tmp_path / "ck.h5")
        whole.advance(140)
        want = [whole.stepper.get_state(), whole.enkf_table(), whole.moments(), whole.wtd_hist_table(),
                whole.stepper.noise_scale()]
        summary = whole.enkf_summary()
    finally:
        whole.close()
    back = EnsembleSimulation.restore(path, cols, forcing)
    try:
        assert back.next_row == 101 and back.enkf_stride == 48 and back.enkf_localisation_cm == 50.0
        back.advance(140)
        got = [back.stepper.get_state(), back.enkf_table(), back.moments(), back.wtd_hist_table(),
               back.stepper.noise_scale()]
    finally:
        back.close()
    for a, b in zip(want, got):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert summary["rows"].tolist() == [48, 96, 144, 192, 240] and np.isfinite(summary["loglik"])


def test_enkf_and_particle_filter_refuse_each_other():
    from hydromodel_amd import _lib as L
    st, cols, _ = _stepper(1, 8)
    try:
        st.set_enkf(48, 5.0, 0.0, 1)
        with pytest.raises(L.HcError, match="the EnKF is on"):
            L.check(st.lib.hc_set_filter(st.h, 48, 5.0, 1))
        assert st.enkf_table().shape[-1] == 8                  # still on
        st.set_enkf(0)
        st.set_filter(48, 5.0, 1)
        with pytest.raises(L.HcError, match="the particle filter is on"):
            L.check(st.lib.hc_set_enkf(st.h, 48, 5.0, 0.0, 1))
        st.set_filter(0)
        for bad in ((48, 0.0, 0.0), (48, np.inf, 0.0), (48, 5.0, -1.0), (48, 5.0, np.nan)):
            with pytest.raises(L.HcError):
                L.check(st.lib.hc_set_enkf(st.h, *bad, 1))
    finally:
        st.close()


ENKF_KEYS = {"enkf_rows", "enkf_count", "enkf_prior_mean_cm", "enkf_prior_std_cm", "enkf_innovation_cm",
             "enkf_post_mean_cm", "enkf_post_std_cm", "enkf_loglik_rows", "enkf_rejected", "enkf_loglik", "enkf_sigma_cm",
             "enkf_localisation_cm"}


def test_cli_enkf_block_writes_the_datasets(tmp_path, monkeypatch, capsys):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    params = _cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    pts = [{"Soil_Properties": {"n": 1.6}}, {"Soil_Properties": {"n": 2.4}}]
    files, logs = {}, {}
    for tag, extra in (("plain", {}), ("ens", {"EnKF": {"Stride": 24, "Sigma_cm": 10.0}}),
                       ("sweep", {"Points": pts, "EnKF": {"Sigma_cm": 10.0, "Localisation_cm": 40, "Seed": 4}})):
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 64, "Seed": 3, "Days": 2, **extra}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = loadResults(tmp_path / f"Run_{tag}_ensemble.h5")
        logs[tag] = capsys.readouterr().out
    plain, ens, sweep = files["plain"], files["ens"], files["sweep"]
    assert "EnKF log-likelihood" not in logs["plain"] and not any(k.startswith("enkf") for k in plain)
    assert set(ens) - set(plain) == ENKF_KEYS
    assert ens["enkf_rows"].tolist() == [24, 48, 72, 96]
    for k in ("enkf_count", "enkf_prior_mean_cm", "enkf_prior_std_cm", "enkf_innovation_cm", "enkf_post_mean_cm",
              "enkf_post_std_cm", "enkf_loglik_rows", "enkf_rejected"):
        assert ens[k].shape == (4,), k
    assert ens["enkf_count"].tolist() == [64] * 4 and float(ens["enkf_sigma_cm"]) == 10.0
    assert float(ens["enkf_localisation_cm"]) == 0.0
    assert np.isclose(float(ens["enkf_loglik"]), ens["enkf_loglik_rows"].sum(), rtol=1e-12)
    assert f"[Ensemble x64] EnKF log-likelihood = {float(ens['enkf_loglik']):.3f} over 4 rows" in logs["ens"]
    assert sweep["enkf_rows"].tolist() == [48, 96]
    for k in ("enkf_count", "enkf_prior_mean_cm", "enkf_loglik_rows", "enkf_rejected"):
        assert sweep[k].shape == (2, 2), k
    assert sweep["enkf_loglik"].shape == (2,) and np.isfinite(sweep["enkf_loglik"]).all()
    assert "[Sweep 2 points x64] EnKF log-likelihood: best point " in logs["sweep"]


def test_an_enkf_sweep_on_two_ranks_writes_what_one_rank_writes(tmp_path):
    params = _cli_params(tmp_path)
    params["Ensemble"] = {"Members": 40, "Seed": 5, "Days": 2, "Distribution": {"Stride": 48},
                          "Points": [{"Soil_Properties": {"n": n}} for n in (1.6, 2.0, 2.4)],
                          "EnKF": {"Stride": 24, "Sigma_cm": 8.0}}
    one, log1 = _run_ranks(tmp_path, "one", params, 1)
    two, log2 = _run_ranks(tmp_path, "two", params, 2)
    for k in sorted(ENKF_KEYS) + ["moments", "wtd_hist"]:
        a, b = np.asarray(one[k]), np.asarray(two[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    line = [s for s in log1.splitlines() if "EnKF log-likelihood" in s]
    assert len(line) == 1 and line == [s for s in log2.splitlines() if "EnKF log-likelihood" in s]
