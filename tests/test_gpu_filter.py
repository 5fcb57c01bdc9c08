"""The particle filter on the GPU (include/hydrocol.h hc_set_filter): the ancestors against a Python-integer restatement
from the members' water tables, the exported q_b and the draw r; q_b against NumPy; the gather of psi and base; the
neutral filter against an unfiltered host-noise run of the same normals; invariance under launch length, point order and
rank count; one member; a twin experiment; resume; the CLI's "Ensemble": {"Filter": ...} block."""
import copy
import json

import numpy as np
import pytest

from helpers import digest, golden
from helpers import cli_params as _cli_params, run_cli_ranks as _run_ranks

pytestmark = pytest.mark.gpu
Q_ONE = 1 << 31


def _spread(psi0, N, seed=12, width=60.0):
    """[N][D]: the initial profile shifted by a per-member offset, uniform over +-width cm -- members whose water tables
    start in different bins, so that the weights differ and resampling has something to choose (the well's members
    otherwise share one bin for weeks)."""
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


def _q_numpy(w, obs, D, dz, sigma):
    """q_b of one point restated: l_b = -0.5 (dz (b - o) / sigma)^2, s = max over occupied bins, floor(2^31 exp(l - s))."""
    n = np.bincount(w, minlength=D)
    t = dz * (np.arange(D) - obs).astype(np.float64) / sigma
    ell = -0.5 * (t * t)
    s = ell[n > 0].max()
    q = np.where(n > 0, np.floor(2.0 ** 31 * np.exp(ell - s)), 0.0).astype(np.int64)
    return q, n, ell, s


@pytest.mark.parametrize("noise", ["philox", "numpy"])
@pytest.mark.parametrize("well, P, mpp", [
    (1, 1, 100), (1, 3, 100), (300, 1, 100), (300, 3, 100), (581, 1, 100), (581, 3, 100),   # D = 101, 300, 581 (split)
    (1, 1, 2500), (1, 2, 2500),                             # three tiles of the prefix scan per point
])
def test_ancestors_weights_and_gather_at_an_assimilation_row(well, P, mpp, noise):
    """Members per point are not a multiple of 64; the states start spread, so q is not uniform."""
    from hydromodel_amd.stepper import filter_ancestors_of
    N = P * mpp
    st, cols, forcing = _stepper(well, N, P, noise)
    D, dz, sigma = cols.dim_d, cols.dz, 1.5 * cols.dz
    obs = int(forcing.wtd_obs[48])
    assert obs >= 0 and forcing.refresh[48]
    try:
        st.set_filter(48, sigma, 11)
        kw = {"fresh_noise": _fresh(st, 1, 47, 1)} if noise == "numpy" else {}
        st.step_rows(1, 47, **kw)
        base_pre = st.get_noise_base() if noise == "numpy" else st.filter_base()
        kw = {"fresh_noise": _fresh(st, 48, 1, 2)} if noise == "numpy" else {}
        out = st.step_rows(48, 1, want_wtd=True, want_psi=True, **kw)
        anc, q, r = st.filter_ancestors(), st.filter_weights(), st.filter_draw()
        psi_post = st.get_state()
        base_post = st.get_noise_base() if noise == "numpy" else st.filter_base()
        table = st.filter_table()
    finally:
        st.close()
    w, forecast = out["wtd"][0], out["psi"][0]
    assert q.shape == (P, D) and r.shape == (P,) and anc.shape == (N,)
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        q_np, n, ell, s = _q_numpy(w[sl], obs, D, dz, sigma)
        assert np.all(np.abs(q[p] - q_np) <= 1) and np.all(q[p][n == 0] == 0)
        near = np.flatnonzero((n > 0) & (ell == s))
        assert near.size and np.all(q[p][near] == Q_ONE)
        assert np.unique(q[p][q[p] > 0]).size >= 2                 # weights that differ: a real choice
        qm = q[p][w[sl]]
        Q = int(qm.astype(object).sum())
        assert 0 <= int(r[p]) < Q
        assert np.array_equal(anc[sl], filter_ancestors_of(qm, int(r[p])) + p * mpp)
        assert table[p, 1, 0] == mpp and table[p, 1, 3] == np.unique(anc[sl]).size
        assert np.isnan(table[p, 2:, 1:]).all() and np.all(table[p, 2:, 0] == 0)
    assert not np.array_equal(anc, np.arange(N))                # not the identity
    assert np.array_equal(psi_post, forecast[anc])               # the analysis: each slot's ancestor, bit for bit
    assert np.array_equal(base_post, base_pre[anc])              # and its base noise vector (row 48 refreshes: no damping)


def test_weight_on_a_few_members_fills_long_slot_ranges():
    """Two points of 2 500 members: in each, 20 members start 40 cm apart from the other 2 480 (above them in point 0,
    below in point 1).  With sigma = dz / 20 only the nearest occupied bin keeps a weight, so in one of the two points the
    20 members share all 2 500 slots: ranges far longer than a wave, written by the whole wave."""
    from hydromodel_amd.stepper import EnsembleStepper, filter_ancestors_of
    _, cols, forcing = digest(1)
    mpp, P = 2500, 2
    psi0 = golden("g1_tables_1.npz")["initial_cond"]
    few = np.zeros(mpp, dtype=bool)
    few[7::125] = True
    off = np.concatenate([np.where(few, 20.0, -20.0), np.where(few, -20.0, 20.0)])
    st = EnsembleStepper([cols] * P, forcing, P * mpp)
    try:
        st.set_state(psi0[None, :] + off[:, None])
        st.set_noise_philox(3, 0)
        st.set_filter(48, cols.dz / 20.0, 5)
        st.step_rows(1, 47)
        base_pre = st.filter_base()
        out = st.step_rows(48, 1, want_wtd=True, want_psi=True)
        anc, q, r = st.filter_ancestors(), st.filter_weights(), st.filter_draw()
        psi_post, base_post = st.get_state(), st.filter_base()
    finally:
        st.close()
    w = out["wtd"][0]
    longest = 0
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        assert np.array_equal(anc[sl], filter_ancestors_of(q[p][w[sl]], int(r[p])) + p * mpp)
        longest = max(longest, int(np.bincount(anc[sl] - p * mpp, minlength=mpp).max()))
    assert longest > 64
    assert np.array_equal(psi_post, out["psi"][0][anc]) and np.array_equal(base_post, base_pre[anc])


def test_neutral_filter_is_the_identity_and_equals_a_host_noise_run_of_the_same_normals():
    from hydromodel_amd.stepper import filter_summary
    N, rows, seed = 64, 150, 5
    st, cols, forcing = _stepper(300, N, seed=seed)
    try:
        st.set_wtd_hist(48)
        st.set_filter(48, 1e30, 3)
        st.step_rows(1, rows)
        assert np.array_equal(st.filter_ancestors(), np.arange(N))
        got = (st.get_state(), st.moments(), st.wtd_hist_table())
        summary = filter_summary(st.filter_table()[0], 48, 1e30)
    finally:
        st.close()
    assert summary["rows"].tolist() == [48, 96, 144] and np.all(summary["survivors"] == N)
    assert np.all(summary["ess"] == N)
    ref, _, _ = _stepper(300, N, seed=seed)
    try:
        live = forcing.refresh.astype(bool) & (forcing.wtd_obs >= 0)
        draw = np.cumsum(live)
        base = np.stack([ref.philox_normals(m, 0) for m in range(N)])
        fresh = np.stack([np.stack([ref.philox_normals(m, int(draw[row])) for m in range(N)])
                          for row in range(1, rows + 1) if live[row]])
        ref.set_noise_host(base)
        ref.set_wtd_hist(48)
        ref.step_rows(1, rows, fresh_noise=fresh)
        want = (ref.get_state(), ref.moments(), ref.wtd_hist_table())
    finally:
        ref.close()
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _sweep_run(rows_per_launch, monkeypatch, fixed=False):
    if fixed:
        monkeypatch.setenv("HYDROCOL_POINT_ORDER", "fixed")
    else:
        monkeypatch.delenv("HYDROCOL_POINT_ORDER", raising=False)
    from hydromodel_amd.stepper import EnsembleStepper
    pts = [digest_point_like(n) for n in (1.6, 2.0, 2.4)]
    _, cols, forcing = pts[0]
    st = EnsembleStepper([c for _, c, _ in pts], forcing, 3 * 70)
    try:
        st.set_generic_exponents(True)
        st.set_state(_spread(golden("g1_tables_1.npz")["initial_cond"], 3 * 70))
        st.set_noise_philox(21, 0)
        st.set_rows_per_launch(rows_per_launch)
        st.set_wtd_hist(48)
        st.set_profile_stats(48)
        st.set_filter(48, 2.0 * cols.dz, 8)
        st.step_rows(1, 240)
        return [st.get_state(), st.filter_table(), st.moments(), st.wtd_hist_table(), st.profile_table(),
                st.filter_base()]
    finally:
        st.close()


def digest_point_like(n):
    """well 1 (D = 101) with the soil's n changed: a parameter point of a sweep"""
    from hydromodel_amd.digest import ColumnTables, ForcingDigest
    from hydromodel_amd.synthetic import default_parameters
    from helpers import WELLS, forcing_frame
    params = default_parameters()
    params["Soil_Properties"]["n"] = n
    cols = ColumnTables(params, WELLS[1])
    return params, cols, ForcingDigest(params, forcing_frame(1), cols)


def test_results_do_not_depend_on_launch_length_or_point_order(monkeypatch):
    runs = [_sweep_run(0, monkeypatch), _sweep_run(48, monkeypatch), _sweep_run(480, monkeypatch),
            _sweep_run(0, monkeypatch, fixed=True)]
    assert (runs[0][1][:, 1:6, 0] == 70).all()               # five assimilations per point
    assert np.all(runs[0][1][:, 1:6, 3] >= 1) and np.any(runs[0][1][:, 1:6, 3] < 70)   # resampling chose
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_one_member_increment_is_the_gaussian_log_density():
    st, cols, forcing = _stepper(1, 1)
    sigma = 7.0
    try:
        st.set_filter(48, sigma, 1)
        w = st.step_rows(1, 96, want_wtd=True)["wtd"][:, 0]
        assert st.filter_ancestors().tolist() == [0]
        t = st.filter_table()[0]
    finally:
        st.close()
    for row in (48, 96):
        d = cols.dz * abs(int(w[row - 1]) - int(forcing.wtd_obs[row]))
        want = -0.5 * (d / sigma) ** 2 - np.log(sigma) - 0.5 * np.log(2.0 * np.pi)
        assert t[row // 48, 0] == 1 and t[row // 48, 1] == 1.0 and t[row // 48, 3] == 1
        assert abs(t[row // 48, 2] - want) <= 1e-12 * max(1.0, abs(want))


def test_increment_and_ess_against_numpy():
    st, cols, forcing = _stepper(300, 256)
    sigma = 1.5 * cols.dz
    try:
        st.set_filter(48, sigma, 2)
        w = st.step_rows(1, 48, want_wtd=True)["wtd"][-1]
        q, t = st.filter_weights()[0], st.filter_table()[0, 1]
    finally:
        st.close()
    q_np, n, ell, s = _q_numpy(w, int(forcing.wtd_obs[48]), cols.dim_d, cols.dz, sigma)
    W = 0.0
    for b in np.flatnonzero(n):
        W += float(n[b]) * np.exp(ell[b] - s)
    inc = s + np.log(W / n.sum()) - np.log(sigma) - 0.5 * np.log(2.0 * np.pi)
    assert abs(t[2] - inc) <= 1e-13 * max(1.0, abs(inc))
    A = sum(int(n[b]) * int(q[b]) for b in range(q.size))
    B = sum(int(n[b]) * int(q[b]) ** 2 for b in range(q.size))
    from fractions import Fraction
    assert abs(t[1] - float(Fraction(A * A, B))) <= 4.5e-16 * float(Fraction(A * A, B))      # within 2 ulp


def test_twin_experiment_filter_lowers_the_crps(capsys):
    """A twin experiment with an uncertain initial water table: every member starts from the initial profile shifted by its
    own offset (uniform over +-60 cm), the "truth" is one more column, shifted by +35 cm and driven by another seed, and its
    water table is the well.  The filtered ensemble follows it better than the open one."""
    from hydromodel_amd.stepper import wtd_distribution
    rows, N = 10 * 48, 256
    psi0 = golden("g1_tables_1.npz")["initial_cond"]
    shifts = np.random.default_rng(12).uniform(-60.0, 60.0, size=N)
    truth, cols, forcing = _stepper(1, 1, seed=999)
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
    crps = {}
    for tag, filt in (("open", 0), ("filtered", 48)):
        st, _, _ = _stepper(1, N, seed=4, forcing=twin)
        try:
            st.set_state(psi0[None, :] + shifts[:, None])
            st.set_wtd_hist(48)
            if filt:
                st.set_filter(filt, 2.0 * cols.dz, 17)
            st.step_rows(1, rows)
            hist = st.wtd_hist_table()[0]
        finally:
            st.close()
        d = wtd_distribution(hist, obs, (0.5,), cols.dz, cols.z, 0, 48)
        crps[tag] = float(d["crps_mean_cm"])
    with capsys.disabled():
        print(f"\n twin experiment, {N} members, {rows // 48} days: mean CRPS open {crps['open']:.4f} cm, "
              f"filtered {crps['filtered']:.4f} cm")
    assert crps["filtered"] < crps["open"]


def test_dump_and_restore_continue_a_filtered_run_bit_for_bit(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(1)
    psi0 = _spread(golden("g1_tables_1.npz")["initial_cond"], 96)
    kw = dict(seed=6, psi0=psi0, wtd_hist_stride=48, filter_stride=48, filter_sigma_cm=2.0 * cols.dz)
    whole = EnsembleSimulation(cols, forcing, 96, **kw)
    try:
        whole.advance(100)
        path = whole.dump(tmp_path / "ck.h5")
        whole.advance(140)
        want = [whole.stepper.get_state(), whole.filter_table(), whole.moments(), whole.wtd_hist_table(),
                whole.stepper.filter_base()]
        summary = whole.filter_summary()
    finally:
        whole.close()
    back = EnsembleSimulation.restore(path, cols, forcing)
    try:
        assert back.next_row == 101 and back.filter_stride == 48
        back.advance(140)
        got = [back.stepper.get_state(), back.filter_table(), back.moments(), back.wtd_hist_table(),
               back.stepper.filter_base()]
    finally:
        back.close()
    for a, b in zip(want, got):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert summary["rows"].tolist() == [48, 96, 144, 192, 240] and np.isfinite(summary["loglik"])
    assert np.any(summary["survivors"][:2] < 96)        # resampled before the dump: the base vectors were carried over


def _point_handle(ns, ids, mpp, psi_all, seed):
    """The handle a rank runs for the sweep points ``ids`` (soil n of each in ``ns``): global member ids point-major,
    each point keyed by its first global member, states taken from the whole sweep's ``psi_all``."""
    from hydromodel_amd.stepper import EnsembleStepper
    pts = [digest_point_like(n) for n in ns]
    st = EnsembleStepper([c for _, c, _ in pts], pts[0][2], len(ids) * mpp)
    st.set_generic_exponents(True)
    st.set_state(np.concatenate([psi_all[k * mpp:(k + 1) * mpp] for k in ids]))
    st.set_noise_philox(seed, ids[0] * mpp)
    if len(ids) > 1:
        st.set_point_member_bases(np.array(ids, dtype=np.int64) * mpp)
    st.set_filter(24, 2.0 * st.cols.dz, 9)
    st.step_rows(1, 150)
    return st


def test_points_split_over_handles_resample_as_in_one_handle():
    """What two ranks of a sweep run -- points {0, 2} in one handle, point 1 in another -- against all three points in one
    handle, from spread states: states, base vectors, filter tables and moments per point, bit for bit."""
    ns, mpp, seed = (1.6, 2.0, 2.4), 60, 31
    psi_all = _spread(golden("g1_tables_1.npz")["initial_cond"], 3 * mpp, seed=4)
    parts = {}
    for ids in ([0, 1, 2], [0, 2], [1]):
        st = _point_handle([ns[k] for k in ids], ids, mpp, psi_all, seed)
        try:
            parts[tuple(ids)] = dict(psi=st.get_state().reshape(len(ids), mpp, -1),
                                     base=st.filter_base().reshape(len(ids), mpp, -1), table=st.filter_table(),
                                     moments=np.asarray(st.moments()).reshape(len(ids), 3, -1))
        finally:
            st.close()
    whole = parts[(0, 1, 2)]
    assert np.any(whole["table"][:, 1:7, 3] < mpp)
    for ids in ((0, 2), (1,)):
        for j, k in enumerate(ids):
            for key in ("psi", "base", "table", "moments"):
                a, b = whole[key][k], parts[ids][key][j]
                assert a.tobytes() == b.tobytes(), (ids, k, key)


FILTER_KEYS = {"filter_rows", "filter_count", "filter_ess", "filter_loglik_rows", "filter_survivors", "filter_loglik",
               "filter_sigma_cm"}


def test_cli_filter_block_writes_the_datasets(tmp_path, monkeypatch, capsys):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    params = _cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    pts = [{"Soil_Properties": {"n": 1.6}}, {"Soil_Properties": {"n": 2.4}}]
    files, logs = {}, {}
    for tag, extra in (("plain", {}), ("ens", {"Filter": {"Stride": 24, "Sigma_cm": 10.0}}),
                       ("sweep", {"Points": pts, "Filter": {"Sigma_cm": 10.0, "Seed": 4}})):
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 64, "Seed": 3, "Days": 2, **extra}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = loadResults(tmp_path / f"Run_{tag}_ensemble.h5")
        logs[tag] = capsys.readouterr().out
    plain, ens, sweep = files["plain"], files["ens"], files["sweep"]
    assert "filter log-likelihood" not in logs["plain"] and not any(k.startswith("filter") for k in plain)
    assert set(ens) - set(plain) == FILTER_KEYS
    assert ens["filter_rows"].tolist() == [24, 48, 72, 96]
    for k in ("filter_count", "filter_ess", "filter_loglik_rows", "filter_survivors"):
        assert ens[k].shape == (4,), k
    assert ens["filter_count"].tolist() == [64] * 4 and float(ens["filter_sigma_cm"]) == 10.0
    assert np.isclose(float(ens["filter_loglik"]), ens["filter_loglik_rows"].sum(), rtol=1e-12)
    assert f"[Ensemble x64] filter log-likelihood = {float(ens['filter_loglik']):.3f} over 4 rows" in logs["ens"]
    assert sweep["filter_rows"].tolist() == [48, 96]
    for k in ("filter_count", "filter_ess", "filter_loglik_rows", "filter_survivors"):
        assert sweep[k].shape == (2, 2), k
    assert sweep["filter_loglik"].shape == (2,) and np.isfinite(sweep["filter_loglik"]).all()
    assert "[Sweep 2 points x64] filter log-likelihood: best point " in logs["sweep"]


def test_a_filtered_sweep_on_two_ranks_writes_what_one_rank_writes(tmp_path):
    params = _cli_params(tmp_path)
    params["Ensemble"] = {"Members": 40, "Seed": 5, "Days": 2, "Distribution": {"Stride": 48},
                          "Points": [{"Soil_Properties": {"n": n}} for n in (1.6, 2.0, 2.4)],
                          "Filter": {"Stride": 24, "Sigma_cm": 8.0}}
    one, log1 = _run_ranks(tmp_path, "one", params, 1)
    two, log2 = _run_ranks(tmp_path, "two", params, 2)
    for k in sorted(FILTER_KEYS) + ["moments", "wtd_hist"]:
        a, b = np.asarray(one[k]), np.asarray(two[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    line = [s for s in log1.splitlines() if "filter log-likelihood" in s]
    assert len(line) == 1 and line == [s for s in log2.splitlines() if "filter log-likelihood" in s]
