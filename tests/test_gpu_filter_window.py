"""The well's record inside the window of the particle filter on the GPU (include/hydrocol.h hc_set_filter_window): off means
off; the captured indices against wtd_out; l_m against its NumPy restatement bit for bit, q_m against NumPy, the ancestry as
an integer function of the exported q_m, the gather; the increment, the ESS and the window's diagnostics in the documented
summation order; absent lagged rows; invariance under launch length, point order and the dealing of a sweep's points to
handles; tempering; period totals; resume between a capture and its assimilation; the CLI's "Filter": {"Window_Offsets":
...} key on one and two ranks; the refusals.  Every case calls the window's entry points, so none passes without them."""
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
STRIDE, OFFSETS = 48, (12, 24, 36)
LAG_ROWS = [STRIDE - o for o in OFFSETS]          # 36, 24, 12: slot j holds row 48 - OFFSETS[j]
NODES = [6, 45]                 # 30 cm (above every well's water table: unsaturated) and 225 cm
VALUES = [0.24, 0.36]
SIGMAS = np.array([0.05, 0.08])


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _spread(psi0, N, seed=12, width=60.0):
    """[N][D]: the initial profile shifted by a per-member offset, uniform over +-width cm -- members whose water tables
    start in different bins, so that the weights differ and resampling has something to choose."""
    return np.asarray(psi0)[None, :] + np.random.default_rng(seed).uniform(-width, width, size=N)[:, None]


def _point_like(n, well=1):
    from hydromodel_amd.digest import ColumnTables, ForcingDigest
    from hydromodel_amd.synthetic import default_parameters
    params = default_parameters()
    params["Soil_Properties"]["n"] = n
    cols = ColumnTables(params, WELLS[well])
    return params, cols, ForcingDigest(params, forcing_frame(1), cols)


def _stepper(well, N, P=1, noise="philox", seed=7):
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(well)
    assert (np.asarray(forcing.wtd_obs[1:97]) >= 0).all()             # an observation on every row of 1 ... 96
    st = EnsembleStepper([cols] * P if P > 1 else cols, forcing, N)
    st.set_state(_spread(golden(f"g1_tables_{well}.npz")["initial_cond"], N))
    if noise == "numpy":
        st.set_noise_host(np.random.default_rng(seed).standard_normal((N, cols.dim_d)))
    else:
        st.set_noise_philox(seed, 0)
    return st, cols, forcing


def _fresh(st, row_begin, n_rows, seed):
    return np.random.default_rng(seed).standard_normal((st.n_refresh(row_begin, n_rows), st.N, st.D))


def _record(T, row_values, rows=(48,)):
    v = np.full((T, len(row_values)), np.nan)
    for r in rows:
        v[r] = row_values
    return v


def _unobserve(st, forcing, row):
    """hc_set_forcing_row: the row keeps its forcing and loses its observation"""
    from hydromodel_amd import _lib as L
    L.check(st.lib.hc_set_forcing_row(st.h, row, float(forcing.precip[row]), float(forcing.atm[row]),
                                      int(forcing.daylight[row]), -1))


def _q_numpy(ell, wmax, D):
    counted = (wmax < D) & np.isfinite(ell)
    s = ell[counted].max()
    e = np.where(counted, np.exp(np.where(counted, ell - s, 0.0)), 0.0)
    return np.floor(2.0 ** 31 * e).astype(np.int64), e, s, counted


def _row_48(well, P, mpp, noise="philox", ms=0, offsets=OFFSETS, unobserved=(), ess_floor=0.0, sigma_dz=1.5, window=True,
            seed=11):
    """One handle stepped to the assimilation at row 48 with the window (and ``ms`` sensors): everything the checks read."""
    N = P * mpp
    st, cols, forcing = _stepper(well, N, P, noise)
    sigma = sigma_dz * cols.dz
    try:
        st.set_filter(STRIDE, sigma, seed)
        if ms:
            st.set_filter_soil_moisture(NODES[:ms], _record(st.T, VALUES[:ms]), SIGMAS[:ms])
        if ess_floor:
            st.set_filter_tempering(ess_floor)
        if window:
            st.set_filter_window(offsets)
        for r in unobserved:
            _unobserve(st, forcing, r)
        kw = {"fresh_noise": _fresh(st, 1, 47, 1)} if noise == "numpy" else {}
        before = st.step_rows(1, 47, want_wtd=True, **kw)
        cap = st.filter_window_capture() if window and offsets else None
        base_pre = st.get_noise_base() if noise == "numpy" else st.filter_base()
        kw = {"fresh_noise": _fresh(st, 48, 1, 2)} if noise == "numpy" else {}
        out = st.step_rows(48, 1, want_wtd=True, want_psi=True, **kw)
        mw = len(st.filter_window_slots()) if window else 0
        got = dict(anc=st.filter_ancestors(), r=st.filter_draw(), q_bins=st.filter_weights(), table=st.filter_table(),
                   psi_post=st.get_state(), base_post=st.get_noise_base() if noise == "numpy" else st.filter_base(),
                   base_pre=base_pre, w=out["wtd"][0].astype(np.int64), forecast=out["psi"][0], sigma=sigma, cols=cols,
                   obs=int(forcing.wtd_obs[48]), wtd_rows=before["wtd"].astype(np.int64), cap=cap, mw=mw,
                   wtd_obs=np.asarray(forcing.wtd_obs), counters=st.counters(), launches=before["launches"])
        if window and offsets:
            got.update(slots=st.filter_window_slots(), wint=st.filter_window_table(), qm=st.filter_member_weights(),
                       cap_after=st.filter_window_capture())
        if ms:
            got.update(smt=st.filter_sm_table(), width=st.filter_sm_width())
        if mw or (ms and st.filter_sm_width()):
            got["ell"] = st.filter_loglik()
            got["theta"] = st.filter_sm_theta() if ms else np.zeros((N, 0))
        if ess_floor:
            got.update(ttable=st.filter_temper_table(), trials=st.filter_temper_trials())
    finally:
        st.close()
    return got


# ---- 1. off means off --------------------------------------------------------------------------------------------------
def _run_96(window, ms=0):
    st, cols, forcing = _stepper(300, 200)
    try:
        st.set_filter(STRIDE, 1.5 * cols.dz, 3)
        if ms:
            st.set_filter_soil_moisture(NODES, _record(st.T, VALUES, (48, 96)), SIGMAS)
        if window is not None:
            st.set_filter_window(window)
        out = st.step_rows(1, 96)
        return dict(psi=st.get_state(), base=st.filter_base(), table=st.filter_table(), q=st.filter_weights(),
                    r=st.filter_draw(), anc=st.filter_ancestors(), counters=np.array(list(st.counters().values())),
                    launches=np.asarray(out["launches"]))
    finally:
        st.close()


@pytest.mark.parametrize("ms", [0, 2])
def test_an_empty_offset_list_is_the_run_without_the_call(ms):
    plain, empty = _run_96(None, ms), _run_96((), ms)
    for k in plain:
        assert _same(plain[k], empty[k]), k
    windowed = _run_96(OFFSETS, ms)
    assert windowed["launches"] > plain["launches"]                    # a launch ends on every lagged row
    assert not _same(windowed["anc"], plain["anc"])


# ---- 2. weights against NumPy ------------------------------------------------------------------------------------------
def _check_row_48(g, P, mpp, ms):
    from hydromodel_amd.stepper import filter_ancestors_of, filter_member_loglik
    cols, N = g["cols"], P * mpp
    D, dz = cols.dim_d, cols.dz
    b, rows = g["cap"]
    assert rows.tolist() == LAG_ROWS and b.dtype == np.int32 and b.shape == (3, N)
    for j, r in enumerate(LAG_ROWS):
        assert np.array_equal(b[j], g["wtd_rows"][r - 1])                    # the index wtd_out returns for that row
    assert g["cap_after"][1].tolist() == [-1, -1, -1] and not g["cap_after"][0].any()    # the assimilation emptied it
    assert g["slots"].tolist() == [0, 1, 2] and g["ell"].shape == (N,) and g["qm"].shape == (N,)
    lag_obs = [int(g["wtd_obs"][r]) for r in LAG_ROWS]
    ell = filter_member_loglik(g["w"], g["theta"], g["obs"], VALUES[:ms], dz, g["sigma"], SIGMAS[:ms], b.T, lag_obs)
    assert g["ell"].tobytes() == ell.tobytes()                               # the same IEEE operations in the same order
    well_only = filter_member_loglik(g["w"], g["theta"], g["obs"], VALUES[:ms], dz, g["sigma"], SIGMAS[:ms])
    assert not np.array_equal(ell, well_only)
    assert not g["q_bins"].any()                                             # the bin table is zeroed on a per-member row
    wmax = np.maximum(g["w"], b.max(axis=0))
    lag_matters = False
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        w, qm = g["w"][sl], g["qm"][sl]
        q_np, _, s, counted = _q_numpy(g["ell"][sl], wmax[sl], D)
        assert counted.all()
        assert np.all(np.abs(qm - q_np) <= 1)                                # the device's exp against NumPy's
        assert np.all(qm[g["ell"][sl] == s] == Q_ONE)
        # members that share the index of row 48 (and, without sensors, everything else of the row) and differ on a
        # lagged row: the inputs hold such pairs with weights well above the floor's grain, and their q_m differ
        if ms == 0:
            for bin_ in np.unique(w):
                m = np.flatnonzero((w == bin_) & (qm > 1 << 16))
                lags = {tuple(b[:, sl][:, i]) for i in m}
                if len(lags) >= 2:
                    by_lag = {}
                    for i in m:
                        by_lag.setdefault(float(g["ell"][sl][i]), set()).add(int(qm[i]))
                    assert all(len(v) == 1 for v in by_lag.values())        # q_m is a function of l_m within the point
                    if len(by_lag) >= 2:
                        assert len({min(v) for v in by_lag.values()}) == len(by_lag)
                        lag_matters = True
        Q = int(qm.astype(object).sum())
        assert 0 <= int(g["r"][p]) < Q
        assert np.array_equal(g["anc"][sl], filter_ancestors_of(qm, int(g["r"][p])) + p * mpp)
        t = g["table"][p]
        assert t[1, 0] == mpp and t[1, 3] == np.unique(g["anc"][sl]).size
        wt = g["wint"][p]
        assert wt[1, :, 0].tolist() == [1.0] * 3 and wt[1, :, 1].tolist() == [dz * o for o in lag_obs]
        assert np.isfinite(wt[1]).all() and np.isnan(wt[0]).all() and np.isnan(wt[2:]).all()
    assert lag_matters or ms
    assert not np.array_equal(g["anc"], np.arange(N))
    assert np.array_equal(g["psi_post"], g["forecast"][g["anc"]])            # each slot's ancestor, bit for bit
    assert np.array_equal(g["base_post"], g["base_pre"][g["anc"]])


@pytest.mark.parametrize("ms", [0, 2])
@pytest.mark.parametrize("noise", ["philox", "numpy"])
@pytest.mark.parametrize("well, P, mpp", [
    (1, 1, 100), (1, 3, 100), (300, 1, 100), (300, 3, 100), (581, 1, 100),    # D = 101, 300, 581 (the split column)
    (1, 1, 2500),                                                            # three tiles of the prefix scan
])
def test_member_weights_ancestry_and_gather_at_a_windowed_row(well, P, mpp, noise, ms):
    """Members per point are not a multiple of 64; the states start spread, so the members' water tables pass the lagged
    rows in different cells."""
    _check_row_48(_row_48(well, P, mpp, noise, ms), P, mpp, ms)


# ---- 3. increment, ESS and diagnostics ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ms", [0, 2])
def test_increment_ess_and_window_diagnostics_against_numpy(ms):
    from hydromodel_amd.stepper import filter_tile_sum
    N = 256
    got = _row_48(300, 1, N, ms=ms, seed=3)
    cols, t, wt = got["cols"], got["table"][0, 1], got["wint"][0, 1]
    b = got["cap"][0]
    q_np, e, s, counted = _q_numpy(got["ell"], np.maximum(got["w"], b.max(axis=0)), cols.dim_d)
    n = int(counted.sum())
    W = filter_tile_sum(e)                                                     # the documented order
    inc = s + np.log(W / n) - np.log(got["sigma"])
    for sg in SIGMAS[:ms]:
        inc -= np.log(sg)
    for _ in range(3):
        inc -= np.log(got["sigma"])
    inc -= 0.5 * float(1 + ms + 3) * np.log(2.0 * np.pi)
    bound = (N + 16 + 3) * 2.0 ** -53          # N_p positive terms, the ulps of exp and log, m_w more log terms
    print(f"\n increment {t[2]!r} against {inc!r}: {abs(t[2] - inc):.3e} (bound {bound * max(1.0, abs(inc)):.3e})")
    assert t[0] == n == N and abs(t[2] - inc) <= bound * max(1.0, abs(inc))
    qm = [int(v) for v in got["qm"]]
    ess = Fraction(sum(qm) ** 2, sum(v * v for v in qm))
    assert abs(t[1] - float(ess)) <= 4.5e-16 * float(ess)                      # within 2 ulp
    for j in range(3):
        x = cols.dz * b[j].astype(np.float64)
        mean = filter_tile_sum(x) / N
        std = np.sqrt(filter_tile_sum((x - mean) * (x - mean)) / (N - 1))
        exact_mean = float(np.mean(x.astype(np.longdouble)))
        exact_std = float(np.sqrt(np.sum((x.astype(np.longdouble) - exact_mean) ** 2) / (N - 1)))
        assert wt[j, 0] == 1.0 and wt[j, 1] == cols.dz * float(got["wtd_obs"][LAG_ROWS[j]])
        assert wt[j, 2] == mean and abs(mean - exact_mean) <= bound * max(1.0, abs(exact_mean))
        assert abs(wt[j, 3] - std) <= bound * max(1.0, std) and abs(wt[j, 3] - exact_std) <= bound * max(1.0, exact_std)
    assert t[3] == np.unique(got["anc"]).size


@pytest.mark.parametrize("ms", [0, 2])
def test_one_member_increment_is_the_joint_gaussian_log_density(ms):
    got = _row_48(300, 1, 1, ms=ms)
    cols, t, wt = got["cols"], got["table"][0, 1], got["wint"][0, 1]
    sigma, b = got["sigma"], got["cap"][0]
    want = -0.5 * (cols.dz * (int(got["w"][0]) - got["obs"]) / sigma) ** 2 - np.log(sigma) - 0.5 * np.log(2.0 * np.pi)
    for i in range(ms):
        want += -0.5 * ((got["theta"][0, i] - VALUES[i]) / SIGMAS[i]) ** 2 - np.log(SIGMAS[i]) - 0.5 * np.log(2.0 * np.pi)
    for j, r in enumerate(LAG_ROWS):
        want += -0.5 * (cols.dz * (int(b[j, 0]) - int(got["wtd_obs"][r])) / sigma) ** 2 - np.log(sigma) \
            - 0.5 * np.log(2.0 * np.pi)
    assert t[0] == 1 and t[1] == 1.0 and t[3] == 1 and got["anc"].tolist() == [0] and got["qm"].tolist() == [Q_ONE]
    assert abs(t[2] - want) <= 1e-12 * max(1.0, abs(want))
    assert wt[:, 3].tolist() == [0.0] * 3 and wt[:, 2].tolist() == [cols.dz * float(v) for v in b[:, 0]]


# ---- 4. an absent lagged row -------------------------------------------------------------------------------------------
def test_a_lagged_row_that_lost_its_observation_is_absent():
    from hydromodel_amd.stepper import filter_member_loglik
    got = _row_48(300, 1, 100, unobserved=(24,))
    cols = got["cols"]
    b, rows = got["cap"]
    assert rows.tolist() == [36, -1, 12] and got["mw"] == 2 and got["slots"].tolist() == [0, 2]
    wt = got["wint"][0, 1]
    assert wt[:, 0].tolist() == [1.0, 0.0, 1.0] and np.isnan(wt[1, 1:]).all() and np.isfinite(wt[[0, 2]]).all()
    lag_obs = [int(got["wtd_obs"][36]), int(got["wtd_obs"][12])]
    ell = filter_member_loglik(got["w"], np.zeros((100, 0)), got["obs"], [], cols.dz, got["sigma"], [], b[[0, 2]].T, lag_obs)
    assert got["ell"].tobytes() == ell.tobytes()


def test_a_row_whose_lagged_rows_all_lost_theirs_takes_the_bin_path():
    got = _row_48(300, 1, 100, unobserved=(12, 24, 36))
    plain = _row_48(300, 1, 100, unobserved=(12, 24, 36), window=False)
    assert got["mw"] == 0 and got["slots"].size == 0 and got["cap"][1].tolist() == [-1, -1, -1]
    assert got["q_bins"].any() and np.isnan(got["wint"]).all()
    assert np.array_equal(got["qm"], got["q_bins"][0][got["w"]])             # the bin path's q of each member's bin
    for k in ("q_bins", "anc", "r", "table", "psi_post", "base_post", "w", "forecast"):
        assert _same(got[k], plain[k]), k
    assert got["launches"] == plain["launches"]                              # and no launch was cut for them


# ---- 5. invariance -----------------------------------------------------------------------------------------------------
SWEEP_N = (1.6, 1.8, 2.1, 2.4)
SWEEP_MPP, SWEEP_ROWS, SWEEP_STRIDE, SWEEP_OFFSETS = 70, 72, 24, (6, 12, 18)


def _sweep_handle(ids, psi_all, rows_per_launch=0):
    """The handle that runs the sweep points ``ids``: global member ids point-major, each point keyed by its first global
    member, states from the whole sweep's ``psi_all``; three windowed assimilations, two sensors on the second."""
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
        st.set_filter_soil_moisture(NODES, _record(st.T, VALUES, (48,)), SIGMAS)
        st.set_filter_window(SWEEP_OFFSETS)
        st.step_rows(1, SWEEP_ROWS)
        n = len(ids)
        return dict(psi=st.get_state().reshape(n, SWEEP_MPP, -1), table=st.filter_table(), smt=st.filter_sm_table(),
                    wint=st.filter_window_table(), moments=np.asarray(st.moments()).reshape(n, 3, -1),
                    base=st.filter_base().reshape(n, SWEEP_MPP, -1))
    finally:
        st.close()


def test_results_do_not_depend_on_launch_length_point_order_or_the_dealing_of_points(monkeypatch):
    psi_all = _spread(golden("g1_tables_1.npz")["initial_cond"], 4 * SWEEP_MPP, seed=4)
    everyone = list(range(4))
    monkeypatch.delenv("HYDROCOL_POINT_ORDER", raising=False)
    whole = _sweep_handle(everyone, psi_all)
    assert (whole["table"][:, 1:4, 0] == SWEEP_MPP).all() and np.isfinite(whole["wint"][:, 1:4]).all()
    assert np.isfinite(whole["smt"][:, 2]).all() and np.any(whole["table"][:, 1:4, 3] < SWEEP_MPP)
    others = [_sweep_handle(everyone, psi_all, 1), _sweep_handle(everyone, psi_all, 7)]
    monkeypatch.setenv("HYDROCOL_POINT_ORDER", "fixed")
    others.append(_sweep_handle(everyone, psi_all))
    monkeypatch.delenv("HYDROCOL_POINT_ORDER", raising=False)
    for other in others:
        for k in whole:
            assert _same(whole[k], other[k]), k
    for ids in ([0, 2], [1, 3]):                               # what two ranks of the sweep run
        part = _sweep_handle(ids, psi_all)
        for j, k in enumerate(ids):
            for key in whole:
                assert whole[key][k].tobytes() == part[key][j].tobytes(), (ids, k, key)


# ---- 6. tempering ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ms", [0, 2])
def test_tempering_on_a_windowed_row_is_the_restatements_bisection(ms):
    from hydromodel_amd.stepper import filter_ancestors_of, filter_temper_of, filter_temper_target
    mpp = 1000
    got = _row_48(300, 1, mpp, ms=ms, ess_floor=0.5, sigma_dz=0.5)
    twin = _row_48(300, 1, mpp, ms=ms, sigma_dz=0.5)
    assert _same(got["ell"], twin["ell"]) and _same(got["table"][:, :, :3], twin["table"][:, :, :3])
    assert _same(got["wint"], twin["wint"])
    D = got["cols"].dim_d
    counted = (np.maximum(got["w"], got["cap"][0].max(axis=0)) < D) & np.isfinite(got["ell"])
    k, trials, q_np = filter_temper_of(got["ell"], counted, 0.5)
    tt = got["ttable"][0, 1]
    dev = [int(v) for v in got["trials"][0][:, 0] if v >= 0]
    assert k < 1024 and tt[0] == k / 1024 and tt[2] == filter_temper_target(0.5, int(counted.sum()))
    assert dev == [v[0] for v in trials] and tt[3] == len(trials) == 11
    assert np.all(np.abs(got["qm"] - q_np) <= 1) and got["qm"].max() == Q_ONE
    assert np.array_equal(got["anc"], filter_ancestors_of(got["qm"], int(got["r"][0])))
    assert not _same(got["anc"], twin["anc"])                                 # tempering changed who survives
    assert _same(got["psi_post"], got["forecast"][got["anc"]])


# ---- 7. period totals --------------------------------------------------------------------------------------------------
def test_period_totals_follow_the_windowed_ancestry():
    from hydromodel_amd.stepper import period_totals_of
    from test_gpu_period_totals import _handle, _setup, _tables
    ends = [72, 96]

    def run(feature):
        st = _handle(200, 67)
        try:
            st.set_filter(48, 8.0, seed=11)
            st.set_filter_window(OFFSETS)
            if feature:
                st.set_period_totals(ends, feature[0], 32, feature[1])
            a = st.step_rows(1, 48, want_diag=True, want_wtd=True)
            anc, mw = st.filter_ancestors(), len(st.filter_window_slots())
            b = st.step_rows(49, 48, want_diag=True, want_wtd=True)
            diag, wtd = np.concatenate([a["diag"], b["diag"]]), np.concatenate([a["wtd"], b["wtd"]])
            return diag, wtd, anc, mw, st.get_state(), (_tables(st) if feature else None)
        finally:
            st.close()

    diag, wtd, anc, mw, psi, _ = run(None)
    thr, fexp = _setup(diag, wtd)
    fexp = [e + 1 for e in fexp]
    assert mw == 3 and len(set(anc.tolist())) < 67 and not np.array_equal(anc, np.arange(67))
    got_diag, got_wtd, got_anc, _, got_psi, (table, hf, hw) = run((thr, fexp))
    assert _same(got_diag, diag) and _same(got_wtd, wtd) and _same(got_anc, anc) and _same(got_psi, psi)
    forcing = digest(200)[2]
    want = period_totals_of(diag, wtd, forcing.wtd_obs, ends, thr, 32, fexp, ancestors={48: anc}, D=200)
    assert _same(table, want["table"]) and _same(hf[0], want["hist_flux"]) and _same(hw[0], want["hist_wtd"])


# ---- 10. refusals, and what turns the window off -----------------------------------------------------------------------
def test_refusals_and_what_turns_the_window_off():
    from hydromodel_amd._lib import HcError, check, iptr
    st, cols, _ = _stepper(1, 64)
    rec = _record(st.T, VALUES)

    def raw(offsets):
        a = np.ascontiguousarray(offsets, dtype=np.int32)
        return check(st.lib.hc_set_filter_window(st.h, a.size, iptr(a)))

    try:
        with pytest.raises(HcError, match="the particle filter is off"):
            raw([12])
        st.set_enkf(48, 5.0, 0.0, 1)
        with pytest.raises(HcError, match="the EnKF is on"):
            raw([12])
        st.set_enkf(0)
        st.set_filter(48, 5.0, 1)
        for bad, what in (([0], r"offset 0 outside \[1, 48\)"), ([48], r"offset 48 outside \[1, 48\)"),
                          ([12, 12], "offset 12 twice"), (list(range(1, 10)), "9 offsets, at most 8")):
            with pytest.raises(HcError, match=what):
                raw(bad)
        with pytest.raises(ValueError, match="Filter Window_Offsets"):
            st.set_filter_window([48])
        assert st.filter_window_n == 0
        st.set_filter_soil_moisture(NODES, rec, SIGMAS)
        with pytest.raises(HcError, match="7 offsets and 2 sensors, at most 8 together"):
            raw(list(range(1, 8)))
        st.set_filter_soil_moisture(None)
        st.set_filter_window(range_ := [1, 2, 3, 4, 5, 6, 7])
        assert st.filter_window_offsets == tuple(range_)
        with pytest.raises(HcError, match="2 sensors and 7 window offsets, at most 8 together"):
            st.set_filter_soil_moisture(NODES, rec, SIGMAS)              # ... likewise when the sensors come second
        st.set_filter_window([36, 12, 24])
        assert st.filter_window_offsets == OFFSETS                       # kept in ascending order
        assert st.filter_window_table().shape == (1, (st.T - 1) // 48 + 1, 3, 4) and np.isnan(st.filter_window_table()).all()
        assert st.filter_window_capture()[1].tolist() == [-1, -1, -1]
        with pytest.raises(HcError, match="gathers the water-table indices of the assimilation row only"):
            st.set_filter_shard([0, 64], 0, None)
        assert st.get_filter_shard() == (0, 0, 0)
        st.set_filter_window(())                                         # the window removed: sharding is accepted again,
        st.set_filter_shard([0, 64], 0, None)
        with pytest.raises(HcError, match="gathers the water-table indices of the assimilation row only"):
            st.set_filter_window(OFFSETS)                                # ... and refuses the window in its turn
        assert st.filter_window_n == 0
        st.set_filter(48, 5.0, 1)                                        # hc_set_filter removes sharding and window alike
        st.set_filter_window(OFFSETS)
        st.set_filter(48, 5.0, 1)
        assert st.filter_window_n == 0
        with pytest.raises(HcError, match="no window offsets"):
            st.filter_window_capture()
        st.set_filter_window(OFFSETS)
        st.set_noise_philox(9, 0)                                        # a new noise source turns the filter off
        assert st.filter_stride == 0 and st.filter_window_n == 0
        with pytest.raises(HcError, match="the particle filter is off"):
            raw([12])
    finally:
        st.close()


def _filter_with_record_and_window():
    """One point, 64 members of well 1, the filter on with the two-sensor record and the offsets (12, 24, 36); no row stepped."""
    st, _, _ = _stepper(1, 64)
    st.set_filter(48, 5.0, 1)
    st.set_filter_soil_moisture(NODES, _record(st.T, VALUES), SIGMAS)
    st.set_filter_window(OFFSETS)
    return st


def test_the_enkfs_off_calls_leave_the_filters_record_and_window_alone():
    from hydromodel_amd._lib import check
    st = _filter_with_record_and_window()
    try:
        check(st.lib.hc_set_enkf_soil_moisture(st.h, 0, None, None, None))
        check(st.lib.hc_set_enkf_window(st.h, 0, None))
        n_arow = (st.T - 1) // 48 + 1
        sm, wt = st.filter_sm_table(), st.filter_window_table()
        assert sm.shape == (1, n_arow, 2, 6) and np.isnan(sm).all()
        assert wt.shape == (1, n_arow, 3, 4) and np.isnan(wt).all()
        assert st.filter_window_capture()[1].tolist() == [-1, -1, -1]
    finally:
        st.close()


def test_nothing_of_the_filters_carries_over_to_the_enkf():
    from hydromodel_amd._lib import HcError, check, dptr
    st = _filter_with_record_and_window()
    try:
        st.set_filter(0)
        st.set_enkf(48, 5.0, 0.0, 1)
        assert st.enkf_sm_width() == 0
        with pytest.raises(HcError, match="no soil-moisture record"):
            check(st.lib.hc_get_enkf_sm_stats(st.h, dptr(np.zeros(1)), -1))
        with pytest.raises(HcError, match="no window offsets"):
            st.enkf_window_capture()
    finally:
        st.close()


# ---- 8. checkpoint -----------------------------------------------------------------------------------------------------
def test_dump_between_a_capture_and_its_assimilation_resumes_bit_for_bit(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(1)
    psi0 = _spread(golden("g1_tables_1.npz")["initial_cond"], 96)
    kw = dict(seed=6, psi0=psi0, filter_stride=STRIDE, filter_sigma_cm=2.0 * cols.dz, filter_window_offsets=OFFSETS)

    def state(sim):
        return [sim.stepper.get_state(), sim.filter_table(), sim.filter_window_table(), sim.moments(),
                sim.stepper.filter_base()]

    whole = EnsembleSimulation(cols, forcing, 96, **kw)
    try:
        whole.advance(40)                                            # rows 12, 24 and 36 are captured, row 48 is ahead
        b, rows = whole.stepper.filter_window_capture()
        assert rows.tolist() == LAG_ROWS and b.any()
        path = whole.dump(tmp_path / "ck.h5")
        whole.advance(56)
        want, summary = state(whole), whole.filter_summary()
    finally:
        whole.close()
    back = EnsembleSimulation.restore(path, cols, forcing)
    try:
        assert back.next_row == 41 and back.filter_window_offsets == OFFSETS
        b2, rows2 = back.stepper.filter_window_capture()
        assert _same(b, b2) and _same(rows, rows2)
        back.advance(56)
        got = state(back)
    finally:
        back.close()
    for a, c in zip(want, got):
        assert _same(a, c)
    assert summary["rows"].tolist() == summary["window_rows"].tolist() == [48, 96]
    assert summary["window_n_obs"] == 6 and summary["window_offsets"].tolist() == list(OFFSETS)
    assert np.isfinite(summary["loglik"])


# ---- 9, 11. the CLI ----------------------------------------------------------------------------------------------------
WINDOW_KEYS = {"filter_window_offsets", "filter_window_observed", "filter_window_obs_cm", "filter_window_prior_mean_cm",
               "filter_window_prior_std_cm"}


def test_cli_window_key_writes_the_datasets_and_the_closing_line(tmp_path, monkeypatch, capsys):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    params = _cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    files, logs = {}, {}
    pts = [{"Soil_Properties": {"n": 1.6}}, {"Soil_Properties": {"n": 2.4}}]
    for tag, extra in (("well", {"Filter": {"Stride": 24, "Sigma_cm": 10.0}}),
                       ("empty", {"Filter": {"Stride": 24, "Sigma_cm": 10.0, "Window_Offsets": []}}),
                       ("ens", {"Filter": {"Stride": 24, "Sigma_cm": 10.0, "Window_Offsets": [18, 6, 12]}}),
                       ("sweep", {"Points": pts, "Filter": {"Sigma_cm": 10.0, "Window_Offsets": [12, 24, 36]}})):
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 64, "Seed": 3, "Days": 2, **extra}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = loadResults(tmp_path / f"Run_{tag}_ensemble.h5")
        logs[tag] = capsys.readouterr().out
    well, empty, ens, sweep = (files[k] for k in ("well", "empty", "ens", "sweep"))
    assert "filter window" not in logs["well"] and "filter window" not in logs["empty"]
    assert set(well) == set(empty) and all(_same(well[k], empty[k]) for k in well)
    assert set(ens) - set(well) == WINDOW_KEYS
    assert ens["filter_rows"].tolist() == [24, 48, 72, 96] and ens["filter_window_offsets"].tolist() == [6, 12, 18]
    for k in WINDOW_KEYS - {"filter_window_offsets"}:
        assert ens[k].shape == (4, 3), k
    assert ens["filter_window_observed"].tolist() == [[1, 1, 1]] * 4 and np.isfinite(ens["filter_window_prior_std_cm"]).all()
    assert not np.array_equal(ens["filter_loglik_rows"], well["filter_loglik_rows"])    # the joint increment
    assert re.search(r"\[Ensemble x64\] filter window: 12 lagged observations over 4 rows\n", logs["ens"])
    assert sweep["filter_window_obs_cm"].shape == (2, 2, 3) and sweep["filter_rows"].tolist() == [48, 96]
    assert "[Sweep 2 points x64] filter window: 6 lagged observations over 2 rows\n" in logs["sweep"]


def test_a_windowed_sweep_on_two_ranks_writes_what_one_rank_writes(tmp_path):
    params = _cli_params(tmp_path)
    params["Ensemble"] = {"Members": 40, "Seed": 5, "Days": 2,
                          "Points": [{"Soil_Properties": {"n": n}} for n in (1.6, 2.0, 2.2, 2.4)],
                          "Filter": {"Stride": 24, "Sigma_cm": 8.0, "Window_Offsets": [6, 12, 18]}}
    one, log1 = _run_ranks(tmp_path, "one", params, 1)
    two, log2 = _run_ranks(tmp_path, "two", params, 2)
    assert set(one) == set(two) and WINDOW_KEYS <= set(one)
    for k in sorted(set(one) - {"gpus"}):
        assert _same(one[k], two[k]), k
    assert one["filter_window_obs_cm"].shape == (4, 4, 3)
    line = [s for s in log1.splitlines() if "filter window:" in s]
    assert len(line) == 1 and line == [s for s in log2.splitlines() if "filter window:" in s]


def test_cli_refuses_a_window_with_a_sharded_single_point_filter(tmp_path, monkeypatch, capsys):
    from hydromodel_amd import cli
    params = _cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    params["Ensemble"] = {"Members": 64, "Days": 1, "Filter": {"Sigma_cm": 10.0, "Sharded": True, "Window_Offsets": [12]}}
    (tmp_path / "p.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as status:
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "p.json")])
    out = capsys.readouterr().out
    assert status.value.code == 1 and "Filter.Window_Offsets is not available with \"Sharded\": true" in out
    assert not (tmp_path / "Sim_01_ensemble.h5").exists() and "Saving" not in out
