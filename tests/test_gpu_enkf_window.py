"""The well's record inside the EnKF's window on the GPU (include/hydrocol.h hc_set_enkf_window): off means off; the
recorded y, the draws, the gain, the reduced gain, the analysis states and the diagnostics against the float64 NumPy
restatements from the forecast states and the recorded y; invariance under launch length, point order and the dealing of a
sweep's points to handles and ranks; a lagged column without spread; a twin experiment; resume between a capture and its
analysis; the CLI's "Window_Offsets" key."""
import copy
import json
import re

import numpy as np
import pytest

from helpers import digest, golden
from helpers import cli_params as _cli_params, run_cli_ranks as _run_ranks
from test_enkf_sm_cpu import analysis_restated
from test_enkf_sqrt_cpu import rtps_restated, sqrt_analysis_restated
from test_gpu_enkf import _eps_restated, _fresh, _spread, _stepper, _y_of, digest_point_like
from test_gpu_enkf_sm import _record

pytestmark = pytest.mark.gpu

METHODS = [("stochastic", 0.0), ("sqrt", 0.0)]
VARIANTS = METHODS + [("sqrt", 0.5), ("stochastic", 0.5)]


def _same(a, b, keys=None):
    for k in keys or a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


def _without(forcing, rows):
    """The forcing with no observation on ``rows`` (such a row is not solved and cannot take part)."""
    f = copy.copy(forcing)
    obs = np.array(forcing.wtd_obs, dtype=np.int32)
    obs[list(rows)] = -1
    f.wtd_obs = obs
    return f


# ---- 2. off means off --------------------------------------------------------------------------------------------------
def _hooks_run(method, window, forcing=None, rows=150):
    """96 members of well 300 over ``rows`` rows, three sensors on rows 48 and 144: states, tables and every hook."""
    st, cols, _ = _stepper(300, 96, seed=5, forcing=forcing)
    try:
        st.set_wtd_hist(48)
        st.set_enkf(48, 2.0 * cols.dz, 40.0, 3)
        nodes = [6, 20, 45]
        st.set_enkf_soil_moisture(nodes, _record(st.T, nodes, [0.22, 0.26, 0.2], rows=(48, 144)), 0.02)
        st.set_enkf_method(method, 0.0)
        if window is not None:
            st.set_enkf_window(window)
        out = st.step_rows(1, rows)
        got = dict(psi=st.get_state(), moments=np.asarray(st.moments()), hist=st.wtd_hist_table(), table=st.enkf_table(),
                   sm=st.enkf_sm_table(), gain=st.enkf_gain(), y=st.enkf_y(), sm_y=st.enkf_sm_y(), sm_gain=st.enkf_sm_gain(),
                   width=np.array(st.enkf_width()))
        if method == "sqrt":
            got.update(kr=st.enkf_sqrt_gain(), dbar=st.enkf_sqrt_shift())
        else:
            got.update(eps=st.enkf_eps(), sm_eps=st.enkf_sm_eps())
        return got, out["launches"], (st.enkf_window_table() if window else None)
    finally:
        st.close()


@pytest.mark.parametrize("method", ["stochastic", "sqrt"])
def test_off_means_off(method):
    _, cols, forcing = digest(300)
    lagged = [r - o for r in (48, 96, 144) for o in (12, 24, 36)]
    blind = _without(forcing, lagged)
    ref, launches, _ = _hooks_run(method, None)
    empty, launches_e, _ = _hooks_run(method, [])
    _same(ref, empty)
    assert launches_e == launches                                     # no launch is cut
    ref_b, launches_b, _ = _hooks_run(method, None, forcing=blind)
    got_b, launches_w, wt = _hooks_run(method, [12, 24, 36], forcing=blind)
    _same(ref_b, got_b)                                               # no lagged row takes part: nothing changes a bit
    assert launches_w == launches_b and np.isnan(wt).all()
    on, launches_on, wt = _hooks_run(method, [12, 24, 36])            # ... and with the record the analysis is another one
    assert launches_on > launches and not np.array_equal(on["psi"], ref["psi"])
    assert (wt[0, 1:4, :, 0] == 1.0).all() and int(on["width"]) == 1 + 3 + 3 and np.isnan(wt[0, 0]).all()


# ---- 3. against NumPy float64 ------------------------------------------------------------------------------------------
def _window_case(well, P, mpp, loc, n_s, n_off, noise, method, alpha, seed=11, sigma=5.0):
    """One analysis at row 48 with the lagged rows of ``n_off`` offsets (of three, the middle one's row has no
    observation), stepped in pieces so that every lagged row's forecast comes back."""
    N = P * mpp
    _, _, f0 = digest(well)
    offsets = {1: (12,), 3: (12, 24, 36)}[n_off]
    forcing = _without(f0, [24]) if n_off == 3 else f0
    st, cols, _ = _stepper(well, N, P, noise, forcing=forcing)
    nodes = {0: [], 1: [12], 3: [6, 20, 33, 45]}[n_s]                 # 3 sensors present of 4
    vals = {0: [], 1: [0.21], 3: [0.27, np.nan, 0.18, 0.24]}[n_s]
    s_sig = np.array([0.02, 0.03, 0.015, 0.025][:len(nodes)])
    present = [o for o in offsets if forcing.wtd_obs[48 - o] >= 0]
    res = dict(cols=cols, forcing=forcing, offsets=offsets, present=present, nodes=nodes, vals=vals, s_sig=s_sig, N=N)
    try:
        st.set_enkf(48, sigma, loc, seed)
        if nodes:
            st.set_enkf_soil_moisture(nodes, _record(st.T, nodes, vals), s_sig)
        st.set_enkf_method(method, alpha)
        st.set_enkf_window(list(reversed(offsets)))                  # any order: kept ascending
        assert st.enkf_window_offsets == offsets
        row, lag, k = 1, {}, 0
        for stop in sorted(48 - o for o in present) + [48]:
            for begin, n, want in ((row, stop - row, False), (stop, 1, True)):
                if n == 0:
                    continue
                k += 1
                kw = {"fresh_noise": _fresh(st, begin, n, k)} if noise == "numpy" else {}
                out = st.step_rows(begin, n, want_wtd=want, want_psi=want, **kw)
            if stop < 48:
                lag[stop] = (out["psi"][0], out["wtd"][0].astype(np.int64))
            row = stop + 1
        res.update(lag=lag, forecast=out["psi"][0], wtd=out["wtd"][0].astype(np.int64), slots=st.enkf_window_slots(),
                   Yw=st.enkf_window_y(), y=st.enkf_y(), K=st.enkf_full_gain(), K0=st.enkf_gain(), post=st.get_state(),
                   table=st.enkf_table(), wt=st.enkf_window_table(), width=st.enkf_width(),
                   held=st.enkf_window_capture()[1])
        res["Ys"] = st.enkf_sm_y() if nodes else res["y"][:, None]
        if method == "sqrt":
            res.update(Kr=st.enkf_sqrt_gain(), dbar=st.enkf_sqrt_shift())
        else:
            res.update(eps=st.enkf_eps(), eps_s=st.enkf_sm_eps() if nodes else np.zeros((N, 0)), eps_w=st.enkf_window_eps())
        if alpha:
            res["relax"] = st.enkf_relaxation_factors()
    finally:
        st.close()
    return res


@pytest.mark.parametrize("method, alpha", VARIANTS)
@pytest.mark.parametrize("noise", ["philox", "numpy"])
@pytest.mark.parametrize("well, P, mpp, loc, n_s, n_off", [
    (1, 1, 100, 0.0, 0, 1), (1, 3, 100, 60.0, 3, 3), (300, 1, 100, 0.0, 3, 1), (300, 2, 100, 50.0, 0, 3),
    (1, 1, 2500, 0.0, 3, 3), (1, 2, 2500, 80.0, 0, 1),        # the grid of test_gpu_enkf_sm.test_analysis_against_numpy
])
def test_analysis_against_numpy(well, P, mpp, loc, n_s, n_off, noise, method, alpha):
    seed, sigma = 11, 5.0
    c = _window_case(well, P, mpp, loc, n_s, n_off, noise, method, alpha, seed, sigma)
    cols, forcing, N = c["cols"], c["forcing"], c["N"]
    D, dz, psat = cols.dim_d, cols.dz, float(cols.soil.psi_sat)
    present, offsets = c["present"], c["offsets"]
    assert present == ([12] if n_off == 1 else [12, 36])              # row 24 has no observation: absent
    assert c["slots"].tolist() == [offsets.index(o) for o in present] and (c["held"] == -1).all()
    sm_present = [i for i, v in enumerate(c["vals"]) if not np.isnan(v)]
    W = 1 + len(sm_present) + len(present)
    assert c["width"] == W and c["K"].shape == (P, D, W) and c["Yw"].shape == (N, len(present))
    # the recorded y is the operator on the lagged row's forecast
    for k, o in enumerate(present):
        psi_l, w_l = c["lag"][48 - o]
        y_np = _y_of(psi_l, w_l, psat, dz)
        assert np.all(np.abs(c["Yw"][:, k] - y_np) <= 1e-12 * (1.0 + np.abs(y_np))), o
    Y = np.concatenate([c["Ys"], c["Yw"]], axis=1)
    assert np.array_equal(Y[:, 0], c["y"]) and np.array_equal(c["K"][..., 0], c["K0"])       # the existing hooks
    lag_obs = np.array([float(forcing.wtd_obs[48 - o]) * dz for o in present])
    o_vec = np.concatenate([[float(forcing.wtd_obs[48]) * dz], np.asarray(c["vals"], dtype=np.float64)[sm_present], lag_obs])
    R = np.concatenate([[sigma], c["s_sig"][sm_present], [sigma] * len(present)]) ** 2
    zeta = np.concatenate([np.asarray(c["nodes"], dtype=np.float64)[sm_present] * dz, lag_obs])   # its own observed depth

    def close(got, want, tag, bar):                                   # relative to the array's largest entry
        err = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
        print(f" {tag}: {err:.1e}", end="")
        assert got.shape == want.shape and err <= bar, (tag, err)

    forecast = c["forecast"]
    if method == "sqrt":
        res = sqrt_analysis_restated(forecast, Y, o_vec, R, zeta, dz, loc, mpp)
        close(c["Kr"], res["Kr"], "Kr", 1e-10)
        close(c["dbar"], res["dbar"], "dbar", 1e-10)
        loglik = analysis_restated(forecast, Y, np.zeros_like(Y), o_vec, R, zeta, dz, loc, mpp)["loglik"]
    else:
        eps_np = np.array([[_eps_restated(seed, m, 48 - o) for o in present] for m in range(N)])
        close(c["eps_w"], eps_np, "eps", 1e-13)                       # the well's draw with the lagged row in the row word
        E = np.concatenate([c["eps"][:, None], c["eps_s"][:, sm_present], c["eps_w"]], axis=1)
        res = analysis_restated(forecast, Y, E, o_vec, R, zeta, dz, loc, mpp)
        loglik = res["loglik"]
    close(c["K"], res["K"], "K", 1e-10)
    assert np.abs(c["K"][..., W - len(present):]).max() > 0.0
    want = res["post"]
    if alpha:
        sb_np, sa_np, f_np, want = rtps_restated(forecast, res["post"], alpha, mpp)
        close(c["relax"][0], sb_np, "sigma_b", 1e-10)
        close(c["relax"][1], sa_np, "sigma_a", 1e-10)
    close(c["post"], want, "states", 1e-9)
    assert not np.array_equal(c["post"], forecast)
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        t = c["table"][p, 1]
        err = abs(t[4] - loglik[p]) / max(1.0, abs(loglik[p]))
        print(f" loglik: {err:.1e}", end="")
        assert t[0] == mpp and t[7] == 0 and err <= 1e-10             # the joint density of everything assimilated
        w = c["wt"][p, 1]
        for j, o in enumerate(offsets):
            if o not in present:
                assert w[j, 0] == 0.0 and np.isnan(w[j, 1:]).all()
                continue
            yk = c["Yw"][sl, present.index(o)]
            assert w[j, 0] == 1.0 and w[j, 1] == float(forcing.wtd_obs[48 - o]) * dz
            assert abs(w[j, 2] - yk.mean()) <= 1e-12 * abs(yk.mean()) and abs(w[j, 3] - yk.std(ddof=1)) <= 1e-10 * (1.0 + yk.std(ddof=1))
        assert np.isnan(c["wt"][p, 0]).all() and np.isnan(c["wt"][p, 2:]).all()
    print()


@pytest.mark.parametrize("noise", ["philox", "numpy"])
def test_the_recorded_y_is_what_the_y_hook_returns_on_that_row(noise):
    """A handle whose stride IS the lagged row analyses there first (no earlier row of it is one), and its hc_get_enkf_y
    holds the forecast y of that row: the window's column must be the same bits."""
    N, seed = 200, 11
    c = _window_case(300, 2, 100, 40.0, 0, 3, noise, "stochastic", 0.0, seed)
    for k, o in enumerate(c["present"]):
        r = 48 - o
        st, _, _ = _stepper(300, N, 2, noise, forcing=c["forcing"])
        try:
            st.set_enkf(r, 5.0, 40.0, seed)
            # the pieces of _window_case up to row r: the host noise is drawn per call
            row, j = 1, 0
            for stop in [s for s in sorted(48 - x for x in c["present"]) if s <= r]:
                for begin, n in ((row, stop - row), (stop, 1)):
                    if n == 0:
                        continue
                    j += 1
                    kw = {"fresh_noise": _fresh(st, begin, n, j)} if noise == "numpy" else {}
                    st.step_rows(begin, n, **kw)
                row = stop + 1
            y = st.enkf_y()
        finally:
            st.close()
        assert y.tobytes() == np.ascontiguousarray(c["Yw"][:, k]).tobytes(), o


# ---- 4. the same bits however it is launched ---------------------------------------------------------------------------
NS, MPP, SEED = (1.6, 2.0, 2.4), 70, 31


def _point_handle(ids, method, rows_per_launch=0):
    from hydromodel_amd.stepper import EnsembleStepper
    pts = [digest_point_like(NS[k]) for k in ids]
    psi_all = _spread(golden("g1_tables_1.npz")["initial_cond"], 3 * MPP, seed=4)
    forcing = _without(pts[0][2], [66, 90, 114])                      # offset 6 absent on rows 72, 96 and 120
    st = EnsembleStepper([c for _, c, _ in pts], forcing, len(ids) * MPP)
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
        v[48] = [0.2, np.nan]
        st.set_enkf_soil_moisture([8, 30], v, [0.02, 0.03])
        st.set_enkf_method(method, 0.5 if method == "sqrt" else 0.0)
        st.set_enkf_window([6, 13, 18])
        st.step_rows(1, 150)
        n = len(ids)
        return dict(psi=st.get_state().reshape(n, MPP, -1), table=st.enkf_table(), sm=st.enkf_sm_table(),
                    win=st.enkf_window_table(), moments=np.asarray(st.moments()).reshape(n, 3, -1),
                    hist=st.wtd_hist_table().reshape(n, -1))
    finally:
        st.close()


@pytest.mark.parametrize("method", ["stochastic", "sqrt"])
def test_results_do_not_depend_on_launch_length_point_order_or_handles(method):
    whole = _point_handle([0, 1, 2], method)
    assert (whole["table"][:, 1:7, 0] == MPP).all()
    assert (whole["win"][:, [1, 2, 6], :, 0] == 1.0).all() and (whole["win"][:, [3, 4, 5], :, 0] == [0.0, 1.0, 1.0]).all()
    runs = {"rows 1": (_point_handle([0, 1, 2], method, 1), [0, 1, 2]), "rows 7": (_point_handle([0, 1, 2], method, 7), [0, 1, 2]),
            "reversed": (_point_handle([2, 1, 0], method), [2, 1, 0]), "split a": (_point_handle([0, 2], method), [0, 2]),
            "split b": (_point_handle([1], method), [1])}
    for tag, (part, ids) in runs.items():
        for j, k in enumerate(ids):
            for key in ("psi", "table", "sm", "win", "moments", "hist"):
                a, b = whole[key][k], part[key][j]
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (tag, k, key)


WINDOW_KEYS = {"enkf_window_offsets", "enkf_window_observed", "enkf_window_obs_cm", "enkf_window_prior_mean_cm",
               "enkf_window_prior_std_cm", "enkf_window_innovation_cm"}


def test_a_window_sweep_on_two_ranks_writes_what_one_rank_writes(tmp_path):
    params = _cli_params(tmp_path)
    params["Ensemble"] = {"Members": 40, "Seed": 5, "Days": 2, "Distribution": {"Stride": 48},
                          "Points": [{"Soil_Properties": {"n": n}} for n in (1.6, 2.0, 2.2, 2.4)],
                          "EnKF": {"Stride": 24, "Sigma_cm": 8.0, "Window_Offsets": [18, 6, 12]}}
    one, log1 = _run_ranks(tmp_path, "one", params, 1)
    two, log2 = _run_ranks(tmp_path, "two", params, 2)
    assert set(one) == set(two) and WINDOW_KEYS <= set(one)
    for k in sorted(WINDOW_KEYS) + ["enkf_loglik_rows", "enkf_prior_mean_cm", "enkf_post_mean_cm", "enkf_post_std_cm",
                                   "moments", "wtd_hist"]:
        a, b = np.asarray(one[k]), np.asarray(two[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert one["enkf_window_obs_cm"].shape == (4, 4, 3) and one["enkf_window_offsets"].tolist() == [6, 12, 18]
    line = [s for s in log1.splitlines() if "EnKF window" in s]
    assert len(line) == 1 and line == [s for s in log2.splitlines() if "EnKF window" in s]


# ---- 5. a lagged column without spread ---------------------------------------------------------------------------------
@pytest.mark.parametrize("method, alpha", METHODS)
@pytest.mark.parametrize("value", [128.0, 100.1])
def test_a_lagged_column_every_member_agrees_on_changes_nothing(method, alpha, value):
    """The y recorded for offset 12 is replaced by one value for every member (hc_set_enkf_window_capture), so the column
    has no covariance with anything and the analysis must be the one without that offset.

    value = 128.0: BIT EQUALITY.  The tile sums of N = 200 copies of 2^7 are exact (N 2^7 < 2^53), so the mean is 2^7, the
    anomalies are exact zeros, and so are the column's covariances, its off-diagonal entries of the Cholesky factor, its
    column of K and Kr and its term of every increment; the terms before it are summed in the same order as without it,
    and x - 0 * y = x, x + 0 * y = x exactly.

    value = 100.1: a DERIVED bound, because the mean of N equal values need not be that value (LAB_NOTES.md 15, "sigma_a =
    0").  With u = 2^-53 the computed mean differs from the value by delta <= N u |value| (plain recursive summation,
    Higham 2002 eq. 4.4, divided by N), and every anomaly is that same delta.  By Cauchy-Schwarz the column's covariance
    with node d is at most sd_d delta sqrt(N / (N - 1)) <= 2 sd_d delta, its own variance delta^2 N / (N - 1) is far below
    sigma^2, so its gain is at most 2 sd_d delta / sigma^2 (S >= R on the diagonal; the coupling it adds to the other
    columns is O(delta^2 / sigma^2) relative, below u) and its term of the increment at most that times the largest
    innovation |o - value| + sigma max|eps| + delta (square root: |o - value| + delta, Kr <= K in magnitude).  On top, the
    states of both runs are each rounded once when the increment is added and once per term of the increment: 8 u
    (1 + |psi| + |increment|).  So |difference_d| <= 2 sd_d delta innov / sigma^2 * 2 + 8 u (1 + |psi_d| + |inc_d|)."""
    N, sigma, seed = 200, 5.0, 11
    out = {}
    for tag, offsets in (("with", (12, 30)), ("without", (30,))):
        st, cols, forcing = _stepper(1, N, 1, "philox")
        try:
            st.set_enkf(48, sigma, 0.0, seed)
            st.set_enkf_method(method, alpha)
            st.set_enkf_window(offsets)
            st.step_rows(1, 40)                                       # rows 18 and 36 are behind it
            y, rows = st.enkf_window_capture()
            assert rows.tolist() == [48 - o for o in offsets]
            if tag == "with":
                y[0] = value
                st.set_enkf_window_capture(y, rows)
            res = st.step_rows(41, 8, want_psi=True)
            out[tag] = dict(post=st.get_state(), forecast=res["psi"][-1], table=st.enkf_table(), K=st.enkf_full_gain())
            if tag == "with" and method == "stochastic":
                eps_max = float(np.abs(st.enkf_window_eps()[:, 0]).max())
        finally:
            st.close()
    a, b = out["with"], out["without"]
    assert np.array_equal(a["forecast"], b["forecast"]) and not np.array_equal(a["post"], a["forecast"])
    if value == 128.0:
        assert a["post"].tobytes() == b["post"].tobytes()
        assert not a["K"][..., 1].any() and np.array_equal(a["K"][..., [0, 2]], b["K"])
        assert a["table"][..., 5:].tobytes() == b["table"][..., 5:].tobytes()       # the posterior diagnostics too
        return
    u = 2.0 ** -53
    delta = N * u * abs(value)
    innov = abs(float(forcing.wtd_obs[36]) * cols.dz - value) + delta + (sigma * eps_max if method == "stochastic" else 0.0)
    sd = a["forecast"].std(axis=0, ddof=1)
    inc = np.abs(b["post"] - b["forecast"])
    bound = 4.0 * sd[None, :] * delta * innov / sigma ** 2 + 8.0 * u * (1.0 + np.abs(b["post"]) + inc)
    diff = np.abs(a["post"] - b["post"])
    print(f" largest difference {diff.max():.2e}, its bound {bound.flat[diff.argmax()]:.2e}")
    assert np.all(diff <= bound)


# ---- 6. twin experiment ------------------------------------------------------------------------------------------------
def _twin(rows, runs):
    """test_gpu_enkf._twin's set-up (well 1, 256 members, +-60 cm offsets, truth at +35 cm, sigma = 2 dz): the mean CRPS of
    the forecast over the daily histogram rows and the failed BDF attempts per member-day of every run."""
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
    crps, failed, lagged = {}, {}, {}
    for tag, (stride, offsets) in runs.items():
        st, _, _ = _stepper(1, N, seed=4, forcing=twin)
        try:
            st.set_state(psi0[None, :] + shifts[:, None])
            st.set_wtd_hist(48)
            if stride:
                st.set_enkf(stride, 2.0 * cols.dz, 0.0, 17)
                st.set_enkf_window(offsets)
            out = st.step_rows(1, rows, want_stats=True)
            hist = st.wtd_hist_table()[0]
            lagged[tag] = int(np.nansum(st.enkf_window_table()[..., 0])) if offsets else 0
        finally:
            st.close()
        crps[tag] = float(wtd_distribution(hist, obs, (0.5,), cols.dz, cols.z, 0, 48)["crps_mean_cm"])
        failed[tag] = float(out["failed"].sum()) / (N * rows / 48.0)
    return crps, failed, lagged


def test_twin_experiment_every_filtered_run_beats_the_open_loop(capsys):
    runs = {"open": (0, ()), "48": (48, ()), "48+[12,24,36]": (48, (12, 24, 36)), "192": (192, ()),
            "192+[48,96,144]": (192, (48, 96, 144))}
    crps, failed, lagged = _twin(10 * 48, runs)
    with capsys.disabled():
        print("\n twin experiment, 256 members, 10 days, +-60 cm spread, sigma = 2 dz: " +
              "; ".join(f"{k}: CRPS {crps[k]:.4f} cm, failed {failed[k]:.4f}/member-day, {lagged[k]} lagged obs" for k in runs))
    for tag in runs:
        if tag != "open":
            assert crps[tag] < crps["open"], tag                      # (not that the windowed runs win: one seed)
    assert lagged["48+[12,24,36]"] > 0 and lagged["192+[48,96,144]"] > 0


# ---- 7. checkpoint -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["stochastic", "sqrt"])
def test_dump_between_a_capture_and_its_analysis_resumes_bit_for_bit(tmp_path, method):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(1)
    psi0 = _spread(golden("g1_tables_1.npz")["initial_cond"], 96)
    kw = dict(seed=6, psi0=psi0, wtd_hist_stride=48, enkf_stride=48, enkf_sigma_cm=2.0 * cols.dz,
              enkf_localisation_cm=50.0, enkf_method=method, enkf_window_offsets=(36, 12, 24))
    whole = EnsembleSimulation(cols, forcing, 96, **kw)
    try:
        whole.advance(78)                                             # rows 60 and 72 are recorded, 84 and 96 are ahead
        assert whole.stepper.enkf_window_capture()[1].tolist() == [-1, 72, 60]
        path = whole.dump(tmp_path / "ck.h5")
        whole.advance(140)
        want = [whole.stepper.get_state(), whole.enkf_table(), whole.enkf_window_table(), whole.moments()]
        summary = whole.enkf_summary()
    finally:
        whole.close()
    back = EnsembleSimulation.restore(path, cols, forcing)
    try:
        assert back.enkf_window_offsets == (12, 24, 36)
        assert back.stepper.enkf_window_capture()[1].tolist() == [-1, 72, 60]
        back.advance(140)
        got = [back.stepper.get_state(), back.enkf_table(), back.enkf_window_table(), back.moments()]
    finally:
        back.close()
    for a, b in zip(want, got):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    took = sum(int(forcing.wtd_obs[r - o] >= 0) for r in (48, 96, 144, 192) for o in (12, 24, 36))
    assert summary["window_rows"].tolist() == [48, 96, 144, 192] and summary["window_n_obs"] == took == 12
    assert summary["window_observed"].all() and np.isfinite(summary["window_innovation_cm"]).all()


def test_refusals_and_what_turns_the_window_off():
    from hydromodel_amd import _lib as L
    st, cols, _ = _stepper(1, 8)
    T = st.T

    def set_raw(offsets):
        a = np.ascontiguousarray(offsets, dtype=np.int32)
        L.check(st.lib.hc_set_enkf_window(st.h, a.size, L.iptr(a)))
    try:
        with pytest.raises(ValueError, match="need the EnKF"):
            st.set_enkf_window([12])
        with pytest.raises(L.HcError, match="the EnKF is off"):
            set_raw([12])
        st.set_enkf(48, 5.0, 0.0, 1)
        for bad in ([0], [48], [60], [12, 12], list(range(1, 10))):   # the library's own refusals
            with pytest.raises(L.HcError):
                set_raw(bad)
        st.set_enkf_soil_moisture([3, 4, 5], np.full((T, 3), 0.2), 0.02)
        with pytest.raises(L.HcError, match="at most 8 together"):
            set_raw([1, 2, 3, 4, 5, 6])
        st.set_enkf_window([1, 2, 3, 4, 5])
        assert st.enkf_window_table().shape == (1, (T - 1) // 48 + 1, 5, 4) and np.isnan(st.enkf_window_table()).all()
        with pytest.raises(L.HcError, match="at most 8 together"):
            st.set_enkf_soil_moisture([3, 4, 5, 6], np.full((T, 4), 0.2), 0.02)
        st.set_enkf(48, 5.0, 0.0, 1)                             # hc_set_enkf turns the window off
        assert st.enkf_window_offsets == ()
        with pytest.raises(L.HcError, match="no window offsets"):
            L.check(st.lib.hc_get_enkf_window_stats(st.h, L.dptr(np.zeros(1)), -1))
    finally:
        st.close()


def _enkf_with_record_and_window():
    """One point, 64 members of well 1, the EnKF on with a two-sensor record and the offsets (12, 24, 36); no row stepped."""
    st, _, _ = _stepper(1, 64)
    st.set_enkf(48, 5.0, 0.0, 1)
    st.set_enkf_soil_moisture([6, 45], _record(st.T, [6, 45], [0.24, 0.36]), 0.02)
    st.set_enkf_window([12, 24, 36])
    return st


def test_the_particle_filters_off_calls_leave_the_enkfs_record_and_window_alone():
    from hydromodel_amd import _lib as L
    st = _enkf_with_record_and_window()
    try:
        L.check(st.lib.hc_set_filter_soil_moisture(st.h, 0, None, None, None))
        L.check(st.lib.hc_set_filter_window(st.h, 0, None))
        n_arow = (st.T - 1) // 48 + 1
        sm, wt = st.enkf_sm_table(), st.enkf_window_table()
        assert sm.shape == (1, n_arow, 2, 6) and np.isnan(sm).all()
        assert wt.shape == (1, n_arow, 3, 4) and np.isnan(wt).all()
        assert st.enkf_window_capture()[1].tolist() == [-1, -1, -1]
    finally:
        st.close()


def test_nothing_of_the_enkfs_carries_over_to_the_particle_filter():
    from hydromodel_amd import _lib as L
    st = _enkf_with_record_and_window()
    try:
        st.set_enkf(0)
        st.set_filter(48, 5.0, 1)
        assert st.filter_sm_width() == 0
        with pytest.raises(L.HcError, match="no soil-moisture record"):
            L.check(st.lib.hc_get_filter_sm_stats(st.h, L.dptr(np.zeros(1)), -1))
        with pytest.raises(L.HcError, match="no window offsets"):
            st.filter_window_capture()
    finally:
        st.close()


def test_cli_window_offsets_writes_the_datasets(tmp_path, monkeypatch, capsys):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    params = _cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    files, logs = {}, {}
    pts = [{"Soil_Properties": {"n": 1.6}}, {"Soil_Properties": {"n": 2.4}}]
    for tag, extra in (("well", {"EnKF": {"Stride": 24, "Sigma_cm": 10.0}}),
                       ("empty", {"EnKF": {"Stride": 24, "Sigma_cm": 10.0, "Window_Offsets": []}}),
                       ("ens", {"EnKF": {"Stride": 24, "Sigma_cm": 10.0, "Window_Offsets": [12, 6]}}),
                       ("sweep", {"Points": pts, "EnKF": {"Sigma_cm": 10.0, "Method": "sqrt", "Window_Offsets": [12, 24, 36]}})):
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 64, "Seed": 3, "Days": 2, **extra}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = loadResults(tmp_path / f"Run_{tag}_ensemble.h5")
        logs[tag] = capsys.readouterr().out
    well, empty, ens, sweep = (files[k] for k in ("well", "empty", "ens", "sweep"))
    _same(well, empty)                                                # an empty list: today's file and lines
    assert set(well) == set(empty) and logs["empty"] == logs["well"].replace("Run_well", "Run_empty")
    assert "EnKF window" not in logs["well"] and set(ens) - set(well) == WINDOW_KEYS
    assert ens["enkf_rows"].tolist() == [24, 48, 72, 96] and ens["enkf_window_offsets"].tolist() == [6, 12]
    assert ens["enkf_window_observed"].tolist() == [[1, 1]] * 4
    for k in WINDOW_KEYS - {"enkf_window_offsets"}:
        assert ens[k].shape == (4, 2), k
    assert np.allclose(ens["enkf_window_innovation_cm"], ens["enkf_window_obs_cm"] - ens["enkf_window_prior_mean_cm"],
                       rtol=0.0, atol=1e-9)
    assert not np.array_equal(ens["enkf_post_mean_cm"], well["enkf_post_mean_cm"])
    assert re.search(r"\[Ensemble x64\] EnKF window: 8 lagged observations over 4 rows \(offsets \[6, 12\]\)", logs["ens"])
    assert sweep["enkf_window_obs_cm"].shape == (2, 2, 3) and sweep["enkf_rows"].tolist() == [48, 96]
    assert "[Sweep 2 points x64] EnKF window: 6 lagged observations over 2 rows" in logs["sweep"]
