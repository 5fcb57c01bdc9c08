"""The EnKF's analysis on the GPU at every slot count of a wavefront (hydrocol.hip ENKF_SLOTS: D = 41 ... 640, the cases
of tests/enkf_depths.py), with the observed water table on the boundary between two slots and, in two of the four
configurations, the full batch m' = 9 = ENKF_OBS: the operator, the draws, the gains, the relaxation, the analysis states,
the tables and the noise field against the float64 NumPy restatements of the existing modules, from the GPU's own
forecast.  Then two tiles of members at the deepest column, one member per point, and the refusal path at D = 64, 65, 640.

Tolerances: the project's bars (LAB_NOTES 13).  A gain that misses its bar against the float64 restatement is judged
against enkf_depths.gain_longdouble on the same forecast: the bar becomes the larger of 1e-10 and 8 x the float64
restatement's own error against it (8: the kernel's fixed-order sums over up to 300 members against NumPy's pairwise
ones), and a kernel error above that is a defect.  No case needed the raised bar: the largest kernel error against the
float64 restatement over all 48 cases is recorded in LAB_NOTES.md 29 and stays below 1e-10 everywhere."""
import numpy as np
import pytest

import enkf_depths as depths
from test_enkf_sm_cpu import analysis_restated
from test_enkf_sqrt_cpu import rtps_restated, sqrt_analysis_restated
from test_gpu_enkf import _eps_restated, _find_wtd, _y_of
from test_gpu_enkf_sm import _eps_sensor

pytestmark = pytest.mark.gpu

ROW, SEED = depths.STRIDE, depths.SEED
STOPS = sorted(ROW - o for o in depths.OFFSETS) + [ROW]               # the launches end on rows 2, 3, 4, 5 and 6


def _same(a, b, tag=None):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), tag


def _run(D, node, tag, mpp=depths.MPP, sigma=depths.SIGMA_CM, noise_field=True, twin=False):
    """One handle stepped in pieces through the analysis on row 6, so that the forecast of every lagged row and of row 6
    comes back; everything the checks read.  ``twin``: the same run with its analyses on every 12th row and the noise
    field on: the forecast and the base vectors as the analysis of row 6 finds them (a retried solve damps a member's
    vector in place, test_gpu_enkf_noise._forecast_base)."""
    from hydromodel_amd.stepper import EnsembleStepper
    cfg = depths.CONFIGS[tag]
    c = depths.build(D, node, cfg["P"], mpp)
    N, forcing, wide = c["N"], c["forcing"], cfg["wide"] and not twin
    alpha_z = cfg["alpha_z"] if noise_field else None
    st = EnsembleStepper(c["points"] if cfg["P"] > 1 else c["cols"], forcing, N)
    res = dict(c, tag=tag, cfg=cfg, alpha_z=alpha_z, sigma=sigma)
    try:
        st.set_state(c["psi0"])
        st.set_noise_host(c["base"])
        st.set_enkf(2 * ROW if twin else ROW, sigma, cfg["loc"], SEED)
        if wide:
            st.set_enkf_soil_moisture(c["nodes"], depths.sensor_record(st.T, c["nodes"], c["values"]), c["sigmas"])
        st.set_enkf_method(cfg["method"], cfg["alpha"])
        if wide:
            st.set_enkf_window(depths.OFFSETS)
        if twin or alpha_z is not None:
            st.set_enkf_noise_field(True, 0.0 if twin else alpha_z)
        row, lag = 1, {}
        for stop in STOPS:
            for begin, n, want in ((row, stop - row, False), (stop, 1, True)):
                if n == 0:
                    continue
                out = st.step_rows(begin, n, fresh_noise=np.zeros((st.n_refresh(begin, n), N, D)), want_wtd=want,
                                   want_psi=want)
            if stop < ROW:
                lag[stop] = (out["psi"][0], out["wtd"][0].astype(np.int64))
            row = stop + 1
        res.update(lag=lag, forecast=out["psi"][0], wtd=out["wtd"][0].astype(np.int64))
        if twin:
            res["z_f"] = st.enkf_noise_base()
            return res
        res.update(width=st.enkf_width(), y=st.enkf_y(), K=st.enkf_full_gain(), K0=st.enkf_gain(), post=st.get_state(),
                   table=st.enkf_table())
        root = cfg["method"] == "sqrt"
        if wide:
            res.update(Ys=st.enkf_sm_y(), Yw=st.enkf_window_y(), slots=st.enkf_window_slots(), smt=st.enkf_sm_table(),
                       wt=st.enkf_window_table(), held=st.enkf_window_capture()[1])
        else:
            res.update(Ys=res["y"][:, None], Yw=np.zeros((N, 0)))
        if root:
            res.update(Kr=st.enkf_sqrt_gain(), dbar=st.enkf_sqrt_shift())
        else:
            res.update(eps=st.enkf_eps(), eps_s=st.enkf_sm_eps() if wide else np.zeros((N, 0)),
                       eps_w=st.enkf_window_eps() if wide else np.zeros((N, 0)))
        if cfg["alpha"] and mpp > 1:
            res["relax"] = st.enkf_relaxation_factors()
        if alpha_z is not None:
            res.update(z_a=st.enkf_noise_base(), nzt=st.enkf_noise_table(), Kz=st.enkf_noise_gain())
            if root:
                res.update(Krz=st.enkf_noise_sqrt_gain(), shift_z=st.enkf_noise_sqrt_shift())
        if wide:                                                      # last: the handle's state is replaced
            at = list(c["nodes"])
            st.set_state(res["forecast"])
            res["theta_f"] = st.model_nodes()["theta"][:, at]
            st.set_state(res["post"])
            res["theta_post"] = st.model_nodes()["theta"][:, at]
    finally:
        st.close()
    return res


def _observations(r):
    """(o [m'], sigma [m'], zeta [m' - 1]) of the analysis: the well, the four sensors, the lagged rows by ascending
    offset (each at its own observed depth)."""
    dz, node, sigma = r["cols"].dz, r["node"], r["sigma"]
    if not r["cfg"]["wide"]:
        return np.array([node * dz]), np.array([sigma]), np.zeros(0)
    lag = [float(r["forcing"].wtd_obs[ROW - o]) * dz for o in depths.OFFSETS]
    o = np.concatenate([[node * dz], r["values"], lag])
    sig = np.concatenate([[sigma], r["sigmas"], [sigma] * len(lag)])
    return o, sig, np.concatenate([np.asarray(r["nodes"], dtype=np.float64) * dz, lag])


class _Figures:
    """The measured maxima of one case, printed in one line (LAB_NOTES.md 29 is filled from them)."""

    def __init__(self, r):
        self.head, self.items = f" depths D={r['D']} {r['tag']} mpp={r['mpp']}:", []

    def close(self, got, want, tag, bar):
        """relative to the array's largest entry (LAB_NOTES 13)"""
        err = depths.rel_to_largest(got, want)
        self.items.append(f"{tag} {err:.1e}")
        assert got.shape == want.shape and err <= bar, (self.head, tag, err)

    def gain(self, got, want, exact, tag, bar=1e-10):
        """a gain against the float64 restatement, with the np.longdouble one as arbiter (the module's docstring)"""
        err, e_np, e_k = (depths.rel_to_largest(got, want), depths.rel_to_largest(want, exact),
                          depths.rel_to_largest(got, exact))
        self.items.append(f"{tag} {err:.1e} (float64 {e_np:.1e}, kernel {e_k:.1e} against longdouble)")
        assert got.shape == want.shape, (self.head, tag)
        assert err <= bar or e_k <= max(bar, 8.0 * e_np), (self.head, tag, err, e_np, e_k)

    def note(self, tag, err):
        self.items.append(f"{tag} {err:.1e}")

    def show(self):
        print(self.head + " " + "; ".join(self.items))


def _exact_gains(x, Y, o, sig, zeta, dz, loc, mpp, root):
    """enkf_depths.gain_longdouble per point: K, Kr [P][D][m'], shift [P][D] (None unless ``root``)"""
    parts = [depths.gain_longdouble(x[p * mpp:(p + 1) * mpp], Y[p * mpp:(p + 1) * mpp], o, sig, zeta, dz, loc, root)
             for p in range(x.shape[0] // mpp)]
    K = np.stack([k for k, _, _ in parts])
    return (K, np.stack([kr for _, kr, _ in parts]), np.stack([s for _, _, s in parts])) if root else (K, None, None)


def _check(r, z_f=None):
    cfg, D, N, P, mpp, node = r["cfg"], r["D"], r["N"], r["P"], r["mpp"], r["node"]
    cols, forcing, wide, root = r["cols"], r["forcing"], r["cfg"]["wide"], r["cfg"]["method"] == "sqrt"
    dz, psat, loc, sigma = cols.dz, float(cols.soil.psi_sat), cfg["loc"], r["sigma"]
    assert all(float(pt.soil.psi_sat) == psat for pt in r["points"])
    fig = _Figures(r)
    forecast, wtd, post = r["forecast"], r["wtd"], r["post"]
    # coverage: the forecast's water tables reach both sides of the slot boundary (test_enkf_depths_cpu.py)
    for i in depths.coverage_indices(D, node):
        assert (wtd == i).any(), (D, i, np.bincount(wtd, minlength=D)[max(node - 3, 0):node + 4])
    # width
    W = depths.ENKF_OBS if wide else 1
    assert r["width"] == W and r["K"].shape == (P, D, W) and int(forcing.wtd_obs[ROW]) == node
    # operator
    assert np.array_equal(_find_wtd(forecast, psat), wtd)
    y_np = _y_of(forecast, wtd, psat, dz)
    assert np.all(np.abs(r["y"] - y_np) <= 1e-12 * (1.0 + np.abs(y_np)))
    assert np.unique(r["y"]).size > np.unique(wtd).size               # a continuous y
    if wide:
        assert r["Ys"].shape == (N, 5) and r["Yw"].shape == (N, 4) and np.array_equal(r["Ys"][:, 0], r["y"])
        assert r["slots"].tolist() == [0, 1, 2, 3] and (r["held"] == -1).all()
        assert np.array_equal(r["Ys"][:, 1:], r["theta_f"])           # model_nodes' bits
        for k, o in enumerate(depths.OFFSETS):
            psi_l, w_l = r["lag"][ROW - o]
            assert np.array_equal(_find_wtd(psi_l, psat), w_l), o
            yl = _y_of(psi_l, w_l, psat, dz)
            assert np.all(np.abs(r["Yw"][:, k] - yl) <= 1e-12 * (1.0 + np.abs(yl))), o
    Y = np.concatenate([r["Ys"], r["Yw"]], axis=1)
    assert Y.shape == (N, W) and np.array_equal(r["K"][..., 0], r["K0"])
    o_vec, sig, zeta = _observations(r)
    R = sig ** 2
    # draws
    if not root:
        members = depths.spread_members(N)
        E = np.concatenate([r["eps"][:, None], r["eps_s"], r["eps_w"]], axis=1)
        assert E.shape == (N, W) and np.isfinite(E).all()
        rows_words = [(ROW, None)]                                    # (the draw's row word, the sensor's record index)
        if wide:
            rows_words += [(ROW, i) for i in range(4)] + [(ROW - o, None) for o in depths.OFFSETS]
        for m in members:
            for k, (row, sensor) in enumerate(rows_words):
                want = _eps_restated(SEED, int(m), row) if sensor is None else _eps_sensor(SEED, int(m), row, sensor)
                assert abs(E[m, k] - want) <= 1e-13 * (1.0 + abs(want)), (m, k)
    # gains
    Kx, Krx, shx = _exact_gains(forecast, Y, o_vec, sig, zeta, dz, loc, mpp, root)
    if root:
        res = sqrt_analysis_restated(forecast, Y, o_vec, R, zeta, dz, loc, mpp)
        fig.gain(r["Kr"], res["Kr"], Krx, "Kr")
        fig.gain(r["dbar"], res["dbar"], shx, "dbar")
        loglik = analysis_restated(forecast, Y, np.zeros_like(Y), o_vec, R, zeta, dz, loc, mpp)["loglik"]
    else:
        res = analysis_restated(forecast, Y, E, o_vec, R, zeta, dz, loc, mpp)
        loglik = res["loglik"]
    fig.gain(r["K"], res["K"], Kx, "K")
    for i in range(W):                                                # the deepest node's sensor has no variance
        if not (wide and i == 4):
            assert np.abs(r["K"][..., i]).max() > 0.0, i
            assert not root or np.abs(r["Kr"][..., i]).max() > 0.0, i
    # states
    want = res["post"]
    if cfg["alpha"]:
        sb_np, sa_np, _, want = rtps_restated(forecast, res["post"], cfg["alpha"], mpp)
        fig.close(r["relax"][0], sb_np, "sigma_b", 1e-10)
        fig.close(r["relax"][1], sa_np, "sigma_a", 1e-10)
    err = float(np.max(np.abs(post - want) / np.maximum(1.0, np.abs(want))))
    fig.note("states", err)
    assert err <= 1e-9, (fig.head, err)
    assert not np.array_equal(post, forecast)
    # tables
    table = r["table"]
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        t = table[p, 1]
        yb, sd = Y[sl, 0].mean(), Y[sl, 0].std(ddof=1)
        assert t[0] == mpp and t[7] == 0
        assert abs(t[1] - yb) <= 1e-12 * abs(yb) and abs(t[2] - sd) <= 1e-10 * sd
        assert abs(t[3] - (node * dz - yb)) <= 1e-10 * (1.0 + abs(t[3]))
        err = abs(t[4] - loglik[p]) / max(1.0, abs(loglik[p]))
        fig.note(f"loglik[{p}]", err)
        assert err <= 1e-10, (fig.head, p, err)
        w_post = _find_wtd(post[sl], psat)
        y_post = _y_of(post[sl], w_post, psat, dz)
        cross = depths.cross_slot_index(D, node)
        if cross is not None:                                         # the update's own find_wtd reads across two slots
            fig.items.append(f"{int((w_post == cross).sum())} analysis columns at {cross}")
            assert (w_post == cross).any(), (fig.head, p)             # ... and t[5], t[6] below are what checks it
        assert abs(t[5] - y_post.mean()) <= 1e-9 * (1.0 + abs(y_post.mean()))
        assert abs(t[6] - y_post.std(ddof=1)) <= 1e-9 * (1.0 + y_post.std(ddof=1))
        assert np.isnan(table[p, 2:, 1:]).all() and np.all(table[p, 2:, 0] == 0) and table[p, 0, 0] == 0
        if not wide:
            continue
        s = r["smt"][p, 1]
        for i in range(4):
            th, tp = r["theta_f"][sl, i], r["theta_post"][sl, i]
            assert s[i, 0] == 1.0 and s[i, 1] == r["values"][i]
            assert abs(s[i, 2] - th.mean()) <= 1e-12 and abs(s[i, 3] - th.std(ddof=1)) <= 1e-10
            assert abs(s[i, 4] - tp.mean()) <= 1e-12 and abs(s[i, 5] - tp.std(ddof=1)) <= 1e-10
        assert np.isnan(r["smt"][p, 2:]).all() and np.isnan(r["smt"][p, 0]).all()
        w = r["wt"][p, 1]
        for j, o in enumerate(depths.OFFSETS):
            yk = r["Yw"][sl, j]
            assert w[j, 0] == 1.0 and w[j, 1] == float(forcing.wtd_obs[ROW - o]) * dz
            assert abs(w[j, 2] - yk.mean()) <= 1e-12 * abs(yk.mean())
            assert abs(w[j, 3] - yk.std(ddof=1)) <= 1e-10 * (1.0 + yk.std(ddof=1))
        assert np.isnan(r["wt"][p, 0]).all() and np.isnan(r["wt"][p, 2:]).all()
    # noise field
    if r["alpha_z"] is not None:
        _check_noise(r, z_f, Y, None if root else E, o_vec, sig, zeta, fig)
    fig.show()


def _check_noise(r, z_f, Y, E, o_vec, sig, zeta, fig):
    from hydromodel_amd.stepper import enkf_noise_analysis_of, split_enkf_noise_table
    cfg, D, P, mpp = r["cfg"], r["D"], r["P"], r["mpp"]
    dz, root, W = r["cols"].dz, cfg["method"] == "sqrt", Y.shape[1]
    z_a, forecast = r["z_a"], r["forecast"]
    stats, rej = split_enkf_noise_table(r["nzt"], D)
    assert r["Kz"].shape == (P, W, D) and not np.array_equal(z_a, z_f) and np.isfinite(z_a).all()
    Kx, Krx, shx = _exact_gains(z_f, Y, o_vec, sig, zeta, dz, cfg["loc"], mpp, root)
    parts = [enkf_noise_analysis_of(forecast[p * mpp:(p + 1) * mpp], z_f[p * mpp:(p + 1) * mpp], Y[p * mpp:(p + 1) * mpp],
                                    o_vec, sig, None if E is None else E[p * mpp:(p + 1) * mpp], zeta=zeta, dz=dz,
                                    localisation_cm=cfg["loc"], method=cfg["method"], relaxation=r["alpha_z"])
             for p in range(P)]
    fig.gain(r["Kz"], np.stack([q["K"] for q in parts]), Kx.transpose(0, 2, 1), "Kz")
    if root:
        fig.gain(r["Krz"], np.stack([q["Kr"] for q in parts]), Krx.transpose(0, 2, 1), "Krz")
        fig.gain(r["shift_z"], np.stack([q["shift"] for q in parts]), shx, "shift_z")
    for p, q in enumerate(parts):
        sl = slice(p * mpp, (p + 1) * mpp)
        for i in range(W):
            assert (r["cfg"]["wide"] and i == 4) or np.abs(r["Kz"][p, i]).max() > 0.0, (p, i)
        err = float(np.max(np.abs(z_a[sl] - q["z"]) / np.maximum(1.0, np.abs(q["z"]))))
        fig.note(f"z[{p}]", err)
        assert err <= 1e-9, (fig.head, p, err)
        assert not q["rejected"].any() and not q["psi_rejected"].any() and rej[p, 1] == 0
        err = max(float(np.abs(stats[p, 1, k] - q["stats"][k]).max()) for k in range(4))
        fig.note(f"noise table[{p}]", err)
        assert err <= 1e-10, (fig.head, p, err)
        blend = (1.0 - r["alpha_z"]) * q["sigma_a"] + r["alpha_z"] * q["sigma_b"]   # what the relaxation is for
        assert np.abs(z_a[sl].std(axis=0, ddof=1) - blend).max() <= 1e-9 * q["sigma_b"].max()
        assert np.isnan(stats[p, 2:6]).all() and np.isnan(rej[p, 2:]).all() and np.isnan(rej[p, 0])


def _case(D, node, tag, mpp=depths.MPP):
    r = _run(D, node, tag, mpp)
    z_f = None
    if r["alpha_z"] is not None:
        twin = _run(D, node, tag, mpp, twin=True)
        _same(twin["forecast"], r["forecast"], "forecast")            # the twin run is this run up to the analysis
        z_f = twin["z_f"]
    _check(r, z_f)


@pytest.mark.parametrize("tag", list(depths.CONFIGS))
@pytest.mark.parametrize("D, node", depths.CASES)
def test_analysis_against_numpy_at_every_slot_count(D, node, tag):
    _case(D, node, tag)


@pytest.mark.parametrize("tag", ["S9", "R9"])
def test_two_tiles_of_members_at_the_deepest_column(tag):
    """300 members a point: two tiles of 256, the second holding 44; with D + m' = 649 columns the partial buffer's rows
    are 649 * 9 long."""
    D, node = depths.CASES[-1]
    assert D == depths.MAX_D and -(-300 // 256) == 2 and 300 - 256 == 44
    _case(D, node, tag, mpp=300)


def test_one_member_per_point_keeps_its_state_at_the_deepest_column():
    """D = 640, two points of one member, m' = 9 with the taper and the relaxation on: no covariance, so the gains are 0,
    the state is the forecast to the bit and the row's log-density is that of independent Gaussians of the errors."""
    D, node = depths.CASES[-1]
    r = _run(D, node, "S9", mpp=1, noise_field=False)
    dz = r["cols"].dz
    _same(r["post"], r["forecast"])
    assert r["width"] == depths.ENKF_OBS and r["K"].shape == (2, D, 9) and np.all(r["K"] == 0.0) and np.all(r["K0"] == 0.0)
    o_vec, sig, _ = _observations(r)
    Y = np.concatenate([r["Ys"], r["Yw"]], axis=1)
    for p in range(2):
        t = r["table"][p, 1]
        d = o_vec - Y[p]
        want = float(np.sum(-0.5 * np.log(2.0 * np.pi * sig * sig) - 0.5 * d * d / (sig * sig)))
        assert t[0] == 1 and t[2] == 0.0 and t[6] == 0.0 and t[1] == r["y"][p] and t[5] == r["y"][p] and t[7] == 0
        assert t[3] == r["node"] * dz - r["y"][p]
        assert abs(t[4] - want) <= 1e-13 * max(1.0, abs(want))
        s, w = r["smt"][p, 1], r["wt"][p, 1]
        assert (s[:, 0] == 1.0).all() and (s[:, 3] == 0.0).all() and (s[:, 5] == 0.0).all()
        assert np.array_equal(s[:, 2], r["theta_f"][p]) and np.array_equal(s[:, 4], r["theta_f"][p])
        assert (w[:, 0] == 1.0).all() and (w[:, 3] == 0.0).all() and np.array_equal(w[:, 2], r["Yw"][p])


@pytest.mark.parametrize("D, node", [c for c in depths.CASES if c[0] in (64, 65, 640)])
def test_the_refusal_path_keeps_every_column_at_the_padding_edges(D, node):
    """sigma_cm = 1e200 (test_gpu_enkf_noise.test_a_member_whose_psi_analysis_is_rejected_keeps_its_vector): S has no
    Cholesky factor, the gain is NaN and the vote refuses every member -- with nine padding slots (D = 64), a last slot of
    one node (D = 65) and none (D = 640), m' = 9 and the noise field on.  Arithmetic on non-finite numbers, nothing else."""
    r = _run(D, node, "S9", sigma=1e200)
    twin = _run(D, node, "S9", sigma=1e200, twin=True)
    _same(twin["forecast"], r["forecast"], "forecast")
    _same(r["post"], r["forecast"], "state")
    assert r["width"] == depths.ENKF_OBS and np.isnan(r["K"]).all() and np.isnan(r["Kz"]).all()
    assert (r["table"][:, 1, 7] == r["mpp"]).all() and (r["table"][:, 1, 0] == r["mpp"]).all()
    _same(r["z_a"], twin["z_f"], "base vectors")
    assert (r["nzt"][:, 1, -1] == 0).all() and np.isfinite(r["nzt"][:, 1, :4 * D]).all()
