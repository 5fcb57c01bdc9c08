"""The EnKF's square-root analysis and its relaxation to prior spread on the host (no GPU): the C-ABI entries, the CLI's
"Method" / "Relaxation" validator and its refusals before any GPU call, and a float64 NumPy restatement of both (used by
the GPU tests too) checked against the identities that define them (include/hydrocol.h hc_set_enkf_method)."""
import inspect
import json
import re
from pathlib import Path

import numpy as np
import pytest

from hydromodel_amd.cli import ENKF_KEYS, enkf_method_settings, enkf_settings, run_cli, soil_moisture_settings
from hydromodel_amd.stepper import ENKF_METHODS, gaspari_cohn

REPO = Path(__file__).resolve().parent.parent
NEW_ENTRIES = ("hc_set_enkf_method", "hc_get_enkf_method", "hc_get_enkf_sqrt_gain", "hc_get_enkf_sqrt_shift",
               "hc_get_enkf_relaxation")


def sqrt_analysis_restated(psi, Y, o, R, zeta_nodes, dz, loc, mpp):
    """The square-root analysis per point in float64 (include/hydrocol.h hc_set_enkf_method): the covariances, taper and
    Cholesky factor L of S = rho o C_YY + R as the stochastic analysis forms them; K = c S^-1; dbar = K (o - Ybar);
    Kr = c L^-T (L + R^1/2)^-1; psi + dbar + (Ybar - Y) Kr^T.  Nothing is drawn: there is no eps argument.
    psi [N][D], Y [N][m'], o / R [m']."""
    N, D = psi.shape
    W = Y.shape[1]
    P = N // mpp
    z = np.arange(D) * dz
    K, Kr, dbar, ybar = np.zeros((P, D, W)), np.zeros((P, D, W)), np.zeros((P, D)), np.zeros((P, W))
    post = psi.copy()
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        yb = Y[sl].mean(axis=0)
        A = Y[sl] - yb
        n1 = mpp - 1
        cyy = A.T @ A / n1 if mpp > 1 else np.zeros((W, W))
        cpy = (psi[sl] - psi[sl].mean(axis=0)).T @ A / n1 if mpp > 1 else np.zeros((D, W))
        zeta = np.concatenate([[yb[0]], np.asarray(zeta_nodes, dtype=np.float64)])
        if loc > 0:
            rho_yy = gaspari_cohn(np.abs(zeta[:, None] - zeta[None, :]) / loc)
            rho_py = gaspari_cohn(np.abs(z[:, None] - zeta[None, :]) / loc)
        else:
            rho_yy, rho_py = np.ones((W, W)), np.ones((D, W))
        L = np.linalg.cholesky(rho_yy * cyy + np.diag(R))
        u = np.linalg.solve(L, (rho_py * cpy).T)                       # L^-1 c^T
        K[p] = np.linalg.solve(L.T, u).T
        M = L + np.diag(np.sqrt(R))
        Kr[p] = np.linalg.solve(M.T, u).T                              # x M = u^T
        dbar[p] = K[p] @ (o - yb)
        post[sl] = psi[sl] + dbar[p][None, :] + (yb[None, :] - Y[sl]) @ Kr[p].T
        ybar[p] = yb
    return {"K": K, "Kr": Kr, "dbar": dbar, "post": post, "ybar": ybar}


def rtps_restated(prior, post, alpha, mpp):
    """Relaxation to prior spread per point and node: sigma_b, sigma_a (N_p - 1; N_p = 1: 0), f = 1 + alpha (sigma_b -
    sigma_a) / sigma_a (1 where sigma_a is 0 or not finite), mean + f (post - mean); a node with f = 1 keeps its bits.
    prior / post [N][D] -> sigma_b, sigma_a, f [P][D], relaxed [N][D]."""
    N, D = post.shape
    P = N // mpp
    sb, sa, f = np.zeros((P, D)), np.zeros((P, D)), np.ones((P, D))
    out = post.copy()
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        if mpp > 1:
            sb[p], sa[p] = prior[sl].std(axis=0, ddof=1), post[sl].std(axis=0, ddof=1)
        good = (sa[p] > 0) & np.isfinite(sa[p])
        with np.errstate(divide="ignore", invalid="ignore"):
            f[p] = np.where(good, 1.0 + alpha * (sb[p] - sa[p]) / sa[p], 1.0)
        mean = post[sl].mean(axis=0)
        out[sl] = np.where(f[p][None, :] == 1.0, post[sl], mean[None, :] + f[p][None, :] * (post[sl] - mean[None, :]))
    return sb, sa, f, out


# ---- 1. the entries ----------------------------------------------------------------------------------------------------
def test_header_declares_and_the_binding_lists_the_new_entries():
    text = (REPO / "include" / "hydrocol.h").read_text()
    from hydromodel_amd import _lib as L
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in L.EXPORTS, name
    assert ENKF_METHODS == ("stochastic", "sqrt")


def test_the_enkf_validators_keep_their_results_with_the_new_keys_present():
    ens = {"Members": 8, "EnKF": {"Sigma_cm": 10.0, "Localisation_cm": 30, "Seed": 4, "Method": "sqrt", "Relaxation": 0.5}}
    assert enkf_settings(ens, 1) == (48, 10.0, 30.0, 4)
    assert soil_moisture_settings(ens, 1) is None
    assert "Method" in ENKF_KEYS and "Relaxation" in ENKF_KEYS
    with pytest.raises(ValueError, match=re.escape("EnKF has unknown keys ['method']")):
        enkf_settings({"Members": 8, "EnKF": {"Sigma_cm": 1.0, "method": "sqrt"}}, 1)


# ---- 2. the validator --------------------------------------------------------------------------------------------------
def _ens(**enkf):
    return {"Members": 8, "EnKF": {"Sigma_cm": 10.0, **enkf}}


@pytest.mark.parametrize("ens, want", [
    ({"Members": 8}, None),
    (_ens(), None),
    ({"Members": 8, "EnKF": None}, None),
    (_ens(Method="sqrt"), ("sqrt", 0.0)),
    (_ens(Method="stochastic"), ("stochastic", 0.0)),
    (_ens(Relaxation=0.5), ("stochastic", 0.5)),
    (_ens(Method="sqrt", Relaxation=1), ("sqrt", 1.0)),
    (_ens(Method="sqrt", Relaxation=0), ("sqrt", 0.0)),
    (dict(_ens(Method="sqrt", Relaxation=0.25), Points=[{}, {}]), ("sqrt", 0.25)),
])
def test_enkf_method_settings_accepts(ens, want):
    got = enkf_method_settings(ens)
    assert got == want and (got is None or isinstance(got[1], float))


@pytest.mark.parametrize("ens, message", [
    (_ens(Method="etkf"), "EnKF.Method = 'etkf' must be one of ['stochastic', 'sqrt']"),
    (_ens(Method="Sqrt"), "EnKF.Method = 'Sqrt' must be one of"),
    (_ens(Method=1), "EnKF.Method = 1 must be one of"),
    (_ens(Method=None), "EnKF.Method = None must be one of"),
    (_ens(Method=["sqrt"]), "EnKF.Method = ['sqrt'] must be one of"),
    (_ens(Relaxation=-0.1), "EnKF.Relaxation = -0.1 must be a finite number in [0, 1]"),
    (_ens(Relaxation=1.5), "EnKF.Relaxation = 1.5 must be a finite number in [0, 1]"),
    (_ens(Relaxation=float("nan")), "EnKF.Relaxation = nan must be a finite number in [0, 1]"),
    (_ens(Relaxation=float("inf")), "EnKF.Relaxation = inf must be a finite number in [0, 1]"),
    (_ens(Relaxation=True), "EnKF.Relaxation = True must be a finite number in [0, 1]"),
    (_ens(Relaxation="0.5"), "EnKF.Relaxation = '0.5' must be a finite number in [0, 1]"),
    (_ens(Relaxation=None), "EnKF.Relaxation = None must be a finite number in [0, 1]"),
    (_ens(Method="sqrt", Stride=0), "EnKF.Method / EnKF.Relaxation need an active EnKF (EnKF.Stride > 0)"),
])
def test_enkf_method_settings_rejects(ens, message):
    with pytest.raises(ValueError) as err:
        enkf_method_settings(ens)
    assert message in str(err.value)


@pytest.mark.parametrize("ens, message", [
    (_ens(Method="etkf"), "EnKF.Method = 'etkf' must be one of"),
    (_ens(Relaxation=2), "EnKF.Relaxation = 2 must be a finite number in [0, 1]"),
    (_ens(Relaxation=True), "EnKF.Relaxation = True must be a finite number"),
    (_ens(Relaxation=0.5, Stride=0), "need an active EnKF"),
    (dict(_ens(Method="sqrt"), GPUs=2), "EnKF with one parameter point runs on one GPU (2 requested)"),
])
def test_a_bad_method_block_ends_the_command_with_status_1_before_any_gpu_call(tmp_path, capsys, monkeypatch, ens,
                                                                                message):
    from hydromodel_amd import ensemble
    from hydromodel_amd.synthetic import default_parameters

    def no_gpu(*a, **k):
        raise AssertionError("a GPU handle was created")
    monkeypatch.setattr(ensemble, "EnsembleStepper", no_gpu)
    params = default_parameters()
    params["Data_Filename"] = str(tmp_path / "missing.csv")          # never reached: the block is refused first
    params["Ensemble"] = ens
    (tmp_path / "p.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as stop:
        run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "p.json")])
    assert stop.value.code == 1
    out = capsys.readouterr().out
    assert message in out and "missing.csv" not in out


# ---- 3. the restatement ------------------------------------------------------------------------------------------------
def _case(N, D, W, seed):
    """Random states and a NON-linear observation of them: y ~ a smooth function of a few nodes plus noise."""
    rng = np.random.default_rng(seed)
    base = np.cumsum(rng.standard_normal((N, D)), axis=1) * 3.0 - 200.0 + 40.0 * rng.standard_normal((N, 1))
    psi = base.copy()
    psi[:, D - 7:] = -3.25                                            # a saturated tail: every member agrees
    nodes = rng.choice(D - 10, size=W, replace=False)
    Y = np.empty((N, W))
    Y[:, 0] = 150.0 + 30.0 * np.tanh(psi[:, nodes[0]] / 80.0 + 2.0) + 0.02 * psi[:, D // 2] + rng.standard_normal(N)
    for i in range(1, W):
        Y[:, i] = 0.25 + 0.1 / (1.0 + np.exp(-psi[:, nodes[i]] / 50.0 - 3.0)) + 0.004 * rng.standard_normal(N)
    o = np.concatenate([[155.0], 0.3 + 0.01 * rng.standard_normal(W - 1)])
    R = np.concatenate([[25.0], rng.uniform(1e-4, 9e-4, W - 1)])
    return psi, Y, o, R, nodes[1:] * 5.0


@pytest.mark.parametrize("N", [100, 2500])
@pytest.mark.parametrize("D", [101, 300])
@pytest.mark.parametrize("W", [1, 4, 9])
def test_the_restated_square_root_analysis_has_the_kalman_mean_and_covariance(N, D, W):
    psi, Y, o, R, zeta = _case(N, D, W, seed=N + D + W)
    res = sqrt_analysis_restated(psi, Y, o, R, zeta, 5.0, 0.0, N)
    A, B = psi - psi.mean(axis=0), Y - Y.mean(axis=0)
    cpp, cpy, cyy = A.T @ A / (N - 1), A.T @ B / (N - 1), B.T @ B / (N - 1)
    K = cpy @ np.linalg.inv(cyy + np.diag(R))
    assert np.abs(res["K"][0] - K).max() <= 1e-10 * np.abs(K).max()
    mean = psi.mean(axis=0) + K @ (o - Y.mean(axis=0))
    err_mean = np.abs(res["post"].mean(axis=0) - mean).max() / np.abs(mean).max()
    Aa = res["post"] - res["post"].mean(axis=0)
    want = cpp - K @ cpy.T
    err_cov = np.abs(Aa.T @ Aa / (N - 1) - want).max() / np.abs(want).max()
    print(f" N={N} D={D} m'={W}: mean {err_mean:.1e}, covariance {err_cov:.1e}")
    assert err_mean <= 1e-12 and err_cov <= 1e-12
    assert np.array_equal(res["post"][:, D - 7:], psi[:, D - 7:])     # no spread, no covariance: untouched
    if W == 1:                                                        # Whitaker & Hamill's scalar form
        s = cyy[0, 0] + R[0]
        closed = res["K"][0, :, 0] / (1.0 + np.sqrt(R[0] / s))
        assert np.abs(res["Kr"][0, :, 0] - closed).max() <= 1e-13 * np.abs(closed).max()


def test_the_restated_square_root_analysis_takes_no_draws_and_tapers_like_the_stochastic_one():
    from test_enkf_sm_cpu import analysis_restated
    assert not {"E", "eps", "seed"} & set(inspect.signature(sqrt_analysis_restated).parameters)
    psi, Y, o, R, zeta = _case(80, 60, 3, seed=2)
    psi = np.concatenate([psi, psi[::-1] + 3.0])                      # two points of 80 members
    Y = np.concatenate([Y, Y[::-1] * 1.01])
    for loc in (0.0, 45.0):
        a = sqrt_analysis_restated(psi, Y, o, R, zeta, 5.0, loc, 80)
        b = analysis_restated(psi, Y, np.zeros_like(Y), o, R, zeta, 5.0, loc, 80)
        assert np.array_equal(a["K"], b["K"]) and np.array_equal(a["ybar"], b["ybar"])
        for p in range(2):                                            # the mean moves by the full gain
            sl = slice(80 * p, 80 * p + 80)
            want = psi[sl].mean(axis=0) + a["K"][p] @ (o - a["ybar"][p])
            assert np.abs(a["post"][sl].mean(axis=0) - want).max() <= 1e-12 * np.abs(want).max()
    one = sqrt_analysis_restated(psi[:1], Y[:1], o, R, zeta, 5.0, 0.0, 1)         # one member: nothing moves
    assert np.array_equal(one["post"], psi[:1]) and not one["Kr"].any() and not one["dbar"].any()


@pytest.mark.parametrize("N", [100, 2500])
@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
def test_the_restated_relaxation_gives_the_blended_spread_and_keeps_the_mean(N, alpha):
    D = 101
    psi, Y, o, R, zeta = _case(N, D, 4, seed=N)
    post = sqrt_analysis_restated(psi, Y, o, R, zeta, 5.0, 0.0, N)["post"]
    sb, sa, f, out = rtps_restated(psi, post, alpha, N)
    assert sb.shape == sa.shape == f.shape == (1, D) and np.isfinite(out).all()
    assert np.abs(sb[0] - psi.std(axis=0, ddof=1)).max() == 0.0 and (sa[0, D - 7:] == 0.0).all()
    want = (1.0 - alpha) * sa[0] + alpha * sb[0]
    err = np.abs(out.std(axis=0, ddof=1) - want).max() / sb.max()
    err_mean = np.abs(out.mean(axis=0) - post.mean(axis=0)).max() / np.abs(post.mean(axis=0)).max()
    print(f" N={N} alpha={alpha}: spread {err:.1e}, mean {err_mean:.1e}")
    assert err <= 1e-10 and err_mean <= 1e-12
    assert (f[0, D - 7:] == 1.0).all() and np.array_equal(out[:, D - 7:], post[:, D - 7:])   # sigma_a = 0: untouched
    assert (f[0, :D - 7] >= 1.0).all()                               # the analysis never widens the spread here
    if alpha == 0.0:
        assert np.array_equal(out, post)
    if alpha == 1.0:
        assert np.abs(out.std(axis=0, ddof=1) - sb[0]).max() <= 1e-10 * sb.max()
    sb1, sa1, f1, out1 = rtps_restated(psi[:1], post[:1], alpha, 1)   # one member: f = 1
    assert not sb1.any() and not sa1.any() and (f1 == 1.0).all() and np.array_equal(out1, post[:1])
