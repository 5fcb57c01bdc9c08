"""The members' forcing state in the EnKF's analysis without a GPU (include/hydrocol.h hc_set_enkf_forcing): the NumPy
restatement against a literal per-member loop with a long-double gain; who keeps their g; the gain without a taper beside
an S that has one; the settings, their checkpoint round trip and their refusals before a handle exists; the CLI's key; the
table's split and summary."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

from hydromodel_amd.cli import forcing_perturbation_settings as cli_settings, run_cli
from hydromodel_amd.stepper import (_enkf_gains_of, enkf_forcing_analysis_of, enkf_forcing_summary, forcing_enkf_settings,
                                    forcing_perturbation_settings, gaspari_cohn, split_enkf_forcing_table)

REPO = Path(__file__).resolve().parents[1]
D, DZ = 9, 10.0
PERT = {"precipitation_sigma": 0.3, "demand_sigma": 0.1, "correlation_days": 3.0}


def test_header_declares_and_the_binding_lists_the_new_entries():
    from hydromodel_amd import _lib
    header = (REPO / "include" / "hydrocol.h").read_text()
    names = ("hc_set_enkf_forcing", "hc_get_enkf_forcing", "hc_get_enkf_g_table", "hc_set_enkf_g_table", "hc_get_enkf_g_gain",
             "hc_get_enkf_g_sqrt_gain", "hc_get_enkf_g_sqrt_shift")
    for name in names:
        assert re.search(rf"^int {name}\(", header, flags=re.M) and name in _lib.EXPORTS, name
    assert not [n for n in _lib.EXPORTS if "enkf_g_" in n and n.endswith("_stats")]      # not an ASSIM_TABLES entry
    assert "the EnKF leaves g alone unless hc_set_enkf_forcing" in header


def _case(N, W, seed):
    """psi [N][D], g [N][2], Y [N][W] that depends on both, observations, errors, taper centres and draws."""
    rng = np.random.default_rng(seed)
    psi = rng.standard_normal((N, D)) * 20.0 - 100.0
    g = rng.standard_normal((N, 2))
    Y = np.stack([30.0 + 0.2 * psi[:, 2 + k] + (4.0 - k) * g[:, 0] - 2.0 * g[:, 1] + rng.standard_normal(N)
                  for k in range(W)], axis=1)
    obs = Y.mean(axis=0) + rng.standard_normal(W) * 3.0
    sigma = 1.0 + rng.random(W)
    zeta = [25.0 + 15.0 * k for k in range(W - 1)]
    return psi, g, Y, obs, sigma, zeta, rng.standard_normal((N, W))


def _literal(g, Y, obs, sigma, zeta, loc, eps, method, alpha):
    """The issue's formulas, one member and one entry at a time: the covariances as explicit sums, S with its taper, the gain
    in long double through an explicit inverse (no taper on C_gY), the update per member, the relaxation per stream."""
    ld = np.longdouble
    N, W = Y.shape
    gb, yb = g.astype(ld).sum(axis=0) / N, Y.astype(ld).sum(axis=0) / N
    cgy, cyy = np.zeros((2, W), ld), np.zeros((W, W), ld)
    for m in range(N):
        for i in range(W):
            for s in range(2):
                cgy[s, i] += (ld(g[m, s]) - gb[s]) * (ld(Y[m, i]) - yb[i])
            for k in range(W):
                cyy[i, k] += (ld(Y[m, i]) - yb[i]) * (ld(Y[m, k]) - yb[k])
    cgy, cyy = cgy / (N - 1), cyy / (N - 1)
    zt = np.concatenate([[float(yb[0])], zeta])
    S = np.zeros((W, W), ld)
    for i in range(W):
        for k in range(W):
            rho = gaspari_cohn(abs(zt[i] - zt[k]) / loc) if loc > 0 else 1.0
            S[i, k] = ld(rho) * cyy[i, k] + (ld(sigma[i]) ** 2 if i == k else 0)
    # S^-1 by Gauss-Jordan in long double
    A = np.concatenate([S, np.eye(W, dtype=ld)], axis=1)
    for i in range(W):
        A[i] = A[i] / A[i, i]
        for k in range(W):
            if k != i:
                A[k] = A[k] - A[k, i] * A[i]
    K = cgy @ A[:, W:]                                                   # [2][W]
    out = np.array(g, dtype=np.float64)
    if method == "stochastic":
        for m in range(N):
            for s in range(2):
                out[m, s] = g[m, s] + float(sum(K[s, j] * (ld(obs[j]) + ld(sigma[j]) * ld(eps[m, j]) - ld(Y[m, j]))
                                                for j in range(W)))
        Kr = shift = None
    else:
        L = np.linalg.cholesky(S.astype(np.float64)).astype(ld)
        # Kr = C_gY L^-T (L + R^1/2)^-1 with explicit long-double inverses of the two triangular factors
        def inverse(T):
            B = np.concatenate([T, np.eye(W, dtype=ld)], axis=1)
            for i in range(W):
                B[i] = B[i] / B[i, i]
                for k in range(W):
                    if k != i:
                        B[k] = B[k] - B[k, i] * B[i]
            return B[:, W:]
        Kr = cgy @ inverse(L.T) @ inverse(L + np.diag(np.asarray(sigma, dtype=ld)))
        shift = K @ (np.asarray(obs, dtype=ld) - yb)
        for m in range(N):
            for s in range(2):
                out[m, s] = g[m, s] + float(shift[s] + sum(Kr[s, j] * (yb[j] - ld(Y[m, j])) for j in range(W)))
    sb, sa = g.std(axis=0, ddof=1), out.std(axis=0, ddof=1)
    if alpha > 0:
        mean = out.mean(axis=0)
        for s in range(2):
            f = 1.0 + alpha * (sb[s] - sa[s]) / sa[s]
            out[:, s] = mean[s] + f * (out[:, s] - mean[s])
    return (K.astype(np.float64).T, None if Kr is None else Kr.astype(np.float64).T,
            None if shift is None else shift.astype(np.float64), out, sb, sa)


@pytest.mark.parametrize("alpha", [0.0, 0.5])
@pytest.mark.parametrize("method", ["stochastic", "sqrt"])
@pytest.mark.parametrize("W", [1, 4])
@pytest.mark.parametrize("N", [7, 300])
def test_the_restatement_is_the_literal_per_member_loop(N, W, method, alpha):
    psi, g, Y, obs, sigma, zeta, eps = _case(N, W, seed=N + W)
    loc = 40.0
    res = enkf_forcing_analysis_of(psi, g, Y, obs, sigma, eps, zeta=zeta, dz=DZ, localisation_cm=loc, method=method,
                                   relaxation=alpha)
    K, Kr, shift, want, sb, sa = _literal(g, Y, obs, sigma, zeta, loc, eps, method, alpha)
    # float64 against long double: the m' x m' solve's conditioning times a few eps; 1e-10 is the project's bar for gains
    assert res["K"].shape == (W, 2) and np.abs(res["K"] - K).max() <= 1e-10 * np.abs(K).max()
    if method == "sqrt":
        assert np.abs(res["Kr"] - Kr).max() <= 1e-10 * np.abs(Kr).max()
        assert np.abs(res["shift"] - shift).max() <= 1e-10 * max(np.abs(shift).max(), 1.0)
    assert np.abs(res["g"] - want).max() <= 1e-9 and not np.array_equal(res["g"], g)
    assert np.abs(res["sigma_b"] - sb).max() <= 1e-12 and np.abs(res["sigma_a"] - sa).max() <= 1e-9
    assert not res["rejected"].any() and not res["psi_rejected"].any()
    assert np.allclose(res["stats"][0], g.mean(axis=0), atol=1e-14) and np.allclose(res["stats"][2], res["g"].mean(axis=0))
    if alpha:
        blend = (1.0 - alpha) * res["sigma_a"] + alpha * res["sigma_b"]
        assert np.abs(res["g"].std(axis=0, ddof=1) - blend).max() <= 1e-12


def test_an_inactive_stream_and_a_psi_rejected_member_keep_their_g_to_the_bit():
    psi, g, Y, obs, sigma, zeta, eps = _case(60, 4, seed=5)
    for method in ("stochastic", "sqrt"):
        res = enkf_forcing_analysis_of(psi, g, Y, obs, sigma, eps, active=(True, False), zeta=zeta, dz=DZ, method=method,
                                       relaxation=0.5)
        assert res["g"][:, 1].tobytes() == g[:, 1].tobytes() and not np.array_equal(res["g"][:, 0], g[:, 0])
        assert np.array_equal(res["stats"][2:, 1], res["stats"][:2, 1])                  # post = prior
        assert not np.array_equal(res["stats"][2:, 0], res["stats"][:2, 0])
    bad = eps.copy()
    bad[7, 0] = np.inf                                                  # member 7's psi analysis is not finite
    res = enkf_forcing_analysis_of(psi, g, Y, obs, sigma, bad, zeta=zeta, dz=DZ, relaxation=0.5)
    assert res["psi_rejected"].tolist() == [k == 7 for k in range(60)] and not res["rejected"].any()
    assert res["g"][7].tobytes() == g[7].tobytes() and not np.array_equal(res["g"][8], g[8])


def test_a_non_finite_update_is_counted_and_not_applied():
    psi, g, Y, obs, sigma, zeta, eps = _case(60, 4, seed=6)
    gg = g.copy()
    gg[11, 0] = np.inf              # the precipitation stream's mean and gain are NaN: nobody can take the update
    res = enkf_forcing_analysis_of(psi, gg, Y, obs, sigma, eps, zeta=zeta, dz=DZ, relaxation=0.5)
    assert res["rejected"].all() and not res["psi_rejected"].any()
    assert res["g"].tobytes() == gg.tobytes()
    assert np.isnan(res["K"][:, 0]).all() and np.isfinite(res["K"][:, 1]).all()


def test_the_gain_has_no_taper_while_s_is_the_one_psi_is_analysed_with():
    psi, g, Y, obs, sigma, zeta, eps = _case(80, 4, seed=7)
    loc = 30.0
    # S as _enkf_gains_of forms it for psi: K_psi S = rho o C_psiY  =>  recover S's action through the gains of g
    K_tap, _, _, yb = _enkf_gains_of(g, Y, obs, sigma, zeta, DZ, loc, False)
    K_free, _, _, _ = _enkf_gains_of(g, Y, obs, sigma, zeta, DZ, loc, False, taper_x=False)
    res = enkf_forcing_analysis_of(psi, g, Y, obs, sigma, eps, zeta=zeta, dz=DZ, localisation_cm=loc)
    assert np.array_equal(res["K"], K_free.T) and not np.allclose(K_tap, K_free)
    A = Y - yb
    cyy, cgy = A.T @ A / 79.0, (g - g.mean(axis=0)).T @ A / 79.0
    zt = np.concatenate([[yb[0]], zeta])
    S = gaspari_cohn(np.abs(zt[:, None] - zt[None, :]) / loc) * cyy + np.diag(np.asarray(sigma) ** 2)
    assert np.abs(K_free @ S - cgy).max() <= 1e-12 * np.abs(cgy).max()                   # K^g S = C_gY, untapered
    K_psi = _enkf_gains_of(psi, Y, obs, sigma, zeta, DZ, loc, False)[0]
    rho = gaspari_cohn(np.abs(np.arange(D)[:, None] * DZ - zt[None, :]) / loc)
    cpy = (psi - psi.mean(axis=0)).T @ A / 79.0
    assert np.abs(K_psi @ S - rho * cpy).max() <= 1e-10 * np.abs(cpy).max()              # the same S serves psi, tapered
    assert np.array_equal(_enkf_gains_of(g, Y, obs, sigma, zeta, DZ, 0.0, False)[0],
                          _enkf_gains_of(g, Y, obs, sigma, zeta, DZ, 0.0, False, taper_x=False)[0])


# ---- the settings ----------------------------------------------------------------------------------------------------------
def test_the_dict_without_the_key_is_the_four_keys_it_was():
    want = {"precipitation_sigma": 0.3, "demand_sigma": 0.1, "correlation_days": 3.0, "seed": None}
    assert forcing_perturbation_settings(PERT) == want
    assert forcing_perturbation_settings(dict(PERT, enkf_relaxation=None)) == want
    assert forcing_perturbation_settings(dict(PERT, enkf_relaxation=0.0)) == dict(want, enkf_relaxation=0.0)
    assert forcing_perturbation_settings(dict(PERT, enkf_relaxation=1)) == dict(want, enkf_relaxation=1.0)
    for bad in (True, -0.1, 1.5, float("nan"), "0.5"):
        with pytest.raises(ValueError, match="relaxation"):
            forcing_perturbation_settings(dict(PERT, enkf_relaxation=bad))


@pytest.fixture(scope="module")
def site():
    from helpers import digest
    _, cols, forcing = digest(1)
    return cols, forcing


def test_the_settings_round_trip_through_the_checkpoints_datasets(site):
    from hydromodel_amd import settings
    kw = dict(enkf_stride=24, enkf_sigma_cm=5.0, forcing_perturbation=dict(PERT, enkf_relaxation=0.25))
    first = settings.normalise("EnsembleSimulation", kw, [site[0]], 6)
    assert first.on["forcing_enkf"] and first.forcing_perturbation["enkf_relaxation"] == 0.25
    data = settings.checkpoint_datasets(first)
    assert data["forcing_enkf_relaxation"].dtype == np.float64 and float(data["forcing_enkf_relaxation"]) == 0.25
    again = settings.checkpoint_keywords({k: np.asarray(v) for k, v in data.items()}, "ck.h5")
    assert again["forcing_perturbation"] == {"precipitation_sigma": 0.3, "demand_sigma": 0.1, "correlation_days": 3.0,
                                             "seed": 6, "enkf_relaxation": 0.25}
    second = settings.normalise("EnsembleSimulation", again, [site[0]], 6)
    assert second.forcing_perturbation == first.forcing_perturbation and second.on == first.on
    plain = settings.normalise("EnsembleSimulation", dict(kw, forcing_perturbation=PERT), [site[0]], 6)
    assert not plain.on["forcing_enkf"] and "forcing_enkf_relaxation" not in settings.checkpoint_datasets(plain)
    assert "enkf_relaxation" not in plain.forcing_perturbation
    starts = [option for option, _ in settings.START]
    assert starts.index("forcing_enkf") == starts.index("enkf_noise_field") + 1
    assert "forcing_enkf" in [option for option, _, _ in settings.RUN_STATE]


class Recorder:
    """The stand-in for ``EnsembleStepper`` of test_run_settings_cpu.py's kind: it logs the calls by name."""
    calls, made = [], 0

    def __init__(self, cols, forcing, n, device=0, flags=None):
        type(self).made += 1
        self.P, self.N, self.D = 1, int(n), cols.dim_d
        self.filter_shard = None

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*args, **kw):
            type(self).calls.append((name, args))
            return np.zeros(self.N)
        return call


@pytest.fixture
def recorder(monkeypatch):
    from hydromodel_amd import ensemble
    Recorder.calls, Recorder.made = [], 0
    monkeypatch.setattr(ensemble, "EnsembleStepper", Recorder)
    return Recorder


def test_the_call_is_made_only_with_the_key_after_the_noise_field(site, recorder):
    from hydromodel_amd.ensemble import EnsembleSimulation
    psi0 = np.linspace(-300.0, 100.0, site[0].dim_d)
    kw = dict(seed=6, psi0=psi0, enkf_stride=24, enkf_sigma_cm=5.0, enkf_noise_field=True)
    EnsembleSimulation(site[0], site[1], 8, forcing_perturbation=PERT, **kw)
    assert "set_enkf_forcing" not in [c[0] for c in recorder.calls]
    recorder.calls = []
    EnsembleSimulation(site[0], site[1], 8, forcing_perturbation=dict(PERT, enkf_relaxation=0.25), **kw)
    names = [c[0] for c in recorder.calls]
    assert names.index("set_enkf_forcing") == names.index("set_enkf_noise_field") + 1
    assert dict(recorder.calls)["set_enkf_forcing"] == (True, 0.25)


@pytest.mark.parametrize("kw, message", [
    (dict(forcing_perturbation=dict(PERT, enkf_relaxation=0.25)), "needs the EnKF (enkf_stride > 0)"),
    (dict(enkf_stride=24, enkf_sigma_cm=5.0, enkf_shard=(8, None), forcing_perturbation=dict(PERT, enkf_relaxation=0.25)),
     "enkf_shard and the forcing analysis exclude each other: the exchanged partials cover psi only"),
    (dict(enkf_stride=24, enkf_sigma_cm=5.0, forcing_perturbation=dict(PERT, enkf_relaxation=1.5)),
     "must be a finite number in [0, 1]"),
    (dict(enkf_stride=24, enkf_sigma_cm=5.0, forcing_perturbation=dict(PERT, enkf_relaxation=True)),
     "must be a number in [0, 1]"),
])
def test_a_refusal_fires_before_any_handle_exists(kw, message, site, recorder):
    from hydromodel_amd.ensemble import EnsembleSimulation
    with pytest.raises(ValueError) as err:
        EnsembleSimulation(site[0], site[1], 8, seed=6, **kw)
    assert message in str(err.value) and recorder.made == 0


# ---- the CLI's key ---------------------------------------------------------------------------------------------------------
BLOCK = {"Precipitation_Sigma": 0.3, "Demand_Sigma": 0.1, "Correlation_Days": 3}


def _ens(value="absent", enkf={"Sigma_cm": 10.0}, **more):
    block = dict(BLOCK) if value == "absent" else dict(BLOCK, EnKF=value)
    ens = {"Members": 8, "Seed": 4, "Forcing_Perturbation": block, **more}
    if enkf is not None:
        ens["EnKF"] = dict(enkf)
    return ens


FOUR = {"precipitation_sigma": 0.3, "demand_sigma": 0.1, "correlation_days": 3.0, "seed": 4}


@pytest.mark.parametrize("ens, want", [
    (_ens(), None),
    (_ens(False), None),
    (_ens(False, enkf=None), None),
    (_ens(True), 0.0),
    (_ens(True, enkf={"Sigma_cm": 10.0, "Relaxation": 0.3}), 0.3),             # true takes the EnKF block's
    (_ens({"Relaxation": 0.5}, enkf={"Sigma_cm": 10.0, "Relaxation": 0.3}), 0.5),
    (_ens({"Relaxation": 0}), 0.0),
    (_ens({"Relaxation": 1}), 1.0),
    (_ens(True, enkf={"Sigma_cm": 10.0, "Sharded": True}, Points=[{}, {}]), 0.0),  # a sweep ignores Sharded
])
def test_the_cli_key_parses(ens, want):
    got = cli_settings(ens)
    assert got == (FOUR if want is None else dict(FOUR, enkf_relaxation=want))


REFUSALS = [
    (_ens(1), "Forcing_Perturbation.EnKF = 1 must be true, false or"),
    (_ens("yes"), "Forcing_Perturbation.EnKF = 'yes' must be true, false or"),
    (_ens(None), "Forcing_Perturbation.EnKF = None must be true, false or"),
    (_ens({}), "Forcing_Perturbation.EnKF = {} must be true, false or"),
    (_ens({"Relaxation": 0.5, "Seed": 1}), "Forcing_Perturbation.EnKF has unknown keys ['Seed']"),
    (_ens({"relaxation": 0.5}), "Forcing_Perturbation.EnKF has unknown keys ['relaxation']"),
    (_ens({"Relaxation": -0.1}), "relaxation = -0.1 must be a finite number in [0, 1]"),
    (_ens({"Relaxation": 1.5}), "relaxation = 1.5 must be a finite number in [0, 1]"),
    (_ens({"Relaxation": True}), "relaxation = True must be a number in [0, 1]"),
    (_ens(True, enkf=None), "Forcing_Perturbation.EnKF needs an active \"EnKF\" block"),
    (_ens(True, enkf={"Sigma_cm": 10.0, "Stride": 0}), "Forcing_Perturbation.EnKF needs an active \"EnKF\" block"),
    (_ens(True, enkf=None, Filter={"Sigma_cm": 10.0}), "Forcing_Perturbation.EnKF with a \"Filter\" block"),
    (_ens(True, enkf={"Sigma_cm": 10.0, "Sharded": True}), "the partials the ranks exchange cover psi only"),
    (_ens({"Relaxation": 0.5}, enkf={"Sigma_cm": 10.0, "Sharded": True}, GPUs=2), "the partials the ranks exchange cover psi only"),
]


@pytest.mark.parametrize("ens, message", REFUSALS)
def test_the_cli_key_is_refused(ens, message):
    with pytest.raises(ValueError) as err:
        cli_settings(ens)
    assert message in str(err.value)


@pytest.mark.parametrize("ens, message", [REFUSALS[0], REFUSALS[4], REFUSALS[8], REFUSALS[9], REFUSALS[11], REFUSALS[12]])
def test_a_bad_key_ends_the_command_with_status_1_before_any_gpu_call(tmp_path, capsys, monkeypatch, ens, message):
    from hydromodel_amd import ensemble
    from hydromodel_amd.synthetic import default_parameters

    def no_gpu(*a, **k):
        raise AssertionError("a GPU handle was created")
    monkeypatch.setattr(ensemble, "EnsembleStepper", no_gpu)
    monkeypatch.delenv("RANK", raising=False)
    params = default_parameters()
    params["Data_Filename"] = str(tmp_path / "missing.csv")          # never reached: the block is refused first
    params["Ensemble"] = ens
    (tmp_path / "p.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as stop:
        run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "p.json")])
    assert stop.value.code == 1
    out = capsys.readouterr().out
    assert message in out and "missing.csv" not in out


def test_the_python_form_of_the_key():
    assert forcing_enkf_settings(None) is None and forcing_enkf_settings(False) is None
    assert forcing_enkf_settings(True, 0.25) == 0.25 and forcing_enkf_settings({"Relaxation": 0.5}, 0.25) == 0.5
    for bad in (1, "on", {"Relaxation": 2}, {"Relaxation": True}, {"a": 1}, {}):
        with pytest.raises(ValueError):
            forcing_enkf_settings(bad)


# ---- the table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [(), (3,)])
def test_split_and_summary_on_a_hand_made_table(lead):
    t = np.full(lead + (6, 9), np.nan)
    row = np.array([0.1, 1.0, 0.3, 0.5, -0.2, 2.0, -0.1, 1.0, 2.0])      # stream 0: columns 0-3, stream 1: 4-7, refused
    t[..., 1, :], t[..., 4, :] = row, row * np.array([1, 1, 1, 0.5, 1, 1, 1, 0.5, 0])
    stats, rej = split_enkf_forcing_table(t)
    assert stats.shape == lead + (6, 4, 2) and rej.shape == lead + (6,)
    assert stats[..., 1, :, 0].reshape(-1, 4)[0].tolist() == [0.1, 1.0, 0.3, 0.5]
    assert stats[..., 1, :, 1].reshape(-1, 4)[0].tolist() == [-0.2, 2.0, -0.1, 1.0]
    s = enkf_forcing_summary(t, 24, 0.25)
    assert s["rows"].tolist() == [24, 96] and s["forcing_relaxation"] == 0.25
    for k in ("forcing_prior_mean", "forcing_prior_std", "forcing_post_mean", "forcing_post_std"):
        assert s[k].shape == lead + (2, 2), k
    assert s["forcing_rejected"].shape == lead + (2,) and s["forcing_rejected"].reshape(-1, 2)[0].tolist() == [2, 0]
    assert np.allclose(s["forcing_spread_ratio"], [(0.5 + 0.25) / 2, (0.5 + 0.25) / 2])
    empty = enkf_forcing_summary(np.full(lead + (6, 9), np.nan), 24, 0.0)
    assert empty["rows"].size == 0 and np.isnan(empty["forcing_spread_ratio"]).all()
