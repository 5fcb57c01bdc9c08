"""The noise field in the EnKF's analysis, without a GPU (include/hydrocol.h hc_set_enkf_noise_field): the entries; the
NumPy restatement ``stepper.enkf_noise_analysis_of`` against the dense formula written out here, both schemes; the
square-root scheme's variance identity; the relaxation's blended spread; the rejection rules; the CLI's ``Noise_Field``
key and its refusals; the summary's keys and shapes."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

from hydromodel_amd.cli import ENKF_KEYS, enkf_noise_settings, run_cli
from hydromodel_amd.stepper import (enkf_noise_analysis_of, enkf_noise_summary, gaspari_cohn, noise_field_settings,
                                    split_enkf_noise_table)

REPO = Path(__file__).resolve().parent.parent
NEW_ENTRIES = ("hc_set_enkf_noise_field", "hc_get_enkf_noise_field", "hc_get_enkf_noise_stats", "hc_set_enkf_noise_stats",
               "hc_get_enkf_noise_gain", "hc_get_enkf_noise_sqrt_gain", "hc_get_enkf_noise_sqrt_shift",
               "hc_get_enkf_noise_base", "hc_set_enkf_noise_base")


def test_header_declares_and_the_binding_lists_the_new_entries():
    text = (REPO / "include" / "hydrocol.h").read_text()
    from hydromodel_amd import _lib as L
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in L.EXPORTS, name
    for cited in ("src/simulation.py:561,592", "599-601", "vrettas_fung.py:154"):
        assert cited in text, cited
    assert "Noise_Field" in ENKF_KEYS


# ---- the restatement -----------------------------------------------------------------------------------------------------
N, D, DZ = 100, 7, 5.0


def _case(W, seed):
    """Random fields z, states that depend on them, and observations that depend non-linearly on the states."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((N, D))
    psi = -150.0 + 25.0 * np.cumsum(z, axis=1) + 10.0 * rng.standard_normal((N, D))
    Y = np.empty((N, W))
    Y[:, 0] = 14.0 + 6.0 * np.tanh(psi[:, 2] / 60.0 + 2.0) + 0.01 * psi[:, 5] + 0.3 * rng.standard_normal(N)
    for i in range(1, W):
        Y[:, i] = 0.25 + 0.1 / (1.0 + np.exp(-psi[:, i] / 50.0 - 3.0)) + 0.004 * rng.standard_normal(N)
    obs = np.concatenate([[15.0], 0.3 + 0.01 * rng.standard_normal(W - 1)])
    sigma = np.concatenate([[2.0], rng.uniform(0.01, 0.03, W - 1)])
    zeta = np.arange(1, W) * DZ                       # the other columns' taper centres: nodes 1, 2, ...
    eps = rng.standard_normal((N, W))
    return psi, z, Y, obs, sigma, zeta, eps


def _dense(z, Y, obs, sigma, zeta, loc):
    """K = (rho o C_zY)(rho o C_YY + R)^-1 with an explicit inverse."""
    A, B = z - z.mean(axis=0), Y - Y.mean(axis=0)
    czy, cyy = A.T @ B / (N - 1), B.T @ B / (N - 1)
    zt = np.concatenate([[Y[:, 0].mean()], zeta])
    depth = np.arange(D) * DZ
    if loc > 0:
        czy = czy * gaspari_cohn(np.abs(depth[:, None] - zt[None, :]) / loc)
        cyy = cyy * gaspari_cohn(np.abs(zt[:, None] - zt[None, :]) / loc)
    S = cyy + np.diag(sigma ** 2)
    return czy @ np.linalg.inv(S), czy, S


@pytest.mark.parametrize("loc", [0.0, 12.0])
@pytest.mark.parametrize("W", [1, 4])
def test_the_stochastic_restatement_is_the_dense_formula(W, loc):
    psi, z, Y, obs, sigma, zeta, eps = _case(W, seed=10 + W)
    res = enkf_noise_analysis_of(psi, z, Y, obs, sigma, eps, zeta=zeta, dz=DZ, localisation_cm=loc)
    K, _, _ = _dense(z, Y, obs, sigma, zeta, loc)
    assert res["K"].shape == (W, D) and np.abs(res["K"].T - K).max() <= 1e-12 * np.abs(K).max()
    want = z + ((obs + sigma * eps) - Y) @ K.T
    assert np.abs(res["z"] - want).max() <= 1e-12 * np.abs(want).max()
    assert not res["rejected"].any() and not res["psi_rejected"].any() and (res["factor"] == 1.0).all()
    assert np.array_equal(res["stats"][0], z.mean(axis=0)) and np.array_equal(res["stats"][1], z.std(axis=0, ddof=1))
    assert np.array_equal(res["stats"][2], res["z"].mean(axis=0))
    assert np.array_equal(res["stats"][3], res["z"].std(axis=0, ddof=1))
    if loc > 0:                                       # a node 2 L and more from every centre gets no increment
        far = np.abs(np.arange(D)[:, None] * DZ - np.concatenate([[Y[:, 0].mean()], zeta])[None, :]) >= 2 * loc
        assert (res["K"].T[far.all(axis=1)] == 0.0).all()


@pytest.mark.parametrize("loc", [0.0, 12.0])
@pytest.mark.parametrize("W", [1, 4])
def test_the_square_root_restatement_is_the_dense_formula(W, loc):
    psi, z, Y, obs, sigma, zeta, _ = _case(W, seed=20 + W)
    res = enkf_noise_analysis_of(psi, z, Y, obs, sigma, zeta=zeta, dz=DZ, localisation_cm=loc, method="sqrt")
    K, czy, S = _dense(z, Y, obs, sigma, zeta, loc)
    Lc = np.linalg.cholesky(S)
    Kr = czy @ np.linalg.inv(Lc.T) @ np.linalg.inv(Lc + np.diag(sigma))
    assert np.abs(res["K"].T - K).max() <= 1e-12 * np.abs(K).max()
    assert np.abs(res["Kr"].T - Kr).max() <= 1e-12 * np.abs(Kr).max()
    yb = Y.mean(axis=0)
    shift = K @ (obs - yb)
    assert np.abs(res["shift"] - shift).max() <= 1e-12 * np.abs(shift).max()
    want = z + shift[None, :] + (yb[None, :] - Y) @ Kr.T
    assert np.abs(res["z"] - want).max() <= 1e-12 * np.abs(want).max()
    # the mean moves by the full gain
    assert np.abs(res["z"].mean(axis=0) - (z.mean(axis=0) + shift)).max() <= 1e-12


@pytest.mark.parametrize("W", [1, 4])
def test_the_square_root_scheme_never_widens_a_node(W):
    """Without taper and relaxation the posterior covariance is C_zz - K C_Yz: its diagonal is at most the prior's."""
    psi, z, Y, obs, sigma, zeta, _ = _case(W, seed=30 + W)
    res = enkf_noise_analysis_of(psi, z, Y, obs, sigma, zeta=zeta, dz=DZ, method="sqrt")
    prior, post = z.var(axis=0, ddof=1), res["z"].var(axis=0, ddof=1)
    assert (post <= prior * (1.0 + 1e-12)).all() and (post < prior).any()
    K, czy, _ = _dense(z, Y, obs, sigma, zeta, 0.0)
    want = prior - np.einsum("di,di->d", K, czy)
    assert np.abs(post - want).max() <= 1e-12 * prior.max()


@pytest.mark.parametrize("method", ["stochastic", "sqrt"])
@pytest.mark.parametrize("alpha", [0.25, 0.5, 1.0])
def test_the_relaxation_gives_the_blended_spread(method, alpha):
    psi, z, Y, obs, sigma, zeta, eps = _case(4, seed=41)
    plain = enkf_noise_analysis_of(psi, z, Y, obs, sigma, eps, zeta=zeta, dz=DZ, method=method)
    res = enkf_noise_analysis_of(psi, z, Y, obs, sigma, eps, zeta=zeta, dz=DZ, method=method, relaxation=alpha)
    sb, sa = z.std(axis=0, ddof=1), plain["z"].std(axis=0, ddof=1)
    assert np.array_equal(res["sigma_b"], sb) and np.array_equal(res["sigma_a"], sa)
    want = (1.0 - alpha) * sa + alpha * sb
    assert np.abs(res["z"].std(axis=0, ddof=1) - want).max() <= 1e-12 * sb.max()
    assert np.abs(res["z"].mean(axis=0) - plain["z"].mean(axis=0)).max() <= 1e-12
    assert np.array_equal(res["K"], plain["K"]) and np.array_equal(res["stats"][3], res["z"].std(axis=0, ddof=1))


def test_the_rejection_rules():
    psi, z, Y, obs, sigma, zeta, eps = _case(4, seed=5)
    # a member whose psi analysis is not finite keeps its z to the bit and is not counted
    bad_eps = eps.copy()
    bad_eps[7, 0] = np.inf
    res = enkf_noise_analysis_of(psi, z, Y, obs, sigma, bad_eps, zeta=zeta, dz=DZ, relaxation=0.5)
    assert res["psi_rejected"].tolist() == [k == 7 for k in range(N)] and not res["rejected"].any()
    assert np.array_equal(res["z"][7], z[7]) and not np.array_equal(res["z"][8], z[8])
    # a non-finite entry in one member's z: node 3's mean, gain and every member's candidate are NaN -- every member keeps
    # its vector and is counted; the psi analysis stands
    zz = z.copy()
    zz[11, 3] = np.inf
    res = enkf_noise_analysis_of(psi, zz, Y, obs, sigma, eps, zeta=zeta, dz=DZ, relaxation=0.5)
    assert res["rejected"].all() and not res["psi_rejected"].any()
    assert np.array_equal(res["z"][:, [0, 1, 2, 4, 5, 6]][np.arange(N) != 11], zz[:, [0, 1, 2, 4, 5, 6]][np.arange(N) != 11])
    assert res["z"][11, 3] == np.inf and np.isnan(res["K"][:, 3]).all() and np.isfinite(res["K"][:, 2]).all()


# ---- the key ---------------------------------------------------------------------------------------------------------------
def _ens(**enkf):
    return {"Members": 8, "EnKF": {"Sigma_cm": 10.0, **enkf}}


@pytest.mark.parametrize("ens, want", [
    ({"Members": 8}, None),
    (_ens(), None),
    (_ens(Noise_Field=False), None),
    (_ens(Noise_Field=True), 0.0),
    (_ens(Noise_Field=True, Relaxation=0.3), 0.3),                       # the default is the block's
    (_ens(Noise_Field={"Relaxation": 0.5}, Relaxation=0.3), 0.5),
    (_ens(Noise_Field={"Relaxation": 0}), 0.0),
    (_ens(Noise_Field={"Relaxation": 1}), 1.0),
    (dict(_ens(Noise_Field=True, Sharded=True), Points=[{}, {}]), 0.0),    # a sweep ignores Sharded
    (_ens(Noise_Field=False, Sharded=True, Stride=0), None),
])
def test_noise_settings_accepts(ens, want):
    got = enkf_noise_settings(ens)
    assert got == want and (got is None or isinstance(got, float))


REFUSALS = [
    (_ens(Noise_Field=1), "EnKF.Noise_Field = 1 must be true, false or"),
    (_ens(Noise_Field="yes"), "EnKF.Noise_Field = 'yes' must be true, false or"),
    (_ens(Noise_Field=None), "EnKF.Noise_Field = None must be true, false or"),
    (_ens(Noise_Field={}), "EnKF.Noise_Field = {} must be true, false or"),
    (_ens(Noise_Field={"Relaxation": 0.5, "Seed": 1}), "must be true, false or"),
    (_ens(Noise_Field={"relaxation": 0.5}), "must be true, false or"),
    (_ens(Noise_Field={"Relaxation": -0.1}), "Noise_Field relaxation = -0.1 must be a finite number in [0, 1]"),
    (_ens(Noise_Field={"Relaxation": 1.5}), "Noise_Field relaxation = 1.5 must be a finite number in [0, 1]"),
    (_ens(Noise_Field={"Relaxation": float("nan")}), "Noise_Field relaxation = nan must be a finite number in [0, 1]"),
    (_ens(Noise_Field={"Relaxation": True}), "Noise_Field relaxation = True must be a number in [0, 1]"),
    (_ens(Noise_Field={"Relaxation": "0.5"}), "Noise_Field relaxation = '0.5' must be a number in [0, 1]"),
    (_ens(Noise_Field=True, Stride=0), "EnKF.Noise_Field needs an active EnKF (EnKF.Stride > 0)"),
    ({"Members": 8, "Noise_Field": True}, "Noise_Field belongs inside the \"EnKF\" block"),
    (dict(_ens(Noise_Field=True, Sharded=True), GPUs=2), "the partials the ranks exchange cover psi only"),
    (_ens(Noise_Field={"Relaxation": 0.5}, Sharded=True), "the partials the ranks exchange cover psi only"),
]


@pytest.mark.parametrize("ens, message", REFUSALS)
def test_noise_settings_rejects(ens, message):
    with pytest.raises(ValueError) as err:
        enkf_noise_settings(ens)
    assert message in str(err.value)


@pytest.mark.parametrize("ens, message", [REFUSALS[0], REFUSALS[7], REFUSALS[9], REFUSALS[11], REFUSALS[13]])
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


def test_the_python_argument_takes_the_same_forms():
    assert noise_field_settings(None) is None and noise_field_settings(False) is None
    assert noise_field_settings(True, 0.25) == 0.25 and noise_field_settings({"relaxation": 0.5}, 0.25) == 0.5
    for bad in (1, "on", {"relaxation": 2}, {"relaxation": True}, {"a": 1}, {}):
        with pytest.raises(ValueError):
            noise_field_settings(bad)


# ---- the summary ---------------------------------------------------------------------------------------------------------
def _table(lead, n_arow, Dn, slots):
    rng = np.random.default_rng(3)
    t = np.full(lead + (n_arow, 4 * Dn + 1), np.nan)
    for j in slots:
        stats = rng.uniform(0.5, 1.5, lead + (4, Dn))
        stats[..., 3, :] = 0.5 * stats[..., 1, :]                   # posterior std: half the prior's
        t[..., j, :4 * Dn] = stats.reshape(lead + (4 * Dn,))
        t[..., j, 4 * Dn] = j
    return t


@pytest.mark.parametrize("lead", [(), (3,)])
def test_summary_keys_and_shapes(lead):
    Dn = 6
    t = _table(lead, 5, Dn, slots=(1, 3))
    stats, rej = split_enkf_noise_table(t, Dn)
    assert stats.shape == lead + (5, 4, Dn) and rej.shape == lead + (5,)
    s = enkf_noise_summary(t, 24, 0.5)
    assert set(s) == {"rows", "noise_prior_mean", "noise_prior_std", "noise_post_mean", "noise_post_std", "noise_rejected",
                      "noise_spread_ratio", "noise_relaxation"}
    assert s["rows"].tolist() == [24, 72] and s["noise_relaxation"] == 0.5
    for k in ("noise_prior_mean", "noise_prior_std", "noise_post_mean", "noise_post_std"):
        assert s[k].shape == lead + (2, Dn), k
    assert s["noise_rejected"].shape == lead + (2,) and s["noise_rejected"].dtype == np.int64
    assert (s["noise_rejected"] == np.array([1, 3])).all()
    assert abs(s["noise_spread_ratio"] - 0.5) <= 1e-15
    empty = enkf_noise_summary(np.full(lead + (5, 4 * Dn + 1), np.nan), 24, 0.0)
    assert empty["rows"].size == 0 and np.isnan(empty["noise_spread_ratio"])


def test_hdf5_dataset_names_of_an_ensemble_and_a_sweep():
    """cli._reduce_enkf_noise on one rank, from a stand-in for the handle: the dataset names and their shapes."""
    from hydromodel_amd import cli

    class Ranks:
        rank, world = 0, 1

        def allreduce_sum(self, x):
            return x

    class Sim:
        def __init__(self, t):
            self.t = t

        def assim_table(self, key):
            assert key == "enkf_noise"
            return self.t

    Dn, T = 6, 97                                        # 97 rows, stride 24: slots 0 ... 4
    keys = {"enkf_noise_field", "enkf_noise_relaxation", "enkf_noise_prior_mean", "enkf_noise_prior_std",
            "enkf_noise_post_mean", "enkf_noise_post_std", "enkf_noise_rejected"}
    for lead, ids, keep in (((), [0], False), ((3,), [0, 1, 2], True)):
        t = _table(lead, 5, Dn, slots=(1, 2, 3, 4))
        P = lead[0] if lead else 1
        out, line = cli._reduce_enkf_noise(Ranks(), Sim(t), ids, P, T, Dn, (24, 5.0, 0.0, None), 0.5, "Ensemble x8", keep)
        assert set(out) == keys and int(out["enkf_noise_field"]) == 1 and float(out["enkf_noise_relaxation"]) == 0.5
        for k in ("enkf_noise_prior_mean", "enkf_noise_prior_std", "enkf_noise_post_mean", "enkf_noise_post_std"):
            assert out[k].shape == lead + (4, Dn), k
        assert out["enkf_noise_rejected"].shape == lead + (4,)
        assert line == " [Ensemble x8] EnKF noise field: posterior spread 0.5000 of prior over 4 rows"
    assert cli._reduce_enkf_noise(Ranks(), None, [], 1, T, Dn, (24, 5.0, 0.0, None), None, "x", False) == ({}, None)
