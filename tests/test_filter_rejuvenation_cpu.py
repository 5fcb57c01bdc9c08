"""Rejuvenation of the particle filter's base noise vectors (include/hydrocol.h hc_set_filter_rejuvenation), the parts
that need no GPU: the shrinkage from the discount, the NumPy restatement's moments within bounds derived from the two
sampling terms, distinct rows after the move, the finiteness vote, the trigger, the summary's keys, the CLI's
"Filter": {"Rejuvenation": ...} key with its refusals, and the exported symbols."""
import json
from fractions import Fraction

import numpy as np
import pytest

from hydromodel_amd.cli import FILTER_KEYS, filter_rejuvenation, filter_settings, run_cli
from hydromodel_amd.stepper import (REJUV_WIDTH, filter_rejuvenation_of, filter_summary, rejuvenation_discount,
                                    rejuvenation_shrinkage)

D = 101


def _resampled(N, distinct, seed):
    """[N][D] vectors of which only ``distinct`` differ, in runs as a monotone ancestry leaves them; and eps [N][D]"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((distinct, D)) * rng.uniform(0.2, 3.0, size=D)[None, :] + rng.uniform(-2, 2, size=D)[None, :]
    anc = np.sort(rng.integers(0, distinct, size=N))
    return x[anc], rng.standard_normal((N, D))


# ---- 1. the shrinkage ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta, exact", [(0.95, Fraction(37, 38)), (0.75, Fraction(5, 6))])
def test_shrinkage_of_the_discount(delta, exact):
    a, h = rejuvenation_shrinkage(delta)
    assert a == (3.0 * delta - 1.0) / (2.0 * delta)              # every operation rounded once, in this order
    assert h == float(np.sqrt(1.0 - a * a))
    assert abs(a - float(exact)) <= 2.3e-16                       # one ulp of a number below 1
    assert abs(a * a + h * h - 1.0) <= 4.5e-16
    assert 0.0 < h < 1.0 and 0.0 < a < 1.0


def test_the_edges_of_the_discount():
    assert rejuvenation_shrinkage(0.5) == (0.5, float(np.sqrt(0.75)))
    assert rejuvenation_discount(0) == 0.0 and rejuvenation_discount(None) == 0.0 and rejuvenation_discount(0.5) == 0.5
    assert rejuvenation_discount(np.float64(0.9)) == 0.9
    for bad in (1.0, 0.4999, -0.5, 1.5, float("nan"), float("inf"), True, False, "0.9", [0.9]):
        with pytest.raises(ValueError, match="filter rejuvenation = .* must be"):
            rejuvenation_discount(bad)
    with pytest.raises(ValueError, match="off"):
        rejuvenation_shrinkage(0.0)


# ---- 2. the moments are what the resampling left ------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [0.95, 0.75])
@pytest.mark.parametrize("N, distinct", [(100, 9), (256, 40), (2500, 130)])
def test_mean_and_variance_are_preserved_within_the_sampling_bounds(N, distinct, delta):
    """With z' = mean + a (z - mean) + h s eps the sample variance of a node is s^2 (a^2 + h^2 V + 2 a h C): V the sample
    variance of N standard normals (standard deviation sqrt(2 / N)), C their sample covariance with the standardised
    anomalies (1 / sqrt(N)).  So var' / s^2 - 1 has standard deviation sqrt((2 h^4 + 4 a^2 h^2) / N), and mean' - mean =
    h s mean(eps) has h s / sqrt(N).  Six of each."""
    z, eps = _resampled(N, distinct, seed=N + distinct)
    assert np.unique(z, axis=0).shape[0] <= distinct < N
    out = filter_rejuvenation_of(z, eps, delta)
    a, h = out["a"], out["h"]
    assert out["applied"] and not out["refused"].any()
    s, s_after = out["s"], out["s_after"]
    assert np.allclose(out["mean"], z.mean(axis=0), rtol=0, atol=1e-12) and np.allclose(s, z.std(axis=0, ddof=1), rtol=1e-12)
    var_bar = 6.0 * np.sqrt((2.0 * h ** 4 + 4.0 * a * a * h * h) / N)
    mean_bar = 6.0 * h * s.max() / np.sqrt(N)
    var_err = np.abs(s_after ** 2 / s ** 2 - 1.0).max()
    mean_err = np.abs(out["z"].mean(axis=0) - out["mean"]).max()
    print(f"\n N_p = {N}, delta = {delta}: variance {var_err / var_bar:.2f} of its bar, mean {mean_err / mean_bar:.2f}")
    assert var_err <= var_bar and mean_err <= mean_bar
    assert np.unique(out["z"], axis=0).shape[0] == N                                # no two members share a field
    row = out["row"]
    assert row.shape == (REJUV_WIDTH,) and row[0] == 1.0 and row[1] == 0.0
    assert row[2] == np.sqrt((s * s).sum() / D) and row[3] == np.sqrt((s_after * s_after).sum() / D)
    assert abs(row[3] / row[2] - 1.0) <= var_bar                                    # (sqrt halves a relative error)


# ---- 3. the vote --------------------------------------------------------------------------------------------------------
def test_a_member_whose_new_vector_is_not_finite_keeps_its_own_and_is_counted():
    z, eps = _resampled(100, 9, seed=5)
    eps[3, 50], eps[77, 0] = np.inf, np.nan
    out = filter_rejuvenation_of(z, eps, 0.95)
    assert out["refused"].nonzero()[0].tolist() == [3, 77] and out["row"][1] == 2.0 and out["row"][0] == 1.0
    assert np.array_equal(out["z"][[3, 77]], z[[3, 77]])
    others = np.delete(np.arange(100), [3, 77])
    assert np.isfinite(out["z"]).all() and not (out["z"][others] == z[others]).all(axis=1).any()
    assert np.isfinite(out["row"]).all()


# ---- 4. the trigger -----------------------------------------------------------------------------------------------------
def test_an_identity_ancestry_or_no_survivor_leaves_every_vector():
    rng = np.random.default_rng(1)
    z, eps = rng.standard_normal((64, D)), rng.standard_normal((64, D))
    for survivors in (None, 64, 0):
        out = filter_rejuvenation_of(z, eps, 0.9, survivors=survivors)
        assert not out["applied"] and out["z"].tobytes() == z.tobytes()
        assert out["row"][:2].tolist() == [0.0, 0.0] and np.isnan(out["row"][2:]).all()
    assert filter_rejuvenation_of(z, eps, 0.9, survivors=63)["applied"]
    one = filter_rejuvenation_of(z[:1], eps[:1], 0.9)                               # N_p = 1: s = 0, survivors = N_p
    assert not one["applied"] and not one["s"].any()
    # a single survivor: s = 0, the move is applied and restores nothing
    same = filter_rejuvenation_of(np.repeat(z[:1], 10, axis=0), eps[:10], 0.9)
    assert same["applied"] and not same["s"].any() and np.unique(same["z"], axis=0).shape[0] == 1


# ---- 5. the summary -----------------------------------------------------------------------------------------------------
def test_the_summary_gains_the_rejuvenation_keys():
    nan = float("nan")
    table = np.array([[0, nan, nan, nan], [50, 20.0, -3.0, 31], [50, 50.0, -1.0, 50], [0, nan, nan, nan]])
    rtable = np.array([[nan] * 4, [1.0, 2.0, 0.9, 0.89], [0.0, 0.0, nan, nan], [nan] * 4])
    s = filter_summary(table, 48, 5.0, rejuvenation_table=rtable)
    assert s["rows"].tolist() == [48, 96] and s["rejuvenated"].tolist() == [1, 0] and s["rejuvenated_rows"] == 1
    assert s["rejuvenation_refused"].tolist() == [2, 0] and s["noise_std_resampled"][0] == 0.9
    assert s["noise_std_rejuvenated"][0] == 0.89 and np.isnan(s["noise_std_rejuvenated"][1])
    assert "rejuvenated" not in filter_summary(table, 48, 5.0)
    sweep = filter_summary(np.stack([table, table]), 48, 5.0, rejuvenation_table=np.stack([rtable, rtable]))
    assert sweep["rejuvenated"].shape == (2, 2) and sweep["rejuvenated_rows"].tolist() == [1, 1]


# ---- 6. the CLI's key ---------------------------------------------------------------------------------------------------
def _ens(**filt):
    return {"Members": 8, "Filter": {"Sigma_cm": 10.0, **filt}}


def test_the_key_parses_and_leaves_the_filters_tuple():
    assert "Rejuvenation" in FILTER_KEYS
    assert filter_rejuvenation(_ens(Rejuvenation=0.95)) == 0.95 and filter_settings(_ens(Rejuvenation=0.95), 1) == (48, 10.0, None)
    assert filter_rejuvenation(_ens(Rejuvenation=0.5, Stride=24, ESS_floor=0.25)) == 0.5
    assert filter_rejuvenation(_ens()) is None and filter_rejuvenation({"Members": 8}) is None
    pts = [{"Soil_Properties": {"n": 1.6}}, {"Soil_Properties": {"n": 2.4}}]
    assert filter_rejuvenation({**_ens(Rejuvenation=0.9, Sharded=True), "Points": pts}) == 0.9     # a sweep ignores Sharded


@pytest.mark.parametrize("ens, message", [
    (_ens(Rejuvenation=0), "Filter.Rejuvenation = 0 must be a finite number with 0.5 <= Rejuvenation < 1"),
    (_ens(Rejuvenation=1), "Filter.Rejuvenation = 1 must be"),
    (_ens(Rejuvenation=0.49), "Filter.Rejuvenation = 0.49 must be"),
    (_ens(Rejuvenation=-0.9), "Filter.Rejuvenation = -0.9 must be"),
    (_ens(Rejuvenation=float("nan")), "Filter.Rejuvenation = nan must be"),
    (_ens(Rejuvenation=float("inf")), "Filter.Rejuvenation = inf must be"),
    (_ens(Rejuvenation="0.9"), "Filter.Rejuvenation = '0.9' must be"),
    (_ens(Rejuvenation=None), "Filter.Rejuvenation = None must be"),
    (_ens(Rejuvenation=True), "Filter.Rejuvenation = True must be a finite number with 0.5 <= Rejuvenation < 1"),
    (_ens(Rejuvenation=False), "Filter.Rejuvenation = False must be"),
    (_ens(Rejuvenation=0.9, Stride=0), "Filter.Rejuvenation needs an active filter (Filter.Stride > 0)"),
    (_ens(Rejuvenation=0.9, Sharded=True), "Filter.Rejuvenation is not available with \"Sharded\": true"),
    ({"Members": 8, "Rejuvenation": 0.9}, "Rejuvenation belongs inside the \"Filter\" block"),
    ({"Members": 8, "Rejuvenation": 0.9, "Filter": {"Sigma_cm": 10.0}}, "Rejuvenation belongs inside the \"Filter\" block"),
    (_ens(rejuvenation=0.9), "Filter has unknown keys ['rejuvenation']"),
])
def test_the_key_rejects(ens, message):
    with pytest.raises(ValueError) as err:
        filter_settings(ens, 2 if ens.get("Filter", {}).get("Sharded") else 1)
    assert message in str(err.value)
    with pytest.raises(ValueError):
        filter_rejuvenation(ens)


def test_a_bad_key_ends_the_cli_with_status_1_before_any_gpu_call(tmp_path, capsys):
    from hydromodel_amd.synthetic import default_parameters
    params = default_parameters()
    params["Data_Filename"] = str(tmp_path / "missing.csv")
    params["Ensemble"] = {"Members": 64, "Days": 1, "Filter": {"Sigma_cm": 10.0, "Rejuvenation": 1.0}}
    (tmp_path / "p.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as status:
        run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "p.json")])
    assert status.value.code == 1
    assert "Filter.Rejuvenation = 1.0 must be a finite number with 0.5 <= Rejuvenation < 1" in capsys.readouterr().out


# ---- 7. the library's side ----------------------------------------------------------------------------------------------
def test_the_entry_points_are_bound():
    from hydromodel_amd import _lib
    for name in ("hc_set_filter_rejuvenation", "hc_get_filter_rejuvenation", "hc_get_filter_rejuvenation_stats",
                 "hc_set_filter_rejuvenation_stats", "hc_get_filter_rejuvenation_moments",
                 "hc_filter_rejuvenation_normals"):
        assert name in _lib.EXPORTS, name
