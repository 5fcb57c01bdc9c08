"""Soil-moisture distributions, the parts that need no GPU: the NumPy restatement of the device's binning
(stepper.theta_hist_of), the quantile bands formed from a table (stepper.theta_distribution) and the CLI's
"Ensemble": {"Profile_Distribution": ...} block (include/hydrocol.h hc_set_theta_hist)."""
import json
import re

import numpy as np
import pytest

from hydromodel_amd.cli import profile_distribution_settings, run_cli
from hydromodel_amd.stepper import theta_distribution, theta_hist_of


# ---- 1. the binning --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [32, 64, 128])
def test_hand_made_values_land_in_their_bins(B):
    edge = 5.0 / B                                         # a bin edge: exact, B is a power of two
    values = [0.0, -0.0, np.nextafter(edge, 0.0), edge, np.nextafter(1.0, 0.0), 1.0,          # counted
              1.0 + 2.0 ** -52, np.nan, -2.0 ** -1074, np.inf, -np.inf, 2.0]                  # outside
    want = [0, 0, 4, 5, B - 1, B - 1]
    theta = np.array(values)[:, None]                      # [N][1]: every value a member of one node
    hist, outside = theta_hist_of(theta, B)
    assert hist.shape == (1, B) and hist.dtype == np.int64
    assert outside == len(values) - len(want)
    expect = np.zeros(B, dtype=np.int64)
    np.add.at(expect, want, 1)
    assert np.array_equal(hist[0], expect)
    for v, b in zip(values, want):                         # and one at a time
        h, o = theta_hist_of(np.array([[v]]), B)
        assert o == 0 and h[0, b] == 1 and h.sum() == 1, (v, b)
    for v in values[len(want):]:
        h, o = theta_hist_of(np.array([[v]]), B)
        assert o == 1 and h.sum() == 0, v


@pytest.mark.parametrize("B", [32, 128])
def test_bins_plus_outside_sum_to_the_members_at_every_node(B):
    rng = np.random.default_rng(3)
    N, D = 67, 9
    theta = rng.uniform(-0.1, 1.1, (N, D))
    theta[rng.integers(0, N, 5), rng.integers(0, D, 5)] = np.nan
    hist, outside = theta_hist_of(theta, B)
    inside = (theta >= 0) & (theta <= 1)
    assert np.array_equal(hist.sum(axis=1), inside.sum(axis=0)) and outside == int((~inside).sum())
    assert np.array_equal(hist.sum(axis=1) + (~inside).sum(axis=0), np.full(D, N))
    for i in range(D):                                     # against numpy's own histogram of the node's values
        ref, _ = np.histogram(theta[inside[:, i], i], bins=B, range=(0.0, 1.0))
        assert np.array_equal(hist[i], ref)


def test_other_bin_counts_are_refused():
    for B in (0, 48, 256):
        with pytest.raises(ValueError, match="32, 64 or 128"):
            theta_hist_of(np.zeros((2, 2)), B)


# ---- 2. the quantile bands -------------------------------------------------------------------------------------------
LEVELS = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)


@pytest.mark.parametrize("B", [32, 64, 128])
def test_quantiles_agree_with_numpys_inverted_cdf_of_the_bin_centres(B):
    rng = np.random.default_rng(B)
    R, D = 4, 6
    hist = np.zeros((R, D, B), dtype=np.int32)
    for r in range(R):
        for i in range(D):
            few = rng.choice(B, size=rng.integers(1, 6), replace=False)          # members of a node sit in a few bins
            hist[r, i, few] = rng.integers(1, 40, few.size)
    d = theta_distribution(hist, LEVELS, B, stride=48)
    assert d["quantiles"].shape == (R, len(LEVELS), D) and d["rows"].tolist() == [0, 48, 96, 144]
    centres = (np.arange(B) + 0.5) / B
    for r in range(R):
        for i in range(D):
            members = np.repeat(centres, hist[r, i])
            for l, p in enumerate(LEVELS):
                assert d["quantiles"][r, l, i] == np.quantile(members, p, method="inverted_cdf"), (r, i, p)
    # levels 0 and 1: the lowest and the highest occupied bin
    occupied = hist > 0
    assert np.array_equal(d["quantiles"][:, 0], (np.argmax(occupied, axis=-1) + 0.5) / B)
    assert np.array_equal(d["quantiles"][:, -1], (B - 1 - np.argmax(occupied[..., ::-1], axis=-1) + 0.5) / B)


def test_an_empty_row_gives_nan_and_a_point_axis_is_kept():
    B = 32
    hist = np.zeros((2, 3, 4, B), dtype=np.int32)          # [P][R][D][B]
    hist[:, 0, :, 7] = 5
    hist[:, 2, :, 9] = 3
    hist[1, 2, :, 31] = 3
    d = theta_distribution(hist, [0.5, 1.0])
    assert d["quantiles"].shape == (2, 3, 2, 4) and d["count"].tolist() == [[5, 0, 3], [5, 0, 6]]
    assert np.isnan(d["quantiles"][:, 1]).all() and np.isnan(d["saturated_fraction"][:, 1]).all()
    assert np.all(d["quantiles"][:, 0] == 7.5 / B) and np.all(d["quantiles"][0, 2] == 9.5 / B)
    assert np.all(d["quantiles"][1, 2, 0] == 9.5 / B) and np.all(d["quantiles"][1, 2, 1] == 31.5 / B)
    # the highest bin occupied on any row: 9 for point 0, 31 for point 1
    assert np.all(d["saturated_fraction"][0, 0] == 0.0) and np.all(d["saturated_fraction"][0, 2] == 1.0)
    assert np.all(d["saturated_fraction"][1, 2] == 0.5)


def test_distribution_refuses_bad_tables_and_levels():
    hist = np.zeros((1, 2, 32), dtype=np.int32)
    with pytest.raises(ValueError, match="at most 16 quantile levels"):
        theta_distribution(hist, np.linspace(0, 1, 17))
    with pytest.raises(ValueError, match="each in"):
        theta_distribution(hist, [1.5])
    with pytest.raises(ValueError, match="32, 64 or 128"):
        theta_distribution(np.zeros((1, 2, 48), dtype=np.int32), [0.5])
    with pytest.raises(ValueError, match="64 were named"):
        theta_distribution(hist, [0.5], 64)


# ---- 3. the CLI's block ----------------------------------------------------------------------------------------------
def _ens(block, **other):
    return {"Members": 8, "Profiles": 48, "Profile_Distribution": block, **other}


@pytest.mark.parametrize("ens, want", [
    ({"Members": 8}, (0, None)),
    ({"Members": 8, "Profiles": 48}, (0, None)),
    (_ens({"Quantiles": [0.05, 0.5, 0.95]}), (128, (0.05, 0.5, 0.95))),
    (_ens({"Bins": 32, "Quantiles": [0, 1]}, Profiles=1), (32, (0.0, 1.0))),
    (_ens({"Bins": 64, "Quantiles": [0.5]}), (64, (0.5,))),
])
def test_settings_accepts(ens, want):
    assert profile_distribution_settings(ens) == want


@pytest.mark.parametrize("ens, message", [
    ({"Members": 8, "Profile_Distribution": {"Quantiles": [0.5]}}, "Profile_Distribution needs the profile rows: Profiles = 0"),
    (_ens({"Quantiles": [0.5]}, Profiles=0), "Profile_Distribution needs the profile rows: Profiles = 0"),
    (_ens({"Quantiles": [0.5]}, Profiles=-3), "Profile_Distribution needs the profile rows: Profiles = -3"),
    (_ens({"Quantiles": [0.5]}, Profiles="48"), "Profile_Distribution needs the profile rows: Profiles = '48'"),
    (_ens({"Bins": 48, "Quantiles": [0.5]}), "Profile_Distribution.Bins = 48 must be 32, 64 or 128"),
    (_ens({"Bins": 256, "Quantiles": [0.5]}), "Profile_Distribution.Bins = 256 must be 32, 64 or 128"),
    (_ens({"Bins": 0, "Quantiles": [0.5]}), "Profile_Distribution.Bins = 0 must be 32, 64 or 128"),
    (_ens({"Bins": "128", "Quantiles": [0.5]}), "Profile_Distribution.Bins = '128' must be 32, 64 or 128"),
    (_ens({"Bins": True, "Quantiles": [0.5]}), "Profile_Distribution.Bins = True must be 32, 64 or 128"),
    (_ens({"Bins": 128}), "Profile_Distribution.Quantiles (a list of levels in [0, 1]) is required"),
    (_ens({"Quantiles": []}), "Profile_Distribution.Quantiles = [] must be a non-empty list"),
    (_ens({"Quantiles": 0.5}), "Profile_Distribution.Quantiles = 0.5 must be a non-empty list"),
    (_ens({"Quantiles": [0.5, 1.5]}), "Profile_Distribution.Quantiles: 1.5 lies outside [0, 1]"),
    (_ens({"Quantiles": [-0.1]}), "Profile_Distribution.Quantiles: -0.1 lies outside [0, 1]"),
    (_ens({"Quantiles": ["0.5"]}), "Profile_Distribution.Quantiles: '0.5' is not a number"),
    (_ens({"Quantiles": [True]}), "Profile_Distribution.Quantiles: True is not a number"),
    (_ens({"Quantiles": [float("nan")]}), "Profile_Distribution.Quantiles: nan is not a number"),
    (_ens({"Quantiles": [k / 16 for k in range(17)]}), "Profile_Distribution.Quantiles holds 17 levels; at most 16"),
    (_ens({"Quantiles": [0.5], "Stride": 48}), "Profile_Distribution has unknown keys ['Stride']"),
    (_ens(128), "Profile_Distribution = 128 must be an object"),
])
def test_settings_rejects(ens, message):
    with pytest.raises(ValueError, match=re.escape(message)):
        profile_distribution_settings(ens)


@pytest.mark.parametrize("ens, message", [
    ({"Members": 8, "Profile_Distribution": {"Quantiles": [0.5]}}, "Profile_Distribution needs the profile rows"),
    (_ens({"Bins": 48, "Quantiles": [0.5]}), "Profile_Distribution.Bins = 48"),
    (_ens({"Quantiles": [2]}), "Profile_Distribution.Quantiles: 2 lies outside"),
])
def test_a_bad_block_ends_the_command_with_status_1_before_any_gpu_call(tmp_path, capsys, ens, message):
    from hydromodel_amd.synthetic import default_parameters
    params = default_parameters()
    params["Data_Filename"] = str(tmp_path / "missing.csv")          # never reached: the block is refused first
    params["Ensemble"] = ens
    (tmp_path / "p.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as stop:
        run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "p.json")])
    assert stop.value.code == 1
    out = capsys.readouterr().out
    assert message in out and "missing.csv" not in out
