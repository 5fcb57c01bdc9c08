"""Period totals per member, the host side (no GPU): the NumPy restatements against hand-computed integers, mean and sigma
against exact fractions, the quantile rule against numpy.quantile(method="inverted_cdf"), the calendar ends of the
synthetic record, the CLI's "Ensemble": {"Periods": ...} block with every refusal, and the library's exports."""
import json
import re
import subprocess
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

from hydromodel_amd.cli import period_plan, period_settings, run_cli
from hydromodel_amd.stepper import (PERIOD_WTD_NONE, flux_max_log2_of, period_ends, period_solved_rows,
                                    period_totals_distribution, period_totals_of, period_totals_stats,
                                    period_totals_table_layout, profile_words_of, split_period_hist,
                                    split_period_totals_table)

S = 2.0 ** -32                           # one step of the row fluxes' quantisation


# ---- 1. the restatement, by hand ---------------------------------------------------------------------------------------
def _tiny():
    """Rows 1 .. 5 of two members; ends [2, 3, 5]; row 3 is skipped, so period 1 (its only row) counts nobody."""
    obs = np.array([7, 7, 7, -1, 7, 7])
    q = np.array([[[4096, 1], [8192, -3]],                     # row 1: q of (transpiration, lateral flow) per member
                  [[4095, 2], [1, -4094]],                     # row 2
                  [[999, 999], [999, 999]],                    # row 3: skipped
                  [[10, 20], [30, 40]],                        # row 4
                  [[5, 6], [7, 8]]], dtype=np.int64)           # row 5
    wtd = np.array([[10, 12], [9, 15], [0, 99], [11, 11], [13, 10]])
    return obs, q * S, wtd, [2, 3, 5]


def test_accumulators_tables_and_histograms_equal_the_hand_computed_integers():
    obs, diag, wtd, ends = _tiny()
    out = period_totals_of(diag, wtd, obs, ends, threshold_nodes=[10, 12], bins=32, flux_max_log2=(-8, -8), D=16)
    # the accumulators as each period ended: sums of q, min, max, rows with wtd <= 10 and <= 12
    assert out["acc_at_end"][0].tolist() == [[8191, 8193], [3, -4097], [9, 12], [10, 15], [2, 0], [2, 1]]
    assert out["acc_at_end"][1].tolist() == [[0, 0], [0, 0], [PERIOD_WTD_NONE] * 2, [0, 0], [0, 0], [0, 0]]
    assert out["acc_at_end"][2].tolist() == [[15, 37], [26, 48], [11, 10], [13, 11], [0, 1], [1, 2]]
    assert out["acc"].tolist() == out["acc_at_end"][1].tolist()         # reset after the last end
    parts = split_period_totals_table(out["table"], 1, 3, 6)
    assert parts["pcnt"].tolist() == [[2, 0, 2]] and parts["ovf"].tolist() == [0]
    # v = A >> 12 is floor: 8191 -> 1, 8193 -> 2, 3 -> 0 and -4097 -> -2 (rint would give -1, truncation -1)
    v0 = np.array([[1, 2], [0, -2], [9, 12], [10, 15], [2, 0], [2, 1]])
    assert np.array_equal(parts["pmom"][0, 0], profile_words_of(v0).sum(axis=1))
    assert parts["pmom"][0, 0, 1].tolist() == [-2, 4, 0, 0, 0] and not parts["pmom"][0, 1].any()
    v2 = np.array([[0, 0], [0, 0], [11, 10], [13, 11], [0, 1], [1, 2]])
    assert np.array_equal(parts["pmom"][0, 2], profile_words_of(v2).sum(axis=1))
    # bins: (v 32) >> 12 over [0, 2^-8 cm) = [0, 4096) steps of 2^-20 cm; the negative total is outside
    hf, hw = out["hist_flux"], out["hist_wtd"]
    assert hf.dtype == np.int32 and hf.shape == (3, 2, 32) and hw.shape == (3, 2, 16)
    assert np.flatnonzero(hf[0, 0]).tolist() == [0] and hf[0, 0, 0] == 2
    assert hf[0, 1].tolist() == [1] + [0] * 31 and out["outside"] == 1
    assert not hf[1].any() and not hw[1].any()
    assert hw[0, 0].tolist() == [0] * 9 + [1, 0, 0, 1, 0, 0, 0] and hw[0, 1].tolist() == [0] * 10 + [1, 0, 0, 0, 0, 1]
    assert hw[2, 0].tolist() == [0] * 10 + [1, 1, 0, 0, 0, 0] and hw[2, 1].tolist() == [0] * 11 + [1, 0, 1, 0, 0]
    assert period_solved_rows(obs, ends).tolist() == [2, 0, 2]


def test_a_larger_total_lands_in_its_bin_and_overflowing_values_are_counted():
    obs = np.ones(3, dtype=int)
    diag = np.array([[[0.75, 3.0]], [[0.5, float("nan")]]])            # one member, rows 1 and 2
    out = period_totals_of(diag, [[4], [4]], obs, [2], bins=32, flux_max_log2=(1, 2), D=8)
    assert out["acc_at_end"][0, :2, 0].tolist() == [5 << 30, 3 << 32] and out["overflow"] == 1    # the NaN counts, adds 0
    assert np.flatnonzero(out["hist_flux"][0, 0]).tolist() == [20]     # 1.25 cm of [0, 2): bin floor(1.25 / 2 * 32)
    assert np.flatnonzero(out["hist_flux"][0, 1]).tolist() == [24]     # 3 cm of [0, 4)
    big = period_totals_of(np.full((3, 1, 2), 255.0), [[4]] * 3, np.ones(4, dtype=int), [3], bins=32, flux_max_log2=(12, 9), D=8)
    assert big["outside"] == 1 and np.flatnonzero(big["hist_flux"][0, 0]).tolist() == [5] and not big["hist_flux"][0, 1].any()
    stats = period_totals_stats(big["table"], 1, [3], 0, 0.0, 5.0)
    assert stats["transpiration_mean_cm"].tolist() == [765.0] and stats["overflow"] == 0


def test_the_ancestry_moves_the_accumulators_and_rows_after_the_last_end_belong_to_no_period():
    obs, diag, wtd, _ = _tiny()
    plain = period_totals_of(diag, wtd, obs, [4])
    moved = period_totals_of(diag, wtd, obs, [4], ancestors={2: [1, 1]})           # after row 2 both slots hold member 1
    assert plain["acc_at_end"][0, :2].tolist() == [[8201, 8223], [23, -4057]]
    assert moved["acc_at_end"][0, :2].tolist() == [[8193 + 10, 8193 + 30], [-4097 + 20, -4097 + 40]]
    assert moved["acc_at_end"][0, 2:4].tolist() == [[11, 11], [15, 15]]
    assert plain["hist_flux"] is None and plain["acc"][2].tolist() == [PERIOD_WTD_NONE] * 2    # row 5: no period
    # the same rows in two calls, the accumulators handed on: a launch boundary or a restore in the middle of a period
    first = period_totals_of(diag[:1], wtd[:1], obs, [4])
    rest = period_totals_of(diag[1:], wtd[1:], obs, [4], row_begin=2, acc=first["acc"])
    assert np.array_equal(rest["table"], plain["table"])


def test_table_layout_and_the_histogram_split():
    lay = period_totals_table_layout(2, 3, 6)
    assert lay["pmom"] == (0, (2, 3, 6, 5)) and lay["pcnt"] == (180, (2, 3)) and lay["ovf"] == (186, (1,))
    assert lay["words"][0] == 2 * 3 * (5 * 6 + 1) + 1
    with pytest.raises(ValueError, match="the layout has 187"):
        split_period_totals_table(np.zeros(186, dtype=np.int64), 2, 3, 6)
    hf, hw = split_period_hist(np.arange(2 * 3 * 2 * (32 + 10)), 2, 3, 32, 10)
    assert hf.shape == (2, 3, 2, 32) and hw.shape == (2, 3, 2, 10) and hw[0, 0, 0, 0] == 2 * 3 * 2 * 32


# ---- 2. mean and sigma -------------------------------------------------------------------------------------------------
def test_mean_and_sigma_equal_the_exact_fractions():
    rng = np.random.default_rng(3)
    N, ends, thr = 7, [3, 4], [5]
    obs = np.ones(5, dtype=int)
    q = rng.integers(0, 1 << 36, (4, N, 2))
    wtd = rng.integers(2, 9, (4, N))
    out = period_totals_of(q * S, wtd, obs, ends, thr, D=10)
    stats = period_totals_stats(out["table"], 1, ends, 1, z0=2.5, dz=5.0, wtd_obs=obs)

    def exact(values, scale):
        mean = Fraction(sum(values), N)
        var = Fraction(sum(v * v for v in values), N) - mean * mean
        return float(mean * scale), float(var) ** 0.5 * float(scale)

    for p, rows in enumerate((slice(0, 3), slice(3, 4))):
        for k, name in enumerate(("transpiration", "lateral_flow")):
            v = [int(a) >> 12 for a in q[rows, :, k].sum(axis=0)]
            m, s = exact(v, Fraction(1, 1 << 20))
            assert stats[name + "_mean_cm"][p] == m and np.isclose(stats[name + "_std_cm"][p], s, rtol=1e-12)
        m, s = exact([int(v) for v in wtd[rows].min(axis=0)], 1)
        assert stats["wtd_shallowest_mean_cm"][p] == 2.5 + 5.0 * m and np.isclose(stats["wtd_shallowest_std_cm"][p], 5.0 * s)
        m, s = exact([int(v) for v in wtd[rows].max(axis=0)], 1)
        assert stats["wtd_deepest_mean_cm"][p] == 2.5 + 5.0 * m and np.isclose(stats["wtd_deepest_std_cm"][p], 5.0 * s)
        m, s = exact([int(v) for v in (wtd[rows] <= 5).sum(axis=0)], 1)
        assert stats["below_rows_mean"][p, 0] == m and np.isclose(stats["below_rows_std"][p, 0], s)
        assert stats["below_fraction_mean"][p, 0] == m / (3, 1)[p]
    assert stats["count"].tolist() == [N, N] and stats["solved_rows"].tolist() == [3, 1] and stats["end_rows"].tolist() == ends
    empty = period_totals_stats(np.zeros(2 * 25 + 2 + 1, dtype=np.int64), 1, ends, 1, 0.0, 5.0, obs)
    assert all(np.isnan(empty[k]).all() for k in empty if k.endswith(("_cm", "_mean", "_std")))
    two = period_totals_stats(np.concatenate([np.tile(out["table"][:50], 2), np.tile(out["table"][50:52], 2), [0]]), 2, ends, 1,
                              2.5, 5.0, obs)
    assert two["transpiration_mean_cm"].shape == (2, 2) and np.array_equal(two["below_rows_mean"][1], stats["below_rows_mean"])


# ---- 3. the quantile rule ----------------------------------------------------------------------------------------------
def test_quantiles_equal_numpys_inverted_cdf_on_the_bin_index():
    rng = np.random.default_rng(2)
    levels, B, D = [0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0], 64, 40
    for N in (1, 2, 7, 67, 1000):
        fi, wi = rng.integers(0, B, (3, 2, N)), rng.integers(0, D, (3, 2, N))
        hf, hw = np.zeros((3, 2, B), dtype=np.int32), np.zeros((3, 2, D), dtype=np.int32)
        for p in range(3):
            for k in range(2):
                np.add.at(hf[p, k], fi[p, k], 1)
                np.add.at(hw[p, k], wi[p, k], 1)
        d = period_totals_distribution(hf, hw, levels, (4, -3), z0=2.5, dz=5.0)
        qf = np.moveaxis(np.quantile(fi, levels, axis=-1, method="inverted_cdf"), 0, -1)         # [3][2][Lv]
        qw = np.moveaxis(np.quantile(wi, levels, axis=-1, method="inverted_cdf"), 0, -1)
        assert np.array_equal(d["transpiration_quantile_cm"], (qf[:, 0] + 0.5) * 16.0 / B)
        assert np.array_equal(d["lateral_flow_quantile_cm"], (qf[:, 1] + 0.5) * 0.125 / B)
        assert np.array_equal(d["wtd_shallowest_quantile_cm"], 2.5 + 5.0 * qw[:, 0])
        assert np.array_equal(d["wtd_deepest_quantile_cm"], 2.5 + 5.0 * qw[:, 1])
        assert np.all(d["count"] == N)
    empty = period_totals_distribution(np.zeros((2, 2, B), dtype=np.int32), np.zeros((2, 2, D), dtype=np.int32), [0.5], (0, 0), 0, 5)
    assert np.isnan(empty["lateral_flow_quantile_cm"]).all() and np.isnan(empty["wtd_deepest_quantile_cm"]).all()
    lead = period_totals_distribution(np.tile(hf, (2, 1, 1, 1)), np.tile(hw, (2, 1, 1, 1)), [0.5], (0, 0), 0, 5)
    assert lead["transpiration_quantile_cm"].shape == (2, 3, 1)
    with pytest.raises(ValueError, match="at most 16 quantile levels"):
        period_totals_distribution(hf, hw, np.linspace(0, 1, 17), (0, 0), 0, 5)
    with pytest.raises(ValueError, match="each in"):
        period_totals_distribution(hf, hw, [1.5], (0, 0), 0, 5)
    with pytest.raises(ValueError, match="a power of two in 32 .. 1024"):
        period_totals_distribution(hf[..., :48], hw, [0.5], (0, 0), 0, 5)


# ---- 4. the periods ----------------------------------------------------------------------------------------------------
def test_row_periods_and_the_month_and_year_ends_of_the_synthetic_water_year():
    from hydromodel_amd.synthetic import synthetic_forcing
    assert period_ends(100, rows=30).tolist() == [30, 60, 90] and period_ends(91, rows=30).tolist() == [30, 60, 90]
    assert period_ends(90, rows=30).tolist() == [30, 60] and period_ends(10, rows=30).size == 0
    _, datenum, _, _ = synthetic_forcing(1)
    days = [31, 30, 31, 31, 28, 31, 30, 31, 30, 31, 31, 30]                  # October 2008 ... September 2009
    assert datenum.size == 48 * 365
    assert period_ends(datenum.size, datenum=datenum, calendar="month").tolist() == (48 * np.cumsum(days) - 1).tolist()
    assert period_ends(datenum.size, datenum=datenum, calendar="year").tolist() == [48 * 92 - 1]       # 2008 ends; 2009 does not
    short = datenum[:48 * 31]                                                # October alone: its last row closes the month
    assert period_ends(short.size, datenum=short, calendar="month").tolist() == [48 * 31 - 1]
    assert period_ends(short.size - 1, datenum=short[:-1], calendar="month").size == 0
    for bad in (dict(), dict(rows=30, calendar="month", datenum=datenum), dict(rows=0), dict(rows=(1 << 20) + 1),
                dict(calendar="week", datenum=datenum), dict(calendar="month", datenum=datenum[:5]), dict(calendar="month")):
        with pytest.raises(ValueError):
            period_ends(datenum.size, **bad)
    for ends in ([], [0], [3, 3], [5, 4], list(range(1, 4098)), [(1 << 20) + 1]):
        with pytest.raises(ValueError):
            period_totals_of(np.zeros((1, 1, 2)), [[0]], np.ones(2), ends)
    assert [flux_max_log2_of(v) for v in (16, 4, 2.0 ** -8, 4096, 1)] == [4, 2, -8, 12, 0]
    for bad in (3, 0, -4, 8192, 2.0 ** -9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="a power of two in 2\\^-8"):
            flux_max_log2_of(bad)


# ---- 5. the CLI's block ------------------------------------------------------------------------------------------------
def _ens(block, **other):
    return {"Members": 8, "Periods": block, **other}


@pytest.mark.parametrize("ens, want", [
    ({"Members": 8}, None),
    (_ens({"Rows": 1440}), {"rows": 1440, "calendar": None, "thresholds_cm": (), "bins": 0, "flux_max_cm": None, "levels": None}),
    (_ens({"Calendar": "month", "Shallower_than_cm": [100, 200.5]}),
     {"rows": None, "calendar": "month", "thresholds_cm": (100.0, 200.5), "bins": 0, "flux_max_cm": None, "levels": None}),
    (_ens({"Calendar": "year", "Bins": 128}),
     {"rows": None, "calendar": "year", "thresholds_cm": (), "bins": 128, "flux_max_cm": (16.0, 4.0),
      "levels": (0.05, 0.25, 0.5, 0.75, 0.95)}),
    (_ens({"Rows": 1, "Bins": 1024, "Transpiration_max_cm": 0.5, "Lateral_flow_max_cm": 4096, "Quantiles": [0, 1]},
          Filter={"Stride": 48, "Sigma_cm": 8.0, "Sharded": True}, Points=[{}, {}]),      # a sweep ignores Sharded
     {"rows": 1, "calendar": None, "thresholds_cm": (), "bins": 1024, "flux_max_cm": (0.5, 4096.0), "levels": (0.0, 1.0)}),
    (_ens({"Rows": 48}, Filter={"Stride": 48, "Sigma_cm": 8.0, "Sharded": False}),
     {"rows": 48, "calendar": None, "thresholds_cm": (), "bins": 0, "flux_max_cm": None, "levels": None}),
])
def test_settings_accepts(ens, want):
    assert period_settings(ens) == want


@pytest.mark.parametrize("ens, message", [
    (_ens({}), "Periods needs exactly one of Rows"),
    (_ens({"Rows": 48, "Calendar": "month"}), "Periods needs exactly one of Rows"),
    (_ens({"Rows": 0}), "Periods.Rows = 0 must be a whole number of rows in 1 .. 1048576"),
    (_ens({"Rows": 1048577}), "Periods.Rows = 1048577 must be a whole number"),
    (_ens({"Rows": 47.5}), "Periods.Rows = 47.5 must be a whole number"),
    (_ens({"Rows": "48"}), "Periods.Rows = '48' must be a whole number"),
    (_ens({"Rows": True}), "Periods.Rows = True must be a whole number"),
    (_ens({"Calendar": "week"}), "Periods.Calendar = 'week' must be \"month\" or \"year\""),
    (_ens({"Calendar": 12}), "Periods.Calendar = 12 must be"),
    (_ens({"Rows": 48, "Shallower_than_cm": 100}), "Periods.Shallower_than_cm = 100 must be a list of at most 4"),
    (_ens({"Rows": 48, "Shallower_than_cm": [1, 2, 3, 4, 5]}), "must be a list of at most 4 depths"),
    (_ens({"Rows": 48, "Shallower_than_cm": [100, "200"]}), "Periods.Shallower_than_cm: '200' is not a depth in cm"),
    (_ens({"Rows": 48, "Shallower_than_cm": [float("nan")]}), "Periods.Shallower_than_cm: nan is not a depth"),
    (_ens({"Rows": 48, "Shallower_than_cm": [True]}), "Periods.Shallower_than_cm: True is not a depth"),
    (_ens({"Rows": 48, "Bins": 48}), "Periods.Bins = 48 must be a power of two in 32 .. 1024"),
    (_ens({"Rows": 48, "Bins": 2048}), "Periods.Bins = 2048 must be a power of two"),
    (_ens({"Rows": 48, "Bins": 0}), "Periods.Bins = 0 must be a power of two"),
    (_ens({"Rows": 48, "Bins": "128"}), "Periods.Bins = '128' must be a power of two"),
    (_ens({"Rows": 48, "Quantiles": [0.5]}), "Periods.Quantiles needs Periods.Bins"),
    (_ens({"Rows": 48, "Transpiration_max_cm": 16}), "Periods.Transpiration_max_cm needs Periods.Bins"),
    (_ens({"Rows": 48, "Lateral_flow_max_cm": 4}), "Periods.Lateral_flow_max_cm needs Periods.Bins"),
    (_ens({"Rows": 48, "Bins": 64, "Transpiration_max_cm": 10}), "Periods.Transpiration_max_cm = 10 must be a power of two in 2^-8"),
    (_ens({"Rows": 48, "Bins": 64, "Lateral_flow_max_cm": 8192}), "Periods.Lateral_flow_max_cm = 8192 must be a power of two"),
    (_ens({"Rows": 48, "Bins": 64, "Lateral_flow_max_cm": "4"}), "Periods.Lateral_flow_max_cm = '4' must be a power of two"),
    (_ens({"Rows": 48, "Bins": 64, "Quantiles": []}), "Periods.Quantiles = [] must be a non-empty list"),
    (_ens({"Rows": 48, "Bins": 64, "Quantiles": [0.5, 1.5]}), "Periods.Quantiles: 1.5 lies outside [0, 1]"),
    (_ens({"Rows": 48, "Bins": 64, "Quantiles": ["0.5"]}), "Periods.Quantiles: '0.5' is not a number"),
    (_ens({"Rows": 48, "Bins": 64, "Quantiles": [k / 16 for k in range(17)]}), "holds 17 levels; at most 16"),
    (_ens({"Rows": 48, "Stride": 48}), "Periods has unknown keys ['Stride']"),
    (_ens([1440]), "Periods = [1440] must be an object"),
    (_ens({"Rows": 48}, Filter={"Stride": 48, "Sigma_cm": 8.0, "Sharded": True}),
     "Periods with \"Filter\": {\"Sharded\": true}: the columns the ranks exchange do not carry"),
])
def test_settings_rejects(ens, message):
    with pytest.raises(ValueError, match=re.escape(message)):
        period_settings(ens)


def test_the_block_is_checked_against_the_record_and_the_column_before_any_gpu_call():
    from hydromodel_amd.synthetic import synthetic_forcing
    cols = SimpleNamespace(z=5.0 * np.arange(200), dz=5.0)
    datenum = synthetic_forcing(1)[1]
    forcing = SimpleNamespace(dim_t=datenum.size, datenum=datenum)
    assert period_plan(None, cols, forcing, 96) is None
    ends, nodes = period_plan(period_settings(_ens({"Rows": 48, "Shallower_than_cm": [100, 102]})), cols, forcing, 100)
    assert ends.tolist() == [48, 96] and nodes.tolist() == [20, 21]              # the first node at or below the depth
    ends, _ = period_plan(period_settings(_ens({"Calendar": "month"})), cols, forcing, 48 * 62)
    assert ends.tolist() == [48 * 31 - 1, 48 * 61 - 1]
    with pytest.raises(ValueError, match=re.escape("Periods: no period ends within the run's 96 rows")):
        period_plan(period_settings(_ens({"Calendar": "month"})), cols, forcing, 96)
    with pytest.raises(ValueError, match=re.escape("Periods.Shallower_than_cm: sensor depth 1000.0 cm lies outside the column")):
        period_plan(period_settings(_ens({"Rows": 48, "Shallower_than_cm": [1000]})), cols, forcing, 96)
    with pytest.raises(ValueError, match=re.escape("Periods: 17519 periods; at most 4096")):
        period_plan(period_settings(_ens({"Rows": 1})), cols, forcing, datenum.size - 1)


@pytest.mark.parametrize("ens, message", [
    (_ens({"Rows": 48, "Bins": 48}), "Periods.Bins = 48"),
    (_ens({"Rows": 48, "Calendar": "year"}), "exactly one of Rows"),
    (_ens({"Rows": 48}, Filter={"Stride": 48, "Sigma_cm": 8.0, "Sharded": True}), "do not carry"),
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


# ---- 6. the library ----------------------------------------------------------------------------------------------------
def test_the_host_unit_compiles_for_gfx950_without_warnings_and_exports_the_entry_points():
    import __graft_entry__ as ge
    ge.build()
    src = ge.CSRC / "hydrocol.hip"
    text = src.read_text()
    assert all(k in text for k in ("period_accumulate_kernel", "period_reduce_kernel", "period_gather_kernel"))
    p = subprocess.run([ge._hipcc(), *ge.HIPCC_FLAGS, '-DHC_KERNEL_HASH="test"', "-Wall", "-fsyntax-only", str(src)],
                       cwd=str(ge.CSRC), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "period" not in p.stderr and "per_" not in p.stderr and "pacc" not in p.stderr, p.stderr[-3000:]
    from hydromodel_amd import _lib
    lib = _lib.load()
    names = [n for n in _lib.EXPORTS if "period_totals" in n]
    assert len(names) == 14 and all(hasattr(lib, n) for n in names)
