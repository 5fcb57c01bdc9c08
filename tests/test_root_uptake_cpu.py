"""Root-water uptake by depth on the host (include/hydrocol.h hc_set_root_uptake): the layers on the midpoint grid, the
NumPy restatement of the device's u against a plain transcription of the reference's formulas on hand-built theta that
reach every branch, the integer tables against hand-computed integers, and what the host makes of the tables.  No GPU."""
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from helpers import rel_err
from hydromodel_amd.stepper import (PROF_Q_MAX, layer_cells, root_uptake_distribution, root_uptake_layer_totals, root_uptake_of,
                                    root_uptake_profile, root_uptake_stats, root_uptake_table_layout, root_uptake_tables_of,
                                    split_root_uptake_table)

M, DZ = 200, 5.0


def _tables(root_scale=1.0, fc=0.25):
    """[5][M]: porosity falling with depth, field capacity, wilting point, 1 / (por - wlt), an exponential root density
    that integrates to about one over the column (times `root_scale`)."""
    i = np.arange(M)
    por = 0.45 - 0.0005 * i
    wlt = np.full(M, 0.1)
    root = root_scale * np.exp(-(i + 0.5) * DZ / 150.0) / 150.0
    return np.stack([por, np.full(M, fc), wlt, 1.0 / (por - wlt), root])


def _call(th, por, fc, wlt, root, atm, seen):
    """tree_roots' efficiency and richards_pde's uptake of one pde_fun call, as the reference writes them; `seen`
    collects the branches the call takes."""
    water_k = np.sum(th - wlt) * DZ
    if water_k > 0.0:
        local = np.cumsum(th) * DZ
        total = local[-1] if local[-1] != 0.0 else 1.0
        d1 = por - wlt
        d1[d1 == 0.0] = 1.0
        a1 = np.maximum(th / d1, local / total)
        a2 = np.zeros(th.shape)
        mid = (wlt < th) & (th <= fc)
        d2 = fc[mid] - wlt[mid]
        d2[d2 == 0.0] = 1.0
        a2[mid] = (th[mid] - fc[mid]) / d2
        a2[th > fc] = 1.0
        a2 = np.minimum(np.maximum(a2, 0.0), 1.0)
        if np.all(a2 == 1.0):
            a2 *= 0.1
            seen.add("guard")
        seen.add("shut" if np.any(a2 == 0.0) else "open")
        rho = np.abs(a1 * a2)
        tot = np.sum(rho) * DZ
        rho = rho / (tot if tot != 0.0 else 1.0)
    else:
        water_k, rho = 0.0, np.zeros(th.shape)
        seen.add("dry")
    x = rho * root
    tot_x = np.sum(x) * DZ
    if tot_x > 1.0:
        x = x / tot_x
        tot_x = np.sum(x) * DZ
        seen.add("renormalised")
    if tot_x > 0.0:
        seen.add("demand" if atm < water_k else "water")
    return min(atm, water_k) / tot_x * x if tot_x > 0.0 else np.zeros(th.shape)


def _reference(theta, tabs, atm, daylight, n_first, n_int, seen):
    por, fc, wlt, _, root = tabs
    u = np.zeros(theta.shape)
    if not daylight:
        return u
    for k, th in enumerate(theta):
        s = slice(1, 1 + n_int)
        if n_int:
            u[k, s] = _call(th[s], por[s].copy(), fc[s], wlt[s], root[s], atm, seen)
        if n_first:
            u[k, :1] = _call(th[:1], por[:1].copy(), fc[:1], wlt[:1], root[:1], atm, seen)
    return u


def _thetas():
    """{name: theta [M]}: one hand-built profile per branch of the reference."""
    i = np.arange(M)
    rng = np.random.default_rng(5)
    return {"dry": np.full(M, 0.05),                                        # water_k <= 0: zeros
            "drowning": 0.3 + 0.0002 * i,                                   # every cell above field capacity: x 0.1
            "mixed": np.where(i % 3 == 0, 0.2, 0.3) + 0.01 * rng.random(M),   # some cells shut down
            "wet_top": np.where(i < 12, 0.35, 0.12),                        # uptake from the top cells only
            "damp": np.full(M, 0.2),                                        # water, but every cell shut down: zeros
            "at_wilting": np.full(M, 0.1)}                                  # water_k = 0 exactly


# ---- 1. the layers -----------------------------------------------------------------------------------------------------
def test_layer_cells_on_the_midpoint_grid_and_its_refusals():
    z = DZ * np.arange(M + 1)                                               # midpoints 2.5, 7.5, ...
    cells = layer_cells(z, [[0, 100], [100, 300], [300, 1500], [2.5, 7.5], [2.6, 12.5]])
    assert cells.tolist() == [[0, 20], [20, 60], [60, 200], [0, 1], [1, 2]] and cells.dtype == np.int32
    with pytest.raises(ValueError, match="1 to 8 uptake layers, got 9"):
        layer_cells(z, [[0, 100]] * 9)
    with pytest.raises(ValueError, match="1 to 8 uptake layers, got 0"):
        layer_cells(z, [])
    with pytest.raises(ValueError, match="top < bottom"):
        layer_cells(z, [[100, 100]])
    with pytest.raises(ValueError, match="top < bottom"):
        layer_cells(z, [[0, float("nan")]])
    with pytest.raises(ValueError, match="holds no midpoint"):
        layer_cells(z, [[3, 7]])
    with pytest.raises(ValueError, match="holds no midpoint"):
        layer_cells(z, [[1000, 2000]])


# ---- 2. the restatement against the reference's formulas ------------------------------------------------------------
@pytest.mark.parametrize("n_int", [1, 63, 64, 65, 160])
@pytest.mark.parametrize("n_first", [0, 1])
def test_the_restatement_follows_the_reference_on_every_branch(n_int, n_first):
    names, theta = zip(*_thetas().items())
    theta = np.array(theta)
    seen = set()
    for root_scale in (1.0, 1000.0):                                        # the second: tot_x > 1
        tabs = _tables(root_scale)
        for atm in (0.02, 5000.0):                                          # the demand binds, the water binds
            want = _reference(theta, tabs, atm, 1, n_first, n_int, seen)
            got = root_uptake_of(theta, tabs, atm, 1, n_first, n_int, DZ)
            assert got.shape == want.shape and np.all(got >= 0.0)
            assert rel_err(got, want, 1e-3) < 1e-11, (root_scale, atm)
            assert not got[:, n_int + 1:].any() and (n_first or not got[:, 0].any())
            assert not got[names.index("dry")].any() and not got[names.index("at_wilting")].any()
            assert got[names.index("drowning"), 1:n_int + 1].all() and got[names.index("wet_top"), 1].all()
            if n_int == 1:
                # one cell a call: no sum has an order, and alpha_01 is the cumulative fraction, exactly 1
                assert np.array_equal(got, want)
            if n_first:
                assert np.array_equal(got[:, 0], want[:, 0])
            # the interior call's integral is what min(atm, water_k) allows
            k = names.index("drowning")
            water_k = np.sum(theta[k, 1:n_int + 1] - tabs[2, 1:n_int + 1]) * DZ
            assert abs(got[k, 1:n_int + 1].sum() * DZ - min(atm, water_k)) < 1e-12 * min(atm, water_k)
            assert not got[names.index("damp")].any()
    # every branch of the reference was reached by some call
    assert seen == {"dry", "guard", "open", "shut", "renormalised", "demand", "water"}
    tabs = _tables()
    assert not root_uptake_of(theta, tabs, 0.02, 0, n_first, n_int, DZ).any()                      # night
    assert not root_uptake_of(theta, tabs, 0.02, 2, n_first, n_int, DZ).any()                      # (bit 1 is the wet season)
    assert not root_uptake_of(theta, tabs, 0.02, 1, n_first, n_int, DZ, flag_et=False).any()       # ET off
    assert root_uptake_of(theta[1], tabs, 0.02, 3, n_first, n_int, DZ).shape == (1, M)


def test_the_layer_totals_sum_the_cells_in_the_documented_order():
    rng = np.random.default_rng(9)
    u = np.zeros((3, M))
    u[:, :161] = rng.random((3, 161)) * 1e-4
    cells = [(0, 6), (0, M), (M - 1, M), (40, 130), (100, 161)]
    U = root_uptake_layer_totals(u, cells, 160, DZ)
    assert U.shape == (3, 6) and not U[:, 3].any()
    for k, (lo, hi) in enumerate([(0, M)] + cells):
        assert rel_err(U[:, k], DZ * u[:, lo:hi].sum(axis=1), 1e-6) < 1e-12
        x = np.zeros((3, 64))
        for i in range(lo, min(hi, 161)):
            x[:, i % 64] = x[:, i % 64] + u[:, i]
        s = 32
        while s:
            x[:, :s] = x[:, :s] + x[:, s:2 * s]
            s //= 2
        assert np.array_equal(U[:, k], DZ * x[:, 0])


# ---- 3. the integer tables -------------------------------------------------------------------------------------------
def test_the_shift_the_share_bins_and_the_outside_count_equal_the_hand_computed_integers():
    acc = np.array([[-4097, 8192, 0, 4096 * 5], [0, 8192, 0, 4096 * 2]], dtype=np.int64)
    out = root_uptake_tables_of(np.zeros((1, 4, M)), np.zeros(3, dtype=np.int32), [1], [(0, 20)], 160, DZ, bins=32, acc=acc,
                                solved=False)
    parts = split_root_uptake_table(out["table"], 1, 1, 1, M + 1)
    # v = A >> 12 = floor(A / 4096): (-2, 2, 0, 5) and (0, 2, 0, 2)
    assert parts["umom"][0, 0, 0].tolist() == [5, 4 + 4 + 0 + 25, 0, 0, 0]
    assert parts["umom"][0, 0, 1].tolist() == [4, 8, 0, 0, 0]
    assert parts["ucnt"].tolist() == [[4]] and out["outside"] == 2          # v_0 = -2 and v_0 = 0 hold no share
    hist = out["hist"][0, 0]
    assert hist[31] == 1 and hist[12] == 1 and hist.sum() == 2              # v_l = v_0: the last bin; 2 32 // 5 = 12
    assert out["hist"].dtype == np.int32 and not out["acc"].any() and out["overflow"] == 0
    assert np.array_equal(out["acc_at_end"][0], acc)


def test_the_limbs_carry_at_two_to_the_twenty_and_clamped_values_are_counted():
    u = np.zeros((1, 3, M))
    u[0, 0, 1] = 2.0 ** -24                                                  # q = 2^20: limbs (0, 1)
    u[0, 1, 1] = (2.0 ** 20 - 1) * 2.0 ** -44                                # q = 2^20 - 1: limbs (2^20 - 1, 0)
    u[0, 2, 2] = 1.0                                                         # q = 2^44: clamped to 2^40 - 1
    u[0, 1, 3] = -(2.0 ** -30)                                               # a negative q adds nothing, and is counted
    out = root_uptake_tables_of(u, np.zeros(2, dtype=np.int32), [1], [(0, 20)], 160, DZ)
    parts = split_root_uptake_table(out["table"], 1, 1, 1, M + 1)
    assert parts["uprof"][0, 0, 1].tolist() == [2 ** 20 - 1, 1]
    assert parts["uprof"][0, 0, 2].tolist() == [PROF_Q_MAX & (2 ** 20 - 1), PROF_Q_MAX >> 20]
    assert not parts["uprof"][0, 0, 3].any() and out["overflow"] == 2 and parts["ovf"][0] == 2
    lay = root_uptake_table_layout(2, 3, 4, M + 1)
    assert lay["umom"] == (0, (2, 3, 5, 5)) and lay["ucnt"][0] == 150 and lay["uprof"] == (156, (2, 3, M, 2))
    assert lay["words"][0] == 156 + 6 * M * 2 + 1
    with pytest.raises(ValueError, match="the layout has"):
        split_root_uptake_table(np.zeros(5), 2, 3, 4, M + 1)


def test_a_period_whose_only_row_is_skipped_counts_nobody_and_the_ancestry_moves_the_accumulators():
    rng = np.random.default_rng(2)
    u = np.zeros((4, 5, M))
    u[:, :, :161] = rng.random((4, 5, 161)) * 1e-4
    wtd_obs = np.array([60, 60, -1, 60, 60], dtype=np.int32)
    day = np.array([0, 1, 1, 0, 1], dtype=np.uint8)
    anc = np.array([4, 4, 0, 1, 2])
    out = root_uptake_tables_of(u, wtd_obs, [1, 2, 4], [(0, 20)], 160, DZ, bins=32, ancestors={3: anc}, daylight=day)
    parts = split_root_uptake_table(out["table"], 1, 3, 1, M + 1)
    assert parts["ucnt"].tolist() == [[5, 0, 5]]
    assert not parts["umom"][0, 1].any() and not parts["uprof"][0, 1].any() and not out["hist"][1].any()
    # period 2 holds the night row 3 (counted: it is solved) and row 4: the totals are row 4's, per member
    q4 = np.rint(root_uptake_layer_totals(u[3], [(0, 20)], 160, DZ) * 2.0 ** 32).astype(np.int64).T
    assert np.array_equal(out["acc_at_end"][2], q4) and not out["acc"].any()
    # the ancestry after row 3 moved nothing that matters here (row 3 is a night row: zeros); on a day row it does
    day[3] = 1
    moved = root_uptake_tables_of(u, wtd_obs, [1, 2, 4], [(0, 20)], 160, DZ, ancestors={3: anc}, daylight=day)
    q3 = np.rint(root_uptake_layer_totals(u[2], [(0, 20)], 160, DZ) * 2.0 ** 32).astype(np.int64).T
    assert np.array_equal(moved["acc_at_end"][2], q3[:, anc] + q4)
    # rows after the last end belong to no period
    late = root_uptake_tables_of(u, wtd_obs, [1, 2], [(0, 20)], 160, DZ, daylight=day)
    assert not late["acc"].any() and late["solved"] is False


# ---- 4. what the host makes of the tables ----------------------------------------------------------------------------
def _table_of(v, uprof, cnt):
    """A one-point, one-period table from the members' v [K][n] and limbs [M][2]."""
    from hydromodel_amd.stepper import profile_words_of
    umom = profile_words_of(np.asarray(v, dtype=np.int64)).astype(object).sum(axis=1).astype(np.int64)
    return np.concatenate([umom.reshape(-1), [cnt], np.asarray(uprof, dtype=np.int64).reshape(-1), [0]])


def test_mean_and_sigma_equal_the_exact_fractions():
    v = np.array([[3 << 20, 5 << 20, 1 << 19, 7], [1 << 20, 4 << 20, 1 << 18, 0]], dtype=np.int64)
    t = _table_of(v, np.zeros((M, 2)), 4)
    st = root_uptake_stats(t, 1, [48], 1, M + 1)
    for k, (mean, std) in enumerate(((st["total_mean_cm"], st["total_std_cm"]), (st["layer_mean_cm"][:, 0], st["layer_std_cm"][:, 0]))):
        vals = [Fraction(int(x), 1 << 20) for x in v[k]]
        mu = sum(vals) / 4
        var = sum((x - mu) ** 2 for x in vals) / 4
        assert mean[0] == float(mu) and abs(std[0] - float(var) ** 0.5) < 1e-15 * float(var) ** 0.5
    assert st["share_of_mean"][0, 0] == st["layer_mean_cm"][0, 0] / st["total_mean_cm"][0]
    assert st["count"].tolist() == [4] and st["end_rows"].tolist() == [48] and st["overflow"] == 0
    empty = root_uptake_stats(_table_of(np.zeros((2, 0)), np.zeros((M, 2)), 0), 1, [48], 1, M + 1)
    assert np.isnan(empty["total_mean_cm"][0]) and np.isnan(empty["share_of_mean"][0, 0])


def test_share_quantiles_equal_numpys_inverted_cdf_on_the_bin_index():
    rng = np.random.default_rng(3)
    B, levels = 64, [0.0, 0.05, 0.5, 0.95, 1.0]
    idx = rng.integers(0, B, size=(2, 3, 41))                              # [n_period][L][members]
    hist = np.zeros((2, 3, B), dtype=np.int32)
    for p in range(2):
        for l in range(3):
            np.add.at(hist[p, l], idx[p, l], 1)
    hist[1, 2] = 0                                                          # nobody binned
    out = root_uptake_distribution(hist, levels)
    assert out["share_quantile"].shape == (2, 5, 3) and out["count"].tolist() == [41, 41]
    for p in range(2):
        for l in range(3):
            if p == 1 and l == 2:
                assert np.all(np.isnan(out["share_quantile"][p, :, l]))
                continue
            want = (np.quantile(idx[p, l], levels, method="inverted_cdf") + 0.5) / B
            assert np.array_equal(out["share_quantile"][p, :, l], want)
    with pytest.raises(ValueError, match="power of two"):
        root_uptake_distribution(np.zeros((1, 1, 48)), [0.5])
    with pytest.raises(ValueError, match="quantile levels"):
        root_uptake_distribution(np.zeros((1, 1, 64)), [1.5])


def test_the_profile_and_the_depth_quantiles_come_from_the_limbs_exactly():
    z = DZ * np.arange(M + 1)
    uprof = np.zeros((M, 2), dtype=np.int64)
    uprof[0] = [1 << 19, 3]                                                 # cells 0, 1 and 10 take 3.5 : 2.5 : 4 parts
    uprof[1] = [1 << 19, 2]
    uprof[10] = [0, 4]
    t = _table_of(np.zeros((2, 2)), uprof, 2)
    out = root_uptake_profile(t, 1, [48], 1, M + 1, z)
    assert out["depth_cm"][:2].tolist() == [2.5, 7.5] and out["profile"].shape == (1, M)
    assert out["profile"][0, 0] == 3.5 * 2.0 ** 20 / 2 * 2.0 ** -44 and out["profile"][0, 10] == 2.0 * 2.0 ** -24
    assert not out["profile"][0, 11:].any()
    # cumulative 0.35, 0.6, ..., 1.0: half of the uptake lies above the bottom of cell 1, 90 % above the bottom of cell 10
    assert out["depth_quantile_cm"].tolist() == [[10.0, 55.0]]
    none = root_uptake_profile(_table_of(np.zeros((2, 2)), np.zeros((M, 2)), 2), 1, [48], 1, M + 1, z)
    assert np.all(np.isnan(none["depth_quantile_cm"])) and not none["profile"].any()
    nobody = root_uptake_profile(_table_of(np.zeros((2, 0)), np.zeros((M, 2)), 0), 1, [48], 1, M + 1, z)
    assert np.all(np.isnan(nobody["profile"]))


# ---- 5. the CLI block ------------------------------------------------------------------------------------------------
LAYERS = [[0, 100], [100, 300], [300, 1500]]


def _ens(uptake, **more):
    return {"Members": 8, "Periods": {"Rows": 48, "Uptake": uptake}, **more}


def test_the_block_is_read_and_the_periods_own_settings_do_not_see_it():
    from hydromodel_amd.cli import period_settings, uptake_settings
    assert uptake_settings({"Members": 8}) is None and uptake_settings({"Members": 8, "Periods": {"Rows": 48}}) is None
    assert uptake_settings(_ens({"Layers_cm": LAYERS})) == \
        {"layers_cm": ((0.0, 100.0), (100.0, 300.0), (300.0, 1500.0)), "bins": 0, "levels": None}
    got = uptake_settings(_ens({"Layers_cm": [[0, 50.5]], "Bins": 128, "Quantiles": [0.05, 0.5, 0.95]}))
    assert got == {"layers_cm": ((0.0, 50.5),), "bins": 128, "levels": (0.05, 0.5, 0.95)}
    assert uptake_settings(_ens({"Layers_cm": LAYERS, "Bins": 32}))["levels"] == (0.05, 0.5, 0.95)
    assert period_settings(_ens({"Layers_cm": LAYERS})) == period_settings({"Members": 8, "Periods": {"Rows": 48}})


@pytest.mark.parametrize("uptake, message", [
    ([[0, 100]], "Periods.Uptake = [[0, 100]] must be an object"),
    ("on", "Periods.Uptake = 'on' must be an object"),
    ({"Layers_cm": LAYERS, "Stride": 2}, "Periods.Uptake has unknown keys ['Stride']"),
    ({"Bins": 128}, "Periods.Uptake.Layers_cm = None must be a list of 1 to 8"),
    ({"Layers_cm": []}, "must be a list of 1 to 8"),
    ({"Layers_cm": [[0, 10]] * 9}, "must be a list of 1 to 8"),
    ({"Layers_cm": [[100, 100]]}, "[100, 100] is not a [top, bottom] pair in cm with top < bottom"),
    ({"Layers_cm": [[0, "100"]]}, "is not a [top, bottom] pair"),
    ({"Layers_cm": [[0, 100, 200]]}, "is not a [top, bottom] pair"),
    ({"Layers_cm": [[0, True]]}, "is not a [top, bottom] pair"),
    ({"Layers_cm": LAYERS, "Bins": 48}, "Periods.Uptake.Bins = 48 must be a power of two in 32 .. 1024"),
    ({"Layers_cm": LAYERS, "Bins": 0}, "Periods.Uptake.Bins = 0 must be a power of two"),
    ({"Layers_cm": LAYERS, "Quantiles": [0.5]}, "Periods.Uptake.Quantiles needs Periods.Uptake.Bins"),
    ({"Layers_cm": LAYERS, "Bins": 64, "Quantiles": []}, "must be a list of 1 to 16 levels"),
    ({"Layers_cm": LAYERS, "Bins": 64, "Quantiles": [1.5]}, "Periods.Uptake.Quantiles: 1.5 is not a level in [0, 1]"),
])
def test_settings_rejects(uptake, message):
    import re
    from hydromodel_amd.cli import uptake_settings
    with pytest.raises(ValueError, match=re.escape(message)):
        uptake_settings(_ens(uptake))


def test_the_block_is_checked_against_the_column_before_any_gpu_call():
    import re
    from types import SimpleNamespace
    from hydromodel_amd.cli import period_settings, uptake_plan, uptake_settings
    cols = SimpleNamespace(z=DZ * np.arange(M + 1), dz=DZ, flags={"ET": True}, n_root_first=1, n_root_int=59)
    assert uptake_plan(None, [cols]) is None
    up = uptake_settings(_ens({"Layers_cm": [[0, 100], [100, 300]]}))
    assert uptake_plan(up, [cols]).tolist() == [[0, 20], [20, 60]]
    for lay in ([300, 1500], [302.5, 400]):                                 # the root zone ends at cell 59: 300 cm
        with pytest.raises(ValueError, match=re.escape(f"layer {[float(v) for v in lay]!r} cm holds no root cell")):
            uptake_plan(uptake_settings(_ens({"Layers_cm": [[0, 100], lay]})), [cols])
    assert uptake_plan(uptake_settings(_ens({"Layers_cm": [[297, 1500]]})), [cols]).tolist() == [[59, 200]]
    with pytest.raises(ValueError, match="holds no midpoint"):
        uptake_plan(uptake_settings(_ens({"Layers_cm": [[3, 7]]})), [cols])
    shallow = SimpleNamespace(z=cols.z, dz=DZ, flags={"ET": True}, n_root_first=0, n_root_int=10)
    assert uptake_plan(uptake_settings(_ens({"Layers_cm": [[0, 100]]})), [cols, shallow]).tolist() == [[0, 20]]
    with pytest.raises(ValueError, match="holds no root cell"):                 # cell 0 is no root cell of that point
        uptake_plan(uptake_settings(_ens({"Layers_cm": [[0, 5]]})), [cols, shallow])
    with pytest.raises(ValueError, match="holds no root cell"):
        uptake_plan(up, [cols, shallow])
    off = SimpleNamespace(z=cols.z, dz=DZ, flags={"ET": False}, n_root_first=1, n_root_int=59)
    with pytest.raises(ValueError, match="Simulation_Flags.ET is off"):
        uptake_plan(up, [off])
    with pytest.raises(ValueError, match=re.escape("Periods with \"Filter\": {\"Sharded\": true}")):
        period_settings(_ens({"Layers_cm": LAYERS}, Filter={"Stride": 48, "Sigma_cm": 8.0, "Sharded": True}))


@pytest.mark.parametrize("uptake, message", [
    ({"Layers_cm": LAYERS, "Bins": 48}, "Periods.Uptake.Bins = 48"),
    ([1, 2], "must be an object"),
    ({"Layers_cm": LAYERS, "Quantiles": [0.5]}, "needs Periods.Uptake.Bins"),
])
def test_a_bad_block_ends_the_command_with_status_1_before_any_gpu_call(tmp_path, capsys, uptake, message):
    import json
    from hydromodel_amd.cli import run_cli
    from hydromodel_amd.synthetic import default_parameters
    params = default_parameters()
    params["Data_Filename"] = str(tmp_path / "missing.csv")          # never reached: the block is refused first
    params["Ensemble"] = _ens(uptake)
    (tmp_path / "p.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as stop:
        run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "p.json")])
    assert stop.value.code == 1
    out = capsys.readouterr().out
    assert message in out and "missing.csv" not in out


# ---- 6. the library --------------------------------------------------------------------------------------------------
def test_the_host_unit_compiles_for_gfx950_without_warnings_and_exports_the_entry_points():
    import __graft_entry__ as ge
    ge.build()
    src = ge.CSRC / "hydrocol.hip"
    text = src.read_text()
    assert all(k in text for k in ("root_uptake_kernel", "uptake_reduce_kernel"))
    p = subprocess.run([ge._hipcc(), *ge.HIPCC_FLAGS, '-DHC_KERNEL_HASH="test"', "-Wall", "-fsyntax-only", str(src)],
                       cwd=str(ge.CSRC), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "uptake" not in p.stderr and "upt_" not in p.stderr and "uacc" not in p.stderr, p.stderr[-3000:]
    from hydromodel_amd import _lib
    lib = _lib.load()
    names = [n for n in _lib.EXPORTS if "root_uptake" in n]
    assert len(names) == 15 and all(hasattr(lib, n) for n in names)
