"""The conductivity statistics without a GPU (include/hydrocol.h hc_set_conductivity_stats): the rule for a row's noise
vector on hand-built cases, the integer restatement of the table against float64 NumPy, the order of the layers' sum, the
run setting from the constructor to a checkpoint's metadata and the CLI's key with every refusal, and the registry's
shapes against the header's formula."""
import ctypes as C

import numpy as np
import pytest

from helpers import digest
from test_run_settings_cpu import recorder, site, start      # noqa: F401  (fixtures: the recording stand-in for the stepper)

LAYERS = [(0.0, 100.0), (100.0, 300.0)]


# ---- 1. the noise rule ------------------------------------------------------------------------------------------------------
def test_base_damping_carries_forward_and_a_refresh_row_damps_its_own_copy():
    from hydromodel_amd.stepper import conductivity_noise_of
    base = np.array([1.0, -2.0, 0.3])
    fresh = np.array([[10.0, 20.0, 0.7], [5.0, 5.0, 5.0]])
    refresh = [False, False, True, False, True, False]
    failed = [0, 2, 1, 0, 0, 1]
    got = conductivity_noise_of(base, fresh, refresh, failed)
    assert np.array_equal(base, [1.0, -2.0, 0.3])            # (the caller's base is left alone)
    b2 = base * 0.8 * 0.8                                   # successive products, as the in-place *= does
    assert np.array_equal(got[0], base)
    assert np.array_equal(got[1], b2)
    assert np.array_equal(got[2], fresh[0] * 0.8) and np.array_equal(fresh[0], [10.0, 20.0, 0.7])
    assert np.array_equal(got[3], b2)                        # the refresh row's failure damped its own copy only
    assert np.array_equal(got[4], fresh[1])
    assert np.array_equal(got[5], b2 * 0.8)


def test_the_philox_base_is_the_draw_times_the_scale_in_one_product():
    from hydromodel_amd.stepper import conductivity_noise_of
    rng = np.random.default_rng(5)
    xi, fresh = rng.standard_normal(101), rng.standard_normal((1, 101))
    refresh, failed = [False, False, True, False], [1, 2, 3, 0]
    got = conductivity_noise_of(xi, fresh, refresh, failed, scale=0.8)
    s1 = np.float64(0.8) * 0.8
    s3 = s1 * 0.8 * 0.8
    assert np.array_equal(got[0], xi * s1) and np.array_equal(got[1], xi * s3) and np.array_equal(got[3], xi * s3)
    assert np.array_equal(got[2], fresh[0] * 0.8 * 0.8 * 0.8)
    # ... which is not the in-memory rule's successive products on the vector: the two sources differ in the last bits
    memory = conductivity_noise_of(xi * 0.8, fresh, refresh, failed)
    assert np.allclose(memory, got, rtol=1e-15, atol=0.0) and not np.array_equal(memory[1], got[1])


# ---- 2. the integer restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 6, 70])
def test_mean_and_sigma_from_the_table_agree_with_numpy(N):
    from hydromodel_amd.stepper import conductivity_layer_of, conductivity_stats, conductivity_tables_of, split_conductivity_table
    D, R = 101, 3
    ranges = [(0, 20), (10, 60), (37, 101)]                  # overlapping; the last ends on the last node
    rng = np.random.default_rng(N)
    ln = rng.normal(-6.0, 3.0, size=(R, 2, N, D))
    ln[0, 0, 0, 5] = -np.inf                                 # K = 0: left out
    ln[1, 1, N - 1, 7] = np.nan                              # left out
    ln[2, 0, 0, 9] = 1500.0                                  # beyond 2^10: clamped, counted in ovf, and still added
    table = conductivity_tables_of(ln, ranges, counted=[True, True, True])
    stats = conductivity_stats(table, 1, R, D, len(ranges), 1)
    parts = split_conductivity_table(table, 1, R, D, len(ranges), 1)
    assert stats["overflow"] == 1 and int(parts["ovf"][0]) == 1
    want_count = np.full((R, D, 2), N)
    want_count[0, 5, 0] -= 1
    want_count[1, 7, 1] -= 1
    assert np.array_equal(stats["count"], want_count)
    masked = np.where(np.isfinite(ln), ln, np.nan)
    masked[2, 0, 0, 9] = (2.0 ** 40 - 1) / 2.0 ** 30         # the clamp
    with np.errstate(invalid="ignore"), np.testing.suppress_warnings() as sup:
        sup.filter(RuntimeWarning)
        for q, name in enumerate(("hrc", "bkg")):
            mean, std = np.nanmean(masked[:, q], axis=1), np.nanstd(masked[:, q], axis=1)
            some = want_count[..., q] > 0
            assert np.array_equal(np.isnan(stats[f"lnK_{name}_mean"]), ~some)
            assert np.max(np.abs(stats[f"lnK_{name}_mean"][some] - mean[some])) < 1e-9
            assert np.max(np.abs(stats[f"lnK_{name}_std"][some] - std[some])) < 1e-9
            assert np.array_equal(stats[f"K_{name}_geomean"][some], np.exp(stats[f"lnK_{name}_mean"][some]))
    # the layers: K_eff = n / sum 1 / K per member, a member with a K = 0 node left out of the layers that hold it
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        k = np.exp(ln[:, 0])
        keff = np.array([conductivity_layer_of(k[j], ranges) for j in range(R)])
        lnk = np.log(np.where((keff > 0) & np.isfinite(keff), keff, np.nan))
    want_l = np.isfinite(lnk).sum(axis=1)
    assert np.array_equal(stats["K_eff_count"], want_l) and want_l[0, 0] == N - 1 and want_l[0, 2] == N
    assert np.array_equal(parts["kcnt_layer"][0], want_l)
    with np.testing.suppress_warnings() as sup:
        sup.filter(RuntimeWarning)
        some = want_l > 0
        assert np.max(np.abs(stats["lnK_eff_mean"][some] - np.nanmean(lnk, axis=1)[some])) < 1e-9
        assert np.max(np.abs(stats["lnK_eff_std"][some] - np.nanstd(lnk, axis=1)[some])) < 1e-9
    # a row that counts nobody
    none = conductivity_tables_of(ln, ranges, counted=[True, False, True])
    p = split_conductivity_table(none, 1, R, D, len(ranges), 1)
    assert not p["kcnt"][0, 1].any() and not p["kmom"][0, 1].any() and not p["kcnt_layer"][0, 1].any()
    assert np.array_equal(p["kmom"][0, 0], parts["kmom"][0, 0]) and np.array_equal(p["kmom"][0, 2], parts["kmom"][0, 2])
    # members are added as integers: two halves of the members sum to the whole
    if N > 1:
        halves = [conductivity_tables_of(ln[:, :, a:b], ranges) for a, b in ((0, N // 2), (N // 2, N))]
        assert np.array_equal(halves[0] + halves[1], table)


def test_the_layer_sum_runs_in_the_layer_storages_order():
    from hydromodel_amd.stepper import conductivity_layer_of, layer_storage_of
    rng = np.random.default_rng(2)
    k = np.exp(rng.normal(-6.0, 4.0, size=(5, 300)))
    k[2, 130] = 0.0
    ranges = [(0, 20), (10, 60), (0, 300), (299, 300), (63, 200)]
    with np.errstate(divide="ignore"):
        got = conductivity_layer_of(k, ranges)
        R, _ = layer_storage_of(1.0 / k, ranges, 1.0)
        want = np.empty_like(got)
        for l, (i0, i1) in enumerate(ranges):                # the documented order, written out
            x = np.zeros((5, 64))
            for i in range(i0, i1):
                x[:, i % 64] = x[:, i % 64] + 1.0 / k[:, i]
            s = 32
            while s:
                x[:, :s] = x[:, :s] + x[:, s:2 * s]
                s //= 2
            want[:, l] = float(i1 - i0) / x[:, 0]
    assert np.array_equal(got, want) and np.array_equal(got, np.diff(np.array(ranges), axis=1).reshape(-1) / R)
    assert np.array_equal(got[:, 3], 1.0 / (1.0 / k[:, 299]))      # a single node: two reciprocals of its K, nothing else
    assert got[2, 2] == 0.0 and got[2, 4] == 0.0 and got[2, 0] > 0.0      # one K = 0 node: the layers that hold it


# ---- 3. the run setting and the CLI's key ----------------------------------------------------------------------------------
def test_the_setting_is_normalised_once_and_refused_before_a_handle(site, recorder):
    from hydromodel_amd import settings
    from hydromodel_amd.ensemble import EnsembleSimulation
    from hydromodel_amd.stepper import MORE_DIAG_TABLES
    cols = site[0]

    def norm(**kw):
        return settings.normalise("EnsembleSimulation", kw, [cols], 6)

    for off in ({}, dict(conductivity=None), dict(conductivity=False)):
        s = norm(profile_stride=48, **off)
        assert s.conductivity is None and not s.on["conductivity"] and s.conductivity_ranges is None
        assert "conductivity" not in settings.tables_on(MORE_DIAG_TABLES, s.on)
        assert "conductivity_layers_cm" not in settings.checkpoint_datasets(s)
    s = norm(profile_stride=48, conductivity=True)
    assert s.on["conductivity"] and s.conductivity == {"layers_cm": None} and s.conductivity_ranges.shape == (0, 2)
    s = norm(profile_stride=48, conductivity={"layers_cm": LAYERS})
    assert s.conductivity_ranges.tolist() == [[0, 20], [20, 60]]
    refused = [(dict(conductivity=True), "conductivity needs the profile statistics"),
               (dict(profile_stride=48, conductivity=3), "conductivity is None, True or"),
               (dict(profile_stride=48, conductivity={"layers": LAYERS}), "unknown keys"),
               (dict(profile_stride=48, conductivity={"layers_cm": [(0, 10)] * 9}), "1 to 8"),
               (dict(profile_stride=48, conductivity={"layers_cm": [(100, 50)]}), "top < bottom"),
               (dict(profile_stride=48, conductivity={"layers_cm": [(501.0, 502.0)]}), "holds no node"),
               (dict(profile_stride=48, conductivity={"layers_cm": [(1.0, 4.0)]}), "holds no node")]
    for kw, message in refused:
        with pytest.raises((ValueError, TypeError), match=message):
            EnsembleSimulation(cols, site[2], 8, seed=6, **kw)
    assert recorder.made == 0
    # a layer of 4096 cm or more, on a column deep enough to hold one
    from hydromodel_amd.stepper import conductivity_ranges
    z = np.arange(0.0, 5000.0, 5.0)
    assert conductivity_ranges(z, 5.0, [(0.0, 4095.0)]).tolist() == [[0, 819]]
    with pytest.raises(ValueError, match="must stay below 4096"):
        conductivity_ranges(z, 5.0, [(0.0, 4100.0)])


def test_the_constructor_sets_the_table_before_the_snapshot_and_the_setting_round_trips(site, recorder, tmp_path):
    from hydromodel_amd import settings
    from hydromodel_amd.ensemble import EnsembleSimulation
    kw = dict(profile_stride=48, conductivity={"layers_cm": LAYERS})
    sim = start("ensemble", site, kw)
    tail = recorder.calls[3:]
    assert tail[0] == "set_profile_stats(int 48)" and tail[1].startswith("set_conductivity_stats(<int32 [2, 2]")
    assert tail[2] == "profile_snapshot(int 0)" and len(tail) == 3
    assert sim.diag_tables_on() == ["profile", "conductivity"]
    recorder.calls = []
    start("ensemble", site, dict(profile_stride=48))         # without the key: the calls a run made before
    assert recorder.calls[3:] == ["set_profile_stats(int 48)", "profile_snapshot(int 0)"]
    # settings -> datasets -> keywords -> settings
    for value, want in ((True, np.zeros((0, 2))), ({"layers_cm": LAYERS}, np.array(LAYERS))):
        first = settings.normalise("EnsembleSimulation", dict(profile_stride=48, conductivity=value), [site[0]], 6)
        data = settings.checkpoint_datasets(first)
        assert data["conductivity_layers_cm"].dtype == np.float64 and np.array_equal(data["conductivity_layers_cm"], want)
        back = settings.checkpoint_keywords(data, "ck")
        assert set(back) == {"profile_stride", "conductivity"}
        second = settings.normalise("EnsembleSimulation", back, [site[0]], 6)
        assert second.on == first.on and np.array_equal(second.conductivity_ranges, first.conductivity_ranges)
    # ... and through a checkpoint file
    sim.stepper.moments = lambda: np.zeros((3, site[2].dim_t), np.int64)
    sim.stepper.diag_raw = lambda key: np.zeros(3, np.int64)
    sim.stepper.diag_counts = lambda: {}
    path = sim.dump(tmp_path / "ck.npz")
    stored = dict(np.load(path))
    assert np.array_equal(stored["conductivity_layers_cm"], np.array(LAYERS)) and "conductivity_table" in stored


CLI_REFUSED = [
    ({"Conductivity": True}, "Conductivity needs the profile rows"),
    ({"Profiles": 48, "Conductivity": 1}, "must be true or an object"),
    ({"Profiles": 48, "Conductivity": "yes"}, "must be true or an object"),
    ({"Profiles": 48, "Conductivity": {"Layers": [[0, 100]]}}, "unknown keys"),
    ({"Profiles": 48, "Conductivity": {"Layers_cm": [[0, 10]] * 9}}, "1 to 8"),
    ({"Profiles": 48, "Conductivity": {"Layers_cm": [[0, "a"]]}}, "not a .top, bottom. pair"),
    ({"Profiles": 48, "Conductivity": {"Layers_cm": [[100, 50]]}}, "top < bottom"),
]


def test_the_clis_key_is_read_and_refused_before_any_gpu_call():
    from hydromodel_amd import cli
    _, cols, _ = digest(1)
    assert cli.conductivity_settings({}) is None and cli.conductivity_settings({"Conductivity": False}) is None
    assert cli.conductivity_settings({"Profiles": 48, "Conductivity": True}) == ()
    assert cli.conductivity_settings({"Profiles": 48, "Conductivity": {}}) == ()
    got = cli.conductivity_settings({"Profiles": 48, "Conductivity": {"Layers_cm": [[0, 100], [100, 300]]}})
    assert got == ((0.0, 100.0), (100.0, 300.0))
    assert cli.conductivity_layer_ranges(got, cols).tolist() == [[0, 20], [20, 60]]
    assert cli.conductivity_layer_ranges(None, cols) is None and cli.conductivity_layer_ranges((), cols).shape == (0, 2)
    for ens, message in CLI_REFUSED:
        with pytest.raises(ValueError, match=message):
            cli.conductivity_settings(ens)
    with pytest.raises(ValueError, match="Conductivity.Layers_cm: .*holds no node"):
        cli.conductivity_layer_ranges(((600.0, 700.0),), cols)
    # false equals absent, all the way to the constructor's keywords; the key reaches them through RunSettings
    assert cli.RunSettings(stride=48).kwargs() == cli.RunSettings(stride=48, conductivity=None).kwargs()
    assert "conductivity" not in cli.RunSettings(stride=48).kwargs()
    assert cli.RunSettings(stride=48, conductivity=()).kwargs()["conductivity"] == {"layers_cm": None}
    assert cli.RunSettings(stride=48, conductivity=got).kwargs()["conductivity"] == {"layers_cm": list(got)}


def test_a_bad_key_ends_the_command_with_status_1_before_the_gpu(tmp_path, capsys, monkeypatch):
    from hydromodel_amd import _lib, cli
    from helpers import cli_params
    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("the library was asked for"))
    params = cli_params(tmp_path)
    params["Ensemble"] = {"Members": 8, "Days": 1, "Profiles": 48, "Conductivity": {"Layers_cm": [[0, 100]], "Bins": 32}}
    with pytest.raises(SystemExit) as stop:
        cli.main(_settings=params)
    assert stop.value.code == 1 and "Conductivity has unknown keys ['Bins']" in capsys.readouterr().out


# ---- 4. the registry's shapes and the header's formula -------------------------------------------------------------------
@pytest.mark.parametrize("P, T, D, L, stride", [(1, 97, 101, 0, 24), (3, 17520, 300, 8, 48), (0, 10, 7, 2, 3)])
def test_the_registrys_shapes_give_the_headers_word_count(P, T, D, L, stride):
    from hydromodel_amd import _lib
    from hydromodel_amd.stepper import (DIAG_TABLES, MORE_DIAG_TABLES, conductivity_table_layout, diag_counts, diag_entry,
                                        diag_keys, diag_layout, diag_placed)
    counts = diag_counts(P, T, D, profile_stride=stride, conductivity_layers=L)
    lay = diag_layout("conductivity", counts)
    n_prow = (T - 1) // stride + 1
    assert lay["words"][0] == P * n_prow * (12 * D + 6 * L) + 1          # include/hydrocol.h
    assert {k: v[1] for k, v in lay.items() if k != "words"} == {
        "kmom": (P, n_prow, D, 2, 5), "kcnt": (P, n_prow, D, 2), "kmom_layer": (P, n_prow, L, 5), "kcnt_layer": (P, n_prow, L),
        "ovf": (1,)}
    assert lay == conductivity_table_layout(P, T, D, L, stride)
    assert diag_placed("conductivity") == ("kmom", "kcnt", "kmom_layer", "kcnt_layer")
    e = diag_entry("conductivity")
    assert "conductivity" in MORE_DIAG_TABLES and diag_keys() == tuple(DIAG_TABLES) + ("conductivity",)
    assert e.dtype == np.int64 and e.outside is None and e.stored == ("conductivity_table", None, False)
    for name in ("hc_get_conductivity_stats", "hc_set_conductivity_stats_tables"):
        assert list(_lib.EXPORTS[name][0]) == [C.c_void_p, C.POINTER(C.c_int64), C.c_int64]
    for name in ("hc_set_conductivity_stats", "hc_clear_conductivity_stats", "hc_get_conductivity_stats_words",
                 "hc_export_conductivity_stats", "hc_reset_conductivity_stats", "hc_get_conductivity_stats_layout",
                 "hc_get_conductivity_stats_overflow", "hc_conductivity_eval"):
        assert name in _lib.EXPORTS
    # a run without the table has no rows of it
    assert diag_layout("conductivity", diag_counts(P, T, D))["words"][0] == 1
