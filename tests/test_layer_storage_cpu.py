"""Soil-water storage by depth layer, the parts that need no GPU: the node ranges of depth layers (stepper.layer_ranges),
the NumPy restatement of the device's per-member reduction in its documented order (stepper.layer_storage_of), mean and
sigma from the integer table (stepper.layer_storage_stats), the quantile bands (stepper.layer_storage_distribution), the
CLI's "Ensemble": {"Storage": ...} block and the library's build (include/hydrocol.h hc_set_layer_storage)."""
import json
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from hydromodel_amd.cli import run_cli, storage_ranges, storage_settings
from hydromodel_amd.stepper import (PROF_SCALE_STORAGE, layer_ranges, layer_storage_distribution, layer_storage_hist_of,
                                    layer_storage_of, layer_storage_stats, layer_storage_tables_of,
                                    split_layer_storage_table)


# ---- 1. layers -> node ranges ------------------------------------------------------------------------------------------
def test_layer_ranges_by_hand():
    z = 5.0 * np.arange(200)                               # nodes at 0, 5, ..., 995 cm
    # top <= z < bottom: a boundary on a node belongs to the layer below it
    assert layer_ranges(z, [(0, 100), (100, 300)]).tolist() == [[0, 20], [20, 60]]
    assert layer_ranges(z, [(0, 100.0001)]).tolist() == [[0, 21]]
    assert layer_ranges(z, [(2.5, 7.5)]).tolist() == [[1, 2]]                  # a single node
    assert layer_ranges(z, [(995, 996)]).tolist() == [[199, 200]]              # the last one
    assert layer_ranges(z, [(-50, 10000)]).tolist() == [[0, 200]]              # the whole column, and beyond
    assert layer_ranges(z, [(0, 300), (100, 200)]).tolist() == [[0, 60], [20, 40]]     # nested
    assert layer_ranges(z + 12.5, [(0, 100)]).tolist() == [[0, 18]]            # z[0] = 12.5: 12.5 ... 97.5
    r = layer_ranges(z, [(k, k + 5) for k in range(0, 40, 5)])
    assert r.dtype == np.int32 and r.tolist() == [[k, k + 1] for k in range(8)]


@pytest.mark.parametrize("layers, message", [
    ([(1, 4)], "holds no node"),                           # between two nodes
    ([(1000, 1100)], "holds no node"),                     # below the column
    ([(0, 100), (5.5, 9.5)], "holds no node"),
    ([(100, 100)], "top < bottom"),
    ([(300, 100)], "top < bottom"),
    ([(0, float("nan"))], "top < bottom"),
    ([(0, 100, 200)], "top < bottom"),
    ([(k, k + 5) for k in range(0, 45, 5)], "1 to 8 storage layers, got 9"),
    ([], "1 to 8 storage layers, got 0"),
])
def test_layer_ranges_refuses(layers, message):
    with pytest.raises(ValueError, match=re.escape(message)):
        layer_ranges(5.0 * np.arange(200), layers)


# ---- 2. the summation order ------------------------------------------------------------------------------------------
def test_the_documented_order_gives_its_bits_and_a_plain_sum_others():
    """theta built so that the order shows: lane 0 of layer [0, 130) adds nodes 0, 64, 128 in that order, the tree then
    adds lane 32's sum to it."""
    big, one = 2.0 ** 53, 1.0
    theta = np.zeros((2, 200))
    theta[0, 0], theta[0, 64], theta[0, 128] = big, one, one       # lane 0: (2^53 + 1) + 1 = 2^53 (each 1 is lost)
    theta[0, 32], theta[0, 96] = one, one                          # lane 32: 1 + 1 = 2, then 2^53 + 2
    theta[1, 0], theta[1, 64], theta[1, 128] = one, one, big       # lane 0: (1 + 1) + 2^53 = 2^53 + 2
    theta[1, 32], theta[1, 96] = one, one                          # then (2^53 + 2) + 2 = 2^53 + 4
    S, u = layer_storage_of(theta, [(0, 130), (0, 64), (64, 65)], 0.5)
    assert S[:, 0].tolist() == [0.5 * (big + 2.0), 0.5 * (big + 4.0)]
    assert u[:, 0].tolist() == [(big + 2.0) / 130.0, (big + 4.0) / 130.0]
    assert S[:, 1].tolist() == [0.5 * big, 0.5 * 2.0]              # [0, 64): 2^53 + 1 (lanes 0 and 32) rounds to 2^53
    assert S[:, 2].tolist() == [0.5, 0.5] and u[:, 2].tolist() == [1.0, 1.0]
    assert float(Fraction(big) + 4) == big + 4.0                   # (the exact sum of either member, which neither order need give)
    assert np.sum(theta[0, :130]) != big + 2.0                     # a plain sum is another order, and other bits
    # the order is fixed by (i0, i1) alone: the same layer in a deeper column, other members alongside
    deep = np.zeros((3, 300))
    deep[1, :200] = theta[0]
    deep[:, 130:] = 0.25
    assert layer_storage_of(deep, [(0, 130)], 0.5)[0][1, 0] == S[0, 0]


def test_the_restatement_on_random_theta():
    rng = np.random.default_rng(1)
    theta = rng.uniform(0.05, 0.45, (67, 200))
    ranges = [(0, 6), (60, 70), (0, 200), (199, 200), (50, 150)]
    S, u = layer_storage_of(theta, ranges, 5.0)
    assert S.shape == u.shape == (67, 5)
    assert np.array_equal(S[:, 3], 5.0 * theta[:, 199]) and np.array_equal(u[:, 3], theta[:, 199])     # one node: bit for bit
    for l, (i0, i1) in enumerate(ranges):
        assert np.allclose(S[:, l], 5.0 * theta[:, i0:i1].sum(axis=1), rtol=1e-14, atol=0)
    assert np.any(S[:, 2] != 5.0 * theta.sum(axis=1))              # ... but not the bits of a plain sum
    x = np.zeros((67, 64))                                          # [0, 6): one node a lane, lanes 0..5, then the tree
    x[:, :6] = theta[:, :6]
    for s in (32, 16, 8, 4, 2, 1):
        x[:, :s] += x[:, s:2 * s]
    assert np.array_equal(S[:, 0], 5.0 * x[:, 0])
    with pytest.raises(ValueError, match="node ranges"):
        layer_storage_of(theta, [(0, 201)], 5.0)
    with pytest.raises(ValueError, match="node ranges"):
        layer_storage_of(theta, [(5, 5)], 5.0)


def test_binning_of_the_layer_mean():
    B = 32
    u = np.array([[0.0, 1.0], [np.nextafter(5.0 / B, 0.0), 5.0 / B], [np.nan, 1.0 + 2.0 ** -52], [-2.0 ** -1074, 0.5]])
    hist, outside = layer_storage_hist_of(u, B)
    assert hist.shape == (2, B) and outside == 3
    assert hist[0].nonzero()[0].tolist() == [0, 4] and hist[1].nonzero()[0].tolist() == [5, 16, B - 1]
    with pytest.raises(ValueError, match="power of two in 32 .. 1024"):
        layer_storage_hist_of(u, 48)
    assert layer_storage_hist_of(u, 1024)[0].shape == (2, 1024)


# ---- 3. mean and sigma from the table ----------------------------------------------------------------------------------
def test_stats_against_exact_fractions():
    rng = np.random.default_rng(2)
    R, N, D, dz = 3, 41, 130, 5.0
    ranges = [(0, 20), (10, 130)]
    theta = rng.uniform(0.0, 0.5, (R, N, D))
    table, (hist, outside) = layer_storage_tables_of(theta, ranges, dz, bins=64, counted=[True, False, True])
    parts = split_layer_storage_table(table, 1, R, 2, 1)
    assert parts["scnt"].tolist() == [[N, 0, N]] and int(parts["ovf"][0]) == 0 and outside == 0
    assert hist.dtype == np.int32 and hist.sum(axis=-1).tolist() == [[N, N], [0, 0], [N, N]]
    st = layer_storage_stats(table, 1, R, 2, 1)
    assert st["rows"].tolist() == [0, 1, 2] and st["count"].tolist() == [N, 0, N] and st["overflow"] == 0
    assert np.isnan(st["mean_cm"][1]).all() and np.isnan(st["std_cm"][1]).all()
    for j in (0, 2):
        S, _ = layer_storage_of(theta[j], ranges, dz)
        for l in range(2):
            q = [Fraction(int(v)) for v in np.rint(S[:, l] * 2.0 ** PROF_SCALE_STORAGE)]
            mean = sum(q) / N
            var = sum(v * v for v in q) / N - mean * mean
            assert st["mean_cm"][j, l] == float(mean) * 2.0 ** -PROF_SCALE_STORAGE
            assert st["std_cm"][j, l] == float(np.sqrt(np.float64(float(var)))) * 2.0 ** -PROF_SCALE_STORAGE
    # P points: the leading axis stays
    two = np.concatenate([np.tile(parts["stor"], (2, 1, 1, 1)).reshape(-1), np.tile(parts["scnt"], (2, 1)).reshape(-1), [0]])
    st2 = layer_storage_stats(two, 2, R, 2, 1)
    assert st2["mean_cm"].shape == (2, R, 2) and np.array_equal(st2["mean_cm"][1], st["mean_cm"], equal_nan=True)
    with pytest.raises(ValueError, match="words"):
        layer_storage_stats(table[:-1], 1, R, 2, 1)


def test_a_nan_or_an_oversized_value_is_counted_not_summed():
    theta = np.full((1, 4, 70), 0.25)
    theta[0, 1, 3] = np.nan
    table, (hist, outside) = layer_storage_tables_of(theta, [(0, 64), (64, 70)], 5.0, bins=32)
    parts = split_layer_storage_table(table, 1, 1, 2, 1)
    assert int(parts["ovf"][0]) == 1 and outside == 1 and hist[0].sum(axis=-1).tolist() == [3, 4]
    assert parts["stor"][0, 0, 0, 0] == 3 * int(5.0 * 16.0 * 2 ** PROF_SCALE_STORAGE)


# ---- 4. the quantile rule ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [32, 1024])
def test_quantiles_are_numpys_inverted_cdf_on_the_bin_index(B):
    rng = np.random.default_rng(4)
    levels = [0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0]
    ranges, dz = [(0, 20), (20, 60), (0, 200)], 5.0
    for N in (1, 2, 7, 67, 1000):
        idx = rng.integers(0, B, (4, 3, N))                 # [R][L][N] bin indices
        hist = np.zeros((4, 3, B), dtype=np.int32)
        for r in range(4):
            for l in range(3):
                np.add.at(hist[r, l], idx[r, l], 1)
        d = layer_storage_distribution(hist, ranges, dz, levels, stride=48)
        assert d["rows"].tolist() == [0, 48, 96, 144] and np.all(d["count"] == N)
        assert d["quantiles_cm"].shape == (4, len(levels), 3) and d["thickness_cm"].tolist() == [100.0, 200.0, 1000.0]
        want = np.quantile(idx, levels, axis=-1, method="inverted_cdf")            # [Lv][R][L]
        assert np.array_equal(d["quantiles_cm"], np.moveaxis((want + 0.5) / B, 0, 1) * d["thickness_cm"])
    empty = layer_storage_distribution(np.zeros((2, 3, B), dtype=np.int32), ranges, dz, [0.5])
    assert np.isnan(empty["quantiles_cm"]).all() and not empty["count"].any()
    lead = layer_storage_distribution(np.tile(hist, (2, 1, 1, 1)), ranges, dz, [0.5])       # a sweep's [P] axis
    assert lead["quantiles_cm"].shape == (2, 4, 1, 3)


def test_distribution_refuses_bad_tables_and_levels():
    hist = np.zeros((1, 2, 32), dtype=np.int32)
    ranges = [(0, 3), (3, 9)]
    with pytest.raises(ValueError, match="at most 16 quantile levels"):
        layer_storage_distribution(hist, ranges, 5.0, np.linspace(0, 1, 17))
    with pytest.raises(ValueError, match="each in"):
        layer_storage_distribution(hist, ranges, 5.0, [1.5])
    with pytest.raises(ValueError, match="a power of two in 32 .. 1024"):
        layer_storage_distribution(np.zeros((1, 2, 48), dtype=np.int32), ranges, 5.0, [0.5])
    with pytest.raises(ValueError, match="for 1 ranges"):
        layer_storage_distribution(hist, ranges[:1], 5.0, [0.5])


# ---- 5. the CLI's block ------------------------------------------------------------------------------------------------
def _ens(block, **other):
    return {"Members": 8, "Profiles": 48, "Storage": block, **other}


TWO = [[0, 100], [100, 300]]


@pytest.mark.parametrize("ens, want", [
    ({"Members": 8}, None),
    ({"Members": 8, "Profiles": 48}, None),
    (_ens({"Layers_cm": TWO}), (((0.0, 100.0), (100.0, 300.0)), 0, None)),
    (_ens({"Layers_cm": TWO, "Bins": 128}), (((0.0, 100.0), (100.0, 300.0)), 128, (0.05, 0.25, 0.5, 0.75, 0.95))),
    (_ens({"Layers_cm": [[0, 50.5]], "Bins": 1024, "Quantiles": [0, 1]}, Profiles=1), (((0.0, 50.5),), 1024, (0.0, 1.0))),
])
def test_settings_accepts(ens, want):
    assert storage_settings(ens) == want


@pytest.mark.parametrize("ens, message", [
    ({"Members": 8, "Storage": {"Layers_cm": TWO}}, "Storage needs the profile rows: Profiles = 0"),
    (_ens({"Layers_cm": TWO}, Profiles=-3), "Storage needs the profile rows: Profiles = -3"),
    (_ens({"Layers_cm": TWO}, Profiles="48"), "Storage needs the profile rows: Profiles = '48'"),
    (_ens({}), "Storage.Layers_cm = None must be a list of 1 to 8"),
    (_ens({"Layers_cm": []}), "Storage.Layers_cm = [] must be a list of 1 to 8"),
    (_ens({"Layers_cm": [[k, k + 1] for k in range(9)]}), "must be a list of 1 to 8"),
    (_ens({"Layers_cm": [[0, 100], 5]}), "Storage.Layers_cm: 5 is not a [top, bottom] pair"),
    (_ens({"Layers_cm": [[0, 100, 200]]}), "Storage.Layers_cm: [0, 100, 200] is not a [top, bottom] pair"),
    (_ens({"Layers_cm": [[0, "100"]]}), "Storage.Layers_cm: [0, '100'] is not a [top, bottom] pair"),
    (_ens({"Layers_cm": [[0, True]]}), "Storage.Layers_cm: [0, True] is not a [top, bottom] pair"),
    (_ens({"Layers_cm": [[0, float("inf")]]}), "is not a [top, bottom] pair"),
    (_ens({"Layers_cm": [[100, 100]]}), "Storage.Layers_cm: [100, 100] must have top < bottom"),
    (_ens({"Layers_cm": [[300, 100]]}), "Storage.Layers_cm: [300, 100] must have top < bottom"),
    (_ens({"Layers_cm": TWO, "Bins": 48}), "Storage.Bins = 48 must be a power of two in 32 .. 1024"),
    (_ens({"Layers_cm": TWO, "Bins": 2048}), "Storage.Bins = 2048 must be a power of two"),
    (_ens({"Layers_cm": TWO, "Bins": 0}), "Storage.Bins = 0 must be a power of two"),
    (_ens({"Layers_cm": TWO, "Bins": "128"}), "Storage.Bins = '128' must be a power of two"),
    (_ens({"Layers_cm": TWO, "Bins": True}), "Storage.Bins = True must be a power of two"),
    (_ens({"Layers_cm": TWO, "Quantiles": [0.5]}), "Storage.Quantiles needs Storage.Bins"),
    (_ens({"Layers_cm": TWO, "Bins": 64, "Quantiles": []}), "Storage.Quantiles = [] must be a non-empty list"),
    (_ens({"Layers_cm": TWO, "Bins": 64, "Quantiles": 0.5}), "Storage.Quantiles = 0.5 must be a non-empty list"),
    (_ens({"Layers_cm": TWO, "Bins": 64, "Quantiles": [0.5, 1.5]}), "Storage.Quantiles: 1.5 lies outside [0, 1]"),
    (_ens({"Layers_cm": TWO, "Bins": 64, "Quantiles": ["0.5"]}), "Storage.Quantiles: '0.5' is not a number"),
    (_ens({"Layers_cm": TWO, "Bins": 64, "Quantiles": [float("nan")]}), "Storage.Quantiles: nan is not a number"),
    (_ens({"Layers_cm": TWO, "Bins": 64, "Quantiles": [k / 16 for k in range(17)]}), "holds 17 levels; at most 16"),
    (_ens({"Layers_cm": TWO, "Stride": 48}), "Storage has unknown keys ['Stride']"),
    (_ens([[0, 100]]), "Storage = [[0, 100]] must be an object"),
])
def test_settings_rejects(ens, message):
    with pytest.raises(ValueError, match=re.escape(message)):
        storage_settings(ens)


def test_layers_are_checked_against_the_column_before_any_gpu_call():
    from types import SimpleNamespace
    cols = SimpleNamespace(z=5.0 * np.arange(200), dz=5.0)
    assert storage_ranges(None, cols) is None
    assert storage_ranges(storage_settings(_ens({"Layers_cm": TWO})), cols).tolist() == [[0, 20], [20, 60]]
    with pytest.raises(ValueError, match=re.escape("Storage.Layers_cm: storage layer (1000.0, 1100.0) cm holds no node")):
        storage_ranges(storage_settings(_ens({"Layers_cm": [[1000, 1100]]})), cols)
    deep = SimpleNamespace(z=20.0 * np.arange(300), dz=20.0)
    with pytest.raises(ValueError, match=re.escape("[0.0, 5000.0] holds 5000 cm of column; a layer must stay below 4096 cm")):
        storage_ranges(storage_settings(_ens({"Layers_cm": [[0, 5000]]})), deep)


@pytest.mark.parametrize("ens, message", [
    ({"Members": 8, "Storage": {"Layers_cm": TWO}}, "Storage needs the profile rows"),
    (_ens({"Layers_cm": TWO, "Bins": 48}), "Storage.Bins = 48"),
    (_ens({"Layers_cm": [[5, 1]]}), "must have top < bottom"),
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
    assert "layer_storage_kernel" in src.read_text()
    p = subprocess.run([ge._hipcc(), *ge.HIPCC_FLAGS, '-DHC_KERNEL_HASH="test"', "-Wall", "-fsyntax-only", str(src)],
                       cwd=str(ge.CSRC), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "layer_storage" not in p.stderr and "stor_" not in p.stderr, p.stderr[-3000:]
    from hydromodel_amd import _lib
    lib = _lib.load()
    names = [n for n in _lib.EXPORTS if "layer_storage" in n]
    assert len(names) == 11 and all(hasattr(lib, n) for n in names)
