"""Ensemble water-table distributions on the host (no GPU): the C-ABI entries, the CLI's "Distribution" validator, the
slot <-> row mapping, the [P] placement of a rank's points and the sum of the int32 tables over ranks
(include/hydrocol.h hc_set_wtd_hist, hc_wtd_distribution)."""
import json
import os
import re
import socket
from pathlib import Path

import numpy as np
import pytest
import torch.multiprocessing as mp

from hydromodel_amd import multigpu
from hydromodel_amd.cli import distribution_settings, run_cli
from hydromodel_amd.stepper import WTD_MAX_LEVELS, place_points, wtd_hist_rows, wtd_hist_slots

REPO = Path(__file__).resolve().parent.parent
NEW_ENTRIES = ("hc_set_wtd_hist", "hc_get_wtd_hist", "hc_set_wtd_hist_table", "hc_reset_wtd_hist", "hc_wtd_distribution")


def test_header_declares_and_the_library_exports_the_distribution_entries():
    text = (REPO / "include" / "hydrocol.h").read_text()
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert re.search(r"#define\s+HC_WTD_MAX_LEVELS\s+" + str(WTD_MAX_LEVELS) + r"\b", text)
    assert re.search(r"#define\s+HC_WTD_HIST_MAX_ENTRIES\b", text)
    from hydromodel_amd import _lib as L
    if not L.LIB_PATH.exists():
        pytest.skip("libhydrocol.so has not been built")
    lib = L.load()
    for name in NEW_ENTRIES:
        assert name in L.EXPORTS and hasattr(lib, name), name


@pytest.mark.parametrize("block, want", [
    (None, (0, None)),
    ({"Stride": 48, "Quantiles": [0.05, 0.5, 0.95]}, (48, (0.05, 0.5, 0.95))),
    ({}, (48, (0.05, 0.25, 0.5, 0.75, 0.95))),
    ({"Stride": 1, "Quantiles": [0, 1]}, (1, (0.0, 1.0))),
    ({"Stride": 12.0, "Quantiles": [0.5] * 16}, (12, (0.5,) * 16)),
    ({"Stride": 0, "Quantiles": [0.5]}, (0, None)),
])
def test_distribution_settings_accepts(block, want):
    ens = {"Members": 8} if block is None else {"Members": 8, "Distribution": block}
    assert distribution_settings(ens) == want


@pytest.mark.parametrize("block, message", [
    ({"Stride": -1}, "Distribution.Stride = -1 must be a row stride >= 0"),
    ({"Stride": 2.5}, "Distribution.Stride = 2.5 must be a row stride >= 0"),
    ({"Stride": "48"}, "Distribution.Stride = '48' must be a row stride >= 0"),
    ({"Stride": True}, "Distribution.Stride = True must be a row stride >= 0"),
    ({"Quantiles": [0.5, 1.5]}, "Distribution.Quantiles: 1.5 lies outside [0, 1]"),
    ({"Quantiles": [-0.1]}, "Distribution.Quantiles: -0.1 lies outside [0, 1]"),
    ({"Quantiles": [0.5] * 17}, "Distribution.Quantiles holds 17 levels; at most 16 are supported"),
    ({"Quantiles": ["median"]}, "Distribution.Quantiles: 'median' is not a number"),
    ({"Quantiles": [None]}, "Distribution.Quantiles: None is not a number"),
    ({"Quantiles": [float("nan")]}, "Distribution.Quantiles: nan is not a number"),
    ({"Quantiles": 0.5}, "Distribution.Quantiles = 0.5 must be a non-empty list"),
    ({"Quantiles": []}, "Distribution.Quantiles = [] must be a non-empty list"),
    (48, "Distribution = 48 must be an object"),
])
def test_distribution_settings_rejects(block, message):
    with pytest.raises(ValueError) as err:
        distribution_settings({"Members": 8, "Distribution": block})
    assert message in str(err.value)


def test_a_bad_distribution_block_ends_the_command_with_status_1_before_any_gpu_call(tmp_path, capsys):
    from hydromodel_amd.synthetic import default_parameters
    params = default_parameters()
    params["Data_Filename"] = str(tmp_path / "missing.csv")          # never reached: the block is refused first
    params["Ensemble"] = {"Members": 8, "Distribution": {"Stride": -2}}
    (tmp_path / "p.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as stop:
        run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "p.json")])
    assert stop.value.code == 1
    out = capsys.readouterr().out
    assert "Distribution.Stride = -2 must be a row stride >= 0" in out and "missing.csv" not in out


def test_slots_map_to_rows_as_the_profile_rows_do():
    assert wtd_hist_slots(17521, 48) == 366 and wtd_hist_slots(97, 48) == 3 and wtd_hist_slots(96, 48) == 2
    assert wtd_hist_slots(10, 1) == 10 and wtd_hist_slots(1, 5) == 1
    assert wtd_hist_rows(97, 48).tolist() == [0, 48, 96]
    assert wtd_hist_rows(11, 3).tolist() == [0, 3, 6, 9]
    rows = wtd_hist_rows(1000, 7)
    assert np.array_equal(rows // 7, np.arange(rows.size)) and rows[-1] < 1000 <= rows[-1] + 7


def test_place_points_puts_a_ranks_tables_at_its_point_ids():
    local = np.arange(2 * 3 * 4, dtype=np.int32).reshape(2, 3, 4)
    out = place_points(local, [4, 1], 5)
    assert out.shape == (5, 3, 4) and out.dtype == np.int64
    assert np.array_equal(out[4], local[0]) and np.array_equal(out[1], local[1])
    assert not out[[0, 2, 3]].any()
    empty = place_points(np.zeros((0, 3, 4), dtype=np.int32), [], 5)
    assert empty.shape == (5, 3, 4) and not empty.any()


def _table(P, n_hrow, D, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, (1 << 31) - 1, size=(P, n_hrow, D), dtype=np.int64).astype(np.int32)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _sum_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), HYDROCOL_DIST_BACKEND="gloo")
    ranks = multigpu.Ranks(expect=world)
    whole = _table(5, 4, 7, 11)
    mine = [k for k in range(5) if k % world == rank]             # round-robin, as deal_points
    total = ranks.allreduce_sum(place_points(whole[mine], mine, 5))
    np.save(os.path.join(out_dir, f"r{rank}.npy"), total)
    ranks.close()


def test_gloo_world2_sum_of_point_tables_equals_the_single_table_bit_for_bit(tmp_path):
    mp.spawn(_sum_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    whole = _table(5, 4, 7, 11)
    for r in range(2):
        got = np.load(tmp_path / f"r{r}.npy")
        assert got.dtype == np.int64 and np.array_equal(got, whole)
        assert np.array_equal(got.astype(np.int32), whole)
