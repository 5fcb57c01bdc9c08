"""The particle filter on the host (no GPU): the C-ABI entries, the CLI's "Filter" validator and its refusals before any
GPU call, the systematic-resampling slot ranges restated with Python integers, the record the host forms from the
diagnostics table, and the [P] assembly of that float64 table over two ranks (include/hydrocol.h hc_set_filter)."""
import json
import os
import re
import socket
from pathlib import Path

import numpy as np
import pytest
import torch.multiprocessing as mp

from hydromodel_amd import multigpu
from hydromodel_amd.cli import filter_settings, run_cli
from hydromodel_amd.stepper import (FILTER_Q_ONE, filter_ancestors_of, filter_slot_ranges, filter_summary, place_points,
                                    stride_rows)

REPO = Path(__file__).resolve().parent.parent
NEW_ENTRIES = ("hc_set_filter", "hc_get_filter_stats", "hc_set_filter_stats", "hc_get_filter_base", "hc_set_filter_base",
               "hc_get_filter_ancestors", "hc_get_filter_weights", "hc_get_filter_draw")


def test_header_declares_and_the_binding_lists_the_filter_entries():
    text = (REPO / "include" / "hydrocol.h").read_text()
    from hydromodel_amd import _lib as L
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in L.EXPORTS, name


@pytest.mark.parametrize("block, gpus, want", [
    (None, 1, (0, None, None)),
    ({"Sigma_cm": 10.0}, 1, (48, 10.0, None)),
    ({"Stride": 24, "Sigma_cm": 2, "Seed": 5}, 1, (24, 2.0, 5)),
    ({"Stride": 12.0, "Sigma_cm": 1e30}, 1, (12, 1e30, None)),
    ({"Stride": 0, "Sigma_cm": 3.0}, 4, (0, None, None)),            # off: nothing to refuse
])
def test_filter_settings_accepts(block, gpus, want):
    ens = {"Members": 8} if block is None else {"Members": 8, "Filter": block}
    assert filter_settings(ens, gpus) == want


def test_filter_settings_lets_a_sweep_run_on_several_ranks():
    ens = {"Members": 8, "Points": [{}, {}], "Filter": {"Sigma_cm": 5.0}}
    assert filter_settings(ens, 2) == (48, 5.0, None)


@pytest.mark.parametrize("block, gpus, message", [
    ({"Stride": -1, "Sigma_cm": 1.0}, 1, "Filter.Stride = -1 must be a row stride >= 0"),
    ({"Stride": 2.5, "Sigma_cm": 1.0}, 1, "Filter.Stride = 2.5 must be a row stride >= 0"),
    ({"Stride": "48", "Sigma_cm": 1.0}, 1, "Filter.Stride = '48' must be a row stride >= 0"),
    ({"Stride": True, "Sigma_cm": 1.0}, 1, "Filter.Stride = True must be a row stride >= 0"),
    ({"Stride": 48}, 1, "Filter.Sigma_cm (the observation error of the well, cm) is required"),
    ({"Sigma_cm": 0.0}, 1, "Filter.Sigma_cm = 0.0 must be a finite number > 0"),
    ({"Sigma_cm": -2.0}, 1, "Filter.Sigma_cm = -2.0 must be a finite number > 0"),
    ({"Sigma_cm": float("inf")}, 1, "Filter.Sigma_cm = inf must be a finite number > 0"),
    ({"Sigma_cm": float("nan")}, 1, "Filter.Sigma_cm = nan must be a finite number > 0"),
    ({"Sigma_cm": "10"}, 1, "Filter.Sigma_cm = '10' must be a finite number > 0"),
    ({"Sigma_cm": 1.0, "Seed": -1}, 1, "Filter.Seed = -1 must be an integer in [0, 2^64)"),
    ({"Sigma_cm": 1.0, "Seed": 1.5}, 1, "Filter.Seed = 1.5 must be an integer in [0, 2^64)"),
    ({"Sigma_cm": 1.0, "Sigma": 2.0}, 1, "Filter has unknown keys ['Sigma']"),
    ({"Sigma_cm": 1.0}, 2, "Filter with one parameter point runs on one GPU (2 requested)"),
    (48, 1, "Filter = 48 must be an object"),
])
def test_filter_settings_rejects(block, gpus, message):
    with pytest.raises(ValueError) as err:
        filter_settings({"Members": 8, "Filter": block}, gpus)
    assert message in str(err.value)


@pytest.mark.parametrize("block, gpus, message", [
    ({"Stride": -2, "Sigma_cm": 1.0}, 1, "Filter.Stride = -2 must be a row stride >= 0"),
    ({"Stride": 48, "Sigma_cm": 0}, 1, "Filter.Sigma_cm = 0 must be a finite number > 0"),
    ({"Sigma_cm": 1.0, "Bogus": 1}, 1, "Filter has unknown keys ['Bogus']"),
    ({"Sigma_cm": 1.0}, 2, "Filter with one parameter point runs on one GPU (2 requested)"),
])
def test_a_bad_filter_block_ends_the_command_with_status_1_before_any_gpu_call(tmp_path, capsys, block, gpus, message):
    from hydromodel_amd.synthetic import default_parameters
    params = default_parameters()
    params["Data_Filename"] = str(tmp_path / "missing.csv")          # never reached: the block is refused first
    params["Ensemble"] = {"Members": 8, "GPUs": gpus, "Filter": block}
    (tmp_path / "p.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as stop:
        run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "p.json")])
    assert stop.value.code == 1
    out = capsys.readouterr().out
    assert message in out and "missing.csv" not in out


def _ancestor_by_definition(q, r):
    """Slot k takes the member m with C_m <= floor((k Q + r) / N) < C_m + q_m (a search: the statement of the rule)."""
    q = [int(v) for v in q]
    n, Q = len(q), sum(q)
    C = np.cumsum([0] + q[:-1]).tolist()
    out = []
    for k in range(n):
        u = (k * Q + int(r)) // n
        out.append(next(m for m in range(n) if C[m] <= u < C[m] + q[m]))
    return np.array(out, dtype=np.int64)


def _check_partition(q, r):
    ranges = filter_slot_ranges(q, r)
    n = len(q)
    k = 0
    for m, (k0, k1) in enumerate(ranges):
        assert k0 == k and k1 >= k0, (m, k0, k1, k)
        if q[m] == 0:
            assert k1 == k0                                  # a zero weight leaves no offspring
        k = k1
    assert k == n
    anc = filter_ancestors_of(q, r)
    assert np.array_equal(anc, _ancestor_by_definition(q, r))
    assert np.all(np.diff(anc) >= 0)                         # systematic resampling keeps member order
    return anc


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 100, 257])
def test_slot_ranges_partition_the_slots(n):
    rng = np.random.default_rng(n)
    for trial in range(6):
        q = rng.integers(0, FILTER_Q_ONE + 1, size=n)
        if trial % 2:
            q[rng.random(n) < 0.5] = 0                       # truncated bins
        q[rng.integers(0, n)] = FILTER_Q_ONE                 # the nearest occupied bin
        Q = int(q.sum())
        for r in (0, Q - 1, int(rng.integers(0, Q))):
            _check_partition(q.tolist(), r)


def test_slot_ranges_edge_cases():
    n = 77                                                   # not a multiple of 64
    one = [FILTER_Q_ONE] * n                                 # one occupied bin: equal weights
    for r in (0, 1, n * FILTER_Q_ONE - 1):
        assert np.array_equal(_check_partition(one, r), np.arange(n))
    lone = [0] * n
    lone[40] = FILTER_Q_ONE                                  # every other member truncated: all slots take member 40
    assert np.all(_check_partition(lone, 12345) == 40)
    two = [0] * n
    two[3], two[70] = FILTER_Q_ONE, 1                        # a weight of 1 in 2^31 + 1 almost never survives
    anc = _check_partition(two, 0)
    assert np.all(anc == 3)
    anc = _check_partition(two, FILTER_Q_ONE)                # ... unless r sits at the very end of [0, Q)
    assert anc[-1] == 70 and np.all(anc[:-1] == 3)


def test_filter_summary_sums_the_increments_in_row_order():
    T, stride = 200, 48
    n_arow = stride_rows(T, stride)
    t = np.zeros((2, n_arow, 4))
    t[:, :, 1:] = np.nan
    t[:, 0, :] = [0.0, np.nan, np.nan, np.nan]
    for j, inc in ((1, -3.5), (2, -4.25), (4, -1.0)):
        t[:, j] = [16.0, 9.5, inc, 7.0]
    t[1, 1:, 2] *= 2.0
    s = filter_summary(t, stride, 10.0)
    assert s["rows"].tolist() == [48, 96, 192]
    assert s["count"].shape == (2, 3) and s["count"].dtype == np.int64 and np.all(s["count"] == 16)
    assert s["loglik"].tolist() == [(-3.5 + -4.25) + -1.0, (-7.0 + -8.5) + -2.0]
    assert s["survivors"].tolist() == [[7, 7, 7], [7, 7, 7]] and s["sigma_cm"] == 10.0
    one = filter_summary(t[0], stride, 10.0)
    assert isinstance(one["loglik"], float) and one["ess"].shape == (3,)
    empty = filter_summary(t[:, :1], stride, 10.0)
    assert empty["rows"].size == 0 and np.all(empty["loglik"] == 0.0)


def _stats_table(P, n_arow, seed):
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((P, n_arow, 4))
    t[..., 0] = rng.integers(1, 100, size=(P, n_arow))
    t[:, 0] = [0.0, np.nan, np.nan, np.nan]                  # slot 0: nothing assimilated
    t[0, 1, 2] = -0.0
    t[-1, -1, 1] = np.frombuffer(np.array([0x7FF8_0000_DEAD_BEEF], dtype=np.uint64).tobytes(), dtype=np.float64)[0]
    return t


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _place_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), HYDROCOL_DIST_BACKEND="gloo")
    ranks = multigpu.Ranks(expect=world)
    whole = _stats_table(5, 6, 3)
    mine = [k for k in range(5) if k % world == rank]             # round-robin, as deal_points
    total = place_points(whole[mine], mine, 5, ranks)
    np.save(os.path.join(out_dir, f"r{rank}.npy"), total)
    ranks.close()


def test_gloo_world2_assembly_of_the_filter_table_keeps_every_bit(tmp_path):
    mp.spawn(_place_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    whole = _stats_table(5, 6, 3)
    for r in range(2):
        got = np.load(tmp_path / f"r{r}.npy")
        assert got.dtype == np.float64 and got.shape == whole.shape
        assert np.array_equal(got.view(np.int64), whole.view(np.int64))     # NaN payloads and -0.0 included
        assert np.signbit(got[0, 1, 2]) and np.isnan(got[0, 0, 1])
