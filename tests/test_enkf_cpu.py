"""The ensemble Kalman filter on the host (no GPU): the C-ABI entries, the CLI's "EnKF" validator and its refusals before
any GPU call, the Gaspari-Cohn taper, the record the host forms from the diagnostics table, and the [P] assembly of that
float64 table over two ranks (include/hydrocol.h hc_set_enkf)."""
import json
import os
import re
import socket
from pathlib import Path

import numpy as np
import pytest
import torch.multiprocessing as mp

from hydromodel_amd import multigpu
from hydromodel_amd.cli import enkf_settings, run_cli
from hydromodel_amd.stepper import ENKF_WIDTH, enkf_summary, gaspari_cohn, place_points, stride_rows

REPO = Path(__file__).resolve().parent.parent
NEW_ENTRIES = ("hc_set_enkf", "hc_get_enkf_stats", "hc_set_enkf_stats", "hc_get_enkf_gain", "hc_get_enkf_y",
               "hc_get_enkf_eps")


def test_header_declares_and_the_binding_lists_the_enkf_entries():
    text = (REPO / "include" / "hydrocol.h").read_text()
    from hydromodel_amd import _lib as L
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in L.EXPORTS, name


@pytest.mark.parametrize("block, gpus, want", [
    (None, 1, (0, None, None, None)),
    ({"Sigma_cm": 10.0}, 1, (48, 10.0, 0.0, None)),
    ({"Stride": 24, "Sigma_cm": 2, "Localisation_cm": 50, "Seed": 5}, 1, (24, 2.0, 50.0, 5)),
    ({"Stride": 12.0, "Sigma_cm": 1e100, "Localisation_cm": 0.0}, 1, (12, 1e100, 0.0, None)),
    ({"Stride": 0, "Sigma_cm": 3.0}, 4, (0, None, None, None)),             # off: nothing to refuse
])
def test_enkf_settings_accepts(block, gpus, want):
    ens = {"Members": 8} if block is None else {"Members": 8, "EnKF": block}
    assert enkf_settings(ens, gpus) == want


def test_enkf_settings_lets_a_sweep_run_on_several_ranks():
    ens = {"Members": 8, "Points": [{}, {}], "EnKF": {"Sigma_cm": 5.0}}
    assert enkf_settings(ens, 2) == (48, 5.0, 0.0, None)


@pytest.mark.parametrize("block, gpus, message", [
    ({"Stride": -1, "Sigma_cm": 1.0}, 1, "EnKF.Stride = -1 must be a row stride >= 0"),
    ({"Stride": 2.5, "Sigma_cm": 1.0}, 1, "EnKF.Stride = 2.5 must be a row stride >= 0"),
    ({"Stride": "48", "Sigma_cm": 1.0}, 1, "EnKF.Stride = '48' must be a row stride >= 0"),
    ({"Stride": True, "Sigma_cm": 1.0}, 1, "EnKF.Stride = True must be a row stride >= 0"),
    ({"Stride": 48}, 1, "EnKF.Sigma_cm (the observation error of the well, cm) is required"),
    ({"Sigma_cm": 0.0}, 1, "EnKF.Sigma_cm = 0.0 must be a finite number > 0"),
    ({"Sigma_cm": -2.0}, 1, "EnKF.Sigma_cm = -2.0 must be a finite number > 0"),
    ({"Sigma_cm": float("inf")}, 1, "EnKF.Sigma_cm = inf must be a finite number > 0"),
    ({"Sigma_cm": float("nan")}, 1, "EnKF.Sigma_cm = nan must be a finite number > 0"),
    ({"Sigma_cm": "10"}, 1, "EnKF.Sigma_cm = '10' must be a finite number > 0"),
    ({"Sigma_cm": 1.0, "Localisation_cm": -1.0}, 1, "EnKF.Localisation_cm = -1.0 must be a finite number >= 0"),
    ({"Sigma_cm": 1.0, "Localisation_cm": float("inf")}, 1, "EnKF.Localisation_cm = inf must be a finite number >= 0"),
    ({"Sigma_cm": 1.0, "Localisation_cm": True}, 1, "EnKF.Localisation_cm = True must be a finite number >= 0"),
    ({"Sigma_cm": 1.0, "Seed": -1}, 1, "EnKF.Seed = -1 must be an integer in [0, 2^64)"),
    ({"Sigma_cm": 1.0, "Seed": 1.5}, 1, "EnKF.Seed = 1.5 must be an integer in [0, 2^64)"),
    ({"Sigma_cm": 1.0, "Localization_cm": 2.0}, 1, "EnKF has unknown keys ['Localization_cm']"),
    ({"Sigma_cm": 1.0}, 2, "EnKF with one parameter point runs on one GPU (2 requested)"),
    (48, 1, "EnKF = 48 must be an object"),
])
def test_enkf_settings_rejects(block, gpus, message):
    with pytest.raises(ValueError) as err:
        enkf_settings({"Members": 8, "EnKF": block}, gpus)
    assert message in str(err.value)


def test_enkf_settings_refuses_the_particle_filter_alongside():
    with pytest.raises(ValueError) as err:
        enkf_settings({"Members": 8, "Filter": {"Sigma_cm": 1.0}, "EnKF": {"Sigma_cm": 1.0}}, 1)
    assert '"Filter" and "EnKF" exclude each other' in str(err.value)


@pytest.mark.parametrize("ens, message", [
    ({"EnKF": {"Stride": -2, "Sigma_cm": 1.0}}, "EnKF.Stride = -2 must be a row stride >= 0"),
    ({"EnKF": {"Stride": 48}}, "EnKF.Sigma_cm (the observation error of the well, cm) is required"),
    ({"EnKF": {"Sigma_cm": 1.0, "Localisation_cm": -3}}, "EnKF.Localisation_cm = -3 must be a finite number >= 0"),
    ({"EnKF": {"Sigma_cm": 1.0, "Bogus": 1}}, "EnKF has unknown keys ['Bogus']"),
    ({"EnKF": {"Sigma_cm": 1.0}, "Filter": {"Sigma_cm": 1.0}}, '"Filter" and "EnKF" exclude each other'),
    ({"EnKF": {"Sigma_cm": 1.0}, "GPUs": 2}, "EnKF with one parameter point runs on one GPU (2 requested)"),
])
def test_a_bad_enkf_block_ends_the_command_with_status_1_before_any_gpu_call(tmp_path, capsys, ens, message):
    from hydromodel_amd.synthetic import default_parameters
    params = default_parameters()
    params["Data_Filename"] = str(tmp_path / "missing.csv")          # never reached: the block is refused first
    params["Ensemble"] = {"Members": 8, **ens}
    (tmp_path / "p.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as stop:
        run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "p.json")])
    assert stop.value.code == 1
    out = capsys.readouterr().out
    assert message in out and "missing.csv" not in out


def _gc_reference(r):
    """Gaspari & Cohn (1999) eq. 4.10 as printed (powers, not Horner), r = |z| / c."""
    if r <= 1.0:
        return -0.25 * r ** 5 + 0.5 * r ** 4 + 0.625 * r ** 3 - 5.0 / 3.0 * r ** 2 + 1.0
    if r <= 2.0:
        return r ** 5 / 12.0 - 0.5 * r ** 4 + 0.625 * r ** 3 + 5.0 / 3.0 * r ** 2 - 5.0 * r + 4.0 - 2.0 / (3.0 * r)
    return 0.0


def test_gaspari_cohn_values():
    assert gaspari_cohn(0.0) == 1.0
    for r in (2.0, 2.0 + 1e-12, 3.0, 1e6, np.inf):
        assert gaspari_cohn(r) == 0.0 or abs(gaspari_cohn(r)) < 1e-15, r
    assert abs(gaspari_cohn(2.0)) < 1e-15 and gaspari_cohn(2.5) == 0.0
    e = 1e-9                                                # continuous at r = 1 and r = 2, both pieces agree at 1
    assert abs(gaspari_cohn(1.0 - e) - gaspari_cohn(1.0 + e)) < 1e-8
    assert abs(gaspari_cohn(2.0 - e)) < 1e-8
    assert abs(gaspari_cohn(1.0) - 5.0 / 24.0) < 1e-15
    r = np.linspace(0.0, 2.5, 1001)
    got = gaspari_cohn(r)
    assert got.shape == r.shape and np.all(np.diff(got) <= 1e-15)       # decreasing
    assert np.all((got >= -1e-15) & (got <= 1.0))          # (rounding near r = 2)
    assert np.allclose(got, [_gc_reference(x) for x in r], rtol=0, atol=1e-14)


def test_enkf_summary_sums_the_increments_in_row_order():
    T, stride = 200, 48
    n_arow = stride_rows(T, stride)
    t = np.full((2, n_arow, ENKF_WIDTH), np.nan)
    t[:, :, 0] = 0.0
    for j, inc in ((1, -3.5), (2, -4.25), (4, -1.0)):
        t[:, j] = [16.0, 120.0, 4.0, -2.0, inc, 118.0, 1.5, 0.0]
    t[1, 1:, 4] *= 2.0
    t[0, 4, 7] = 2.0
    s = enkf_summary(t, stride, 10.0, z0_cm=5.0)
    assert s["rows"].tolist() == [48, 96, 192]
    assert s["count"].shape == (2, 3) and s["count"].dtype == np.int64 and np.all(s["count"] == 16)
    assert s["loglik"].tolist() == [(-3.5 + -4.25) + -1.0, (-7.0 + -8.5) + -2.0]
    assert np.all(s["prior_mean_cm"] == 125.0) and np.all(s["post_mean_cm"] == 123.0)
    assert np.all(s["prior_std_cm"] == 4.0) and np.all(s["innovation_cm"] == -2.0) and np.all(s["post_std_cm"] == 1.5)
    assert s["rejected"].tolist() == [[0, 0, 2], [0, 0, 0]] and s["sigma_cm"] == 10.0
    one = enkf_summary(t[0], stride, 10.0)
    assert isinstance(one["loglik"], float) and one["prior_mean_cm"].tolist() == [120.0] * 3
    empty = enkf_summary(t[:, :1], stride, 10.0)
    assert empty["rows"].size == 0 and np.all(empty["loglik"] == 0.0)


def _stats_table(P, n_arow, seed):
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((P, n_arow, ENKF_WIDTH))
    t[..., 0] = rng.integers(1, 100, size=(P, n_arow))
    t[:, 0] = [0.0] + [np.nan] * (ENKF_WIDTH - 1)            # slot 0: nothing analysed
    t[0, 1, 3] = -0.0
    t[-1, -1, 5] = np.frombuffer(np.array([0x7FF8_0000_DEAD_BEEF], dtype=np.uint64).tobytes(), dtype=np.float64)[0]
    return t


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _place_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), HYDROCOL_DIST_BACKEND="gloo")
    ranks = multigpu.Ranks(expect=world)
    whole = _stats_table(5, 6, 7)
    mine = [k for k in range(5) if k % world == rank]             # round-robin, as deal_points
    total = place_points(whole[mine], mine, 5, ranks)
    np.save(os.path.join(out_dir, f"r{rank}.npy"), total)
    ranks.close()


def test_gloo_world2_assembly_of_the_enkf_table_keeps_every_bit(tmp_path):
    mp.spawn(_place_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    whole = _stats_table(5, 6, 7)
    for r in range(2):
        got = np.load(tmp_path / f"r{r}.npy")
        assert got.dtype == np.float64 and got.shape == whole.shape
        assert np.array_equal(got.view(np.int64), whole.view(np.int64))     # NaN payloads and -0.0 included
        assert np.signbit(got[0, 1, 3]) and np.isnan(got[0, 0, 1])
