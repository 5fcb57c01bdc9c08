"""Soil-water storage by depth layer reduced on the GPU (include/hydrocol.h hc_set_layer_storage): both tables against the
NumPy restatement (the documented summation order over hc_model_nodes' theta: no tolerance), the single-node layer, their
independence of launch length, member split, slices per block, parameter points and handles, no side effects on the run or on the other
tables, resume, the refusals (but the one for a point of more than 2^31 - 1 members, which no test can allocate) and the
CLI's "Ensemble": {"Storage": ...} block.  Every input keeps theta inside [0, 1], and
every test says so: the overflow and outside counts are 0 wherever the kernel ran."""
import copy
import json
from functools import lru_cache

import numpy as np
import pytest

from helpers import cli_params, digest, digest_point, golden, run_cli_ranks
from test_gpu_enkf import _spread

pytestmark = pytest.mark.gpu

ROWS = 96                                                   # two days
# most lanes empty; across the 64-node stride; the whole column; one node, the last lane sweep partial; two that overlap
LAYERS_200 = [(0, 6), (60, 70), (0, 200), (199, 200), (50, 150), (100, 180)]


def _stepper(well, N, stride, layers, bins, points=None, seed=7, offset=0, bases=None, psi=None, theta_bins=0):
    """A handle on `well` with profile statistics at `stride` and, for layers, the layer storage; row 0 counted."""
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(well)
    st = EnsembleStepper(points or cols, forcing, N)
    st.set_state(_spread(golden(f"g1_tables_{well}.npz")["initial_cond"], N) if psi is None else psi)
    st.set_noise_philox(seed, offset)
    if bases is not None:
        st.set_point_member_bases(np.asarray(bases))
    st.set_profile_stats(stride)
    if theta_bins:
        st.set_theta_hist(theta_bins)
    if layers:
        st.set_layer_storage(layers, bins)
    st.profile_snapshot(0)
    return st, cols, forcing


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _parts(st):
    from hydromodel_amd.stepper import split_layer_storage_table
    return split_layer_storage_table(st.layer_storage_table(), st.P, st.T, len(st.storage_ranges), st.profile_stride)


# ---- 1, 2. exactness -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("well, N, rows, layers, B, stride", [
    (200, 67, 3, LAYERS_200, 32, 1),            # 67 = 16 rounds of 4 waves + 3; every row staged
    (200, 67, 2, LAYERS_200, 1024, 48),         # a launch ends on each profile row (and the table stays small)
    (300, 3, 2, [(0, 300)], 64, 1),             # fewer members than waves
])
def test_every_row_equals_the_restated_reduction_of_the_models_theta(well, N, rows, layers, B, stride):
    from hydromodel_amd.stepper import (PROF_SCALE_STORAGE, layer_storage_of, layer_storage_tables_of,
                                        split_layer_storage_table, stride_rows)
    st, cols, forcing = _stepper(well, N, stride, layers, B)
    L, dz, slots = len(layers), cols.dz, stride_rows(forcing.dim_t, stride)
    try:
        assert all((i1 - i0) * dz < 4096.0 for i0, i1 in layers)
        got_ranges, got_bins = st.layer_storage_layout()
        assert got_ranges.tolist() == [list(r) for r in layers] and got_bins == B
        for r in range(rows + 1):                                       # row 0: the snapshot of the initial state
            if r:
                assert forcing.wtd_obs[r * stride] >= 0
                st.step_rows((r - 1) * stride + 1, stride)
            theta = st.model_nodes()["theta"]
            table, (hist, outside) = layer_storage_tables_of(theta[None], layers, dz, B)
            want = split_layer_storage_table(table, 1, 1, L, 1)
            assert outside == 0 and int(want["ovf"][0]) == 0
            got, got_hist = _parts(st), st.layer_storage_hist_table()
            assert got["stor"].shape == (1, slots, L, 5) and got_hist.shape == (1, slots, L, B)
            assert got_hist.dtype == np.int32
            assert np.array_equal(got["stor"][0, r], want["stor"][0, 0]), r
            assert got["scnt"][0, r] == N and np.array_equal(got_hist[0, r], hist[0]), r
            assert not got["stor"][0, r + 1:].any() and not got["scnt"][0, r + 1:].any() and not got_hist[0, r + 1:].any()
            S, u = layer_storage_of(theta, layers, dz)
            assert np.all(got_hist[0, r].sum(axis=-1) == N)
            for l, (i0, i1) in enumerate(layers):
                if i1 - i0 == 1:                                        # a single-node layer: S = dz theta, bit for bit
                    assert _same(S[:, l], dz * theta[:, i0])
                    assert got["stor"][0, r, l, 0] == int(np.rint(dz * theta[:, i0] * 2.0 ** PROF_SCALE_STORAGE).sum())
        assert L == 1 or len({tuple(h) for h in got_hist[0, rows]}) > 1     # the layers' members sit in different bins
        stats = st.layer_storage_stats()
        # the host's mean and sigma are those of the members' S: a value is quantised to within 2^-29 cm
        assert np.allclose(stats["mean_cm"][rows], S.mean(axis=0), rtol=1e-12, atol=2.0 ** -28)
        assert np.allclose(stats["std_cm"][rows], S.std(axis=0), rtol=1e-6, atol=2.0 ** -27)
        assert st.layer_storage_outside() == 0 and st.layer_storage_overflow() == 0
    finally:
        st.close()


# ---- 3. independence of the run's shape --------------------------------------------------------------------------------
LAYERS_RUN = [(0, 20), (0, 60), (60, 70), (0, 200)]


def _run(N, layers, bins=128, rpl=0, offset=0, points=None, bases=None, psi=None):
    """(moments table, histogram table, profile table) after two days at stride 48 on well 200."""
    st, _, _ = _stepper(200, N, 48, layers, bins, offset=offset, points=points, bases=bases, psi=psi)
    try:
        if rpl:
            st.set_rows_per_launch(rpl)
        st.step_rows(1, ROWS)
        assert st.profile_overflow() == 0
        if not layers:
            return None, None, st.profile_table()
        assert st.layer_storage_outside() == 0 and st.layer_storage_overflow() == 0
        return st.layer_storage_table(), st.layer_storage_hist_table(), st.profile_table()
    finally:
        st.close()


@lru_cache(maxsize=None)
def _spread_67():
    psi = _spread(golden("g1_tables_200.npz")["initial_cond"], 67)
    psi.setflags(write=False)
    return psi


@lru_cache(maxsize=None)
def _whole_67():
    return _run(67, LAYERS_RUN, psi=_spread_67())


def test_the_tables_do_not_depend_on_the_launch_length():
    from hydromodel_amd.stepper import split_layer_storage_table
    table, hist, prof = _whole_67()
    T = digest(200)[2].dim_t
    parts = split_layer_storage_table(table, 1, T, len(LAYERS_RUN), 48)
    assert hist.shape == (1, (T - 1) // 48 + 1, len(LAYERS_RUN), 128)
    assert np.all(parts["scnt"][0, :3] == 67) and not parts["scnt"][0, 3:].any()
    assert np.all(hist[0, :3].sum(axis=-1) == 67) and not hist[0, 3:].any()
    short, hist_short, prof_short = _run(67, LAYERS_RUN, rpl=7, psi=_spread_67())
    assert _same(short, table) and _same(hist_short, hist) and _same(prof_short, prof)
    assert _same(_run(67, None, psi=_spread_67())[2], prof)         # the profile table of a run without the storage


def test_one_handle_equals_two_handles_summed():
    table, hist, prof = _whole_67()
    psi = _spread_67()
    a, hist_a, prof_a = _run(30, LAYERS_RUN, rpl=5, offset=0, psi=psi[:30])
    b, hist_b, prof_b = _run(37, LAYERS_RUN, rpl=11, offset=30, psi=psi[30:])
    assert _same(a + b, table) and _same(hist_a + hist_b, hist) and _same(prof_a + prof_b, prof)


def test_blocks_that_take_several_member_slices_give_the_same_tables(monkeypatch):
    """A point of more than 65 535 slices of 128 members has its blocks take several slices each; the hook lowers that
    bound (read when the handle is made) so that 1000 members do: 8 slices on 3 blocks, the last slice of 104 members."""
    psi = _spread(golden("g1_tables_200.npz")["initial_cond"], 1000)
    want = _run(1000, LAYERS_RUN, psi=psi)
    monkeypatch.setenv("HYDROCOL_DEBUG_STORAGE_GRID_Y", "3")
    got = _run(1000, LAYERS_RUN, psi=psi)
    assert all(_same(g, w) for g, w in zip(got, want))
    from hydromodel_amd.stepper import split_layer_storage_table
    assert np.all(split_layer_storage_table(got[0], 1, digest(200)[2].dim_t, len(LAYERS_RUN), 48)["scnt"][0, :3] == 1000)


def test_two_parameter_points_one_handle_equals_two_handles_summed():
    from hydromodel_amd.stepper import split_layer_storage_table
    _, base, _ = digest(200)
    _, other, _ = digest_point("a003")
    pts = [base, other]
    psi = _spread(golden("g1_tables_200.npz")["initial_cond"], 134)     # point 0: members [0, 67), point 1: [67, 134)

    def members(lo, hi):
        return np.concatenate([psi[lo:hi], psi[67 + lo:67 + hi]])

    whole, hist, prof = _run(134, LAYERS_RUN, 64, points=pts, bases=[0, 5000], psi=psi)
    a, hist_a, prof_a = _run(60, LAYERS_RUN, 64, rpl=5, points=pts, bases=[0, 5000], psi=members(0, 30))
    b, hist_b, prof_b = _run(74, LAYERS_RUN, 64, rpl=11, points=pts, bases=[30, 5030], psi=members(30, 67))
    parts = split_layer_storage_table(whole, 2, digest(200)[2].dim_t, len(LAYERS_RUN), 48)
    assert np.all(parts["scnt"][:, :3] == 67) and np.all(hist[:, :3].sum(axis=-1) == 67)
    assert not _same(parts["stor"][0], parts["stor"][1])            # the points differ
    assert _same(a + b, whole) and _same(hist_a + hist_b, hist) and _same(prof_a + prof_b, prof)


# ---- 4. the run is left alone ----------------------------------------------------------------------------------------
def test_the_storage_leaves_the_run_and_the_other_tables_alone():
    """States, wtd_out, moments, counters, the profile table and the theta histogram with the storage on equal those
    with it off."""
    res = []
    for layers in (None, [(0, 40), (0, 300)]):
        st, _, _ = _stepper(300, 64, 3, layers, 128, seed=3, theta_bins=64)
        try:
            out = st.step_rows(1, ROWS, want_wtd=True)
            res.append((st.get_state(), out["wtd"], st.moments(), st.counters(), st.profile_table(), st.theta_hist_table()))
            if layers:
                assert st.layer_storage_outside() == 0 and st.layer_storage_overflow() == 0
                assert np.all(_parts(st)["scnt"][0, :ROWS // 3 + 1] == 64)
        finally:
            st.close()
    (a_psi, a_w, a_m, a_c, a_p, a_t), (b_psi, b_w, b_m, b_c, b_p, b_t) = res
    assert _same(a_psi, b_psi) and _same(a_w, b_w) and np.array_equal(a_m, b_m) and a_c == b_c and _same(a_p, b_p)
    assert _same(a_t, b_t)


# ---- 5. the tables travel --------------------------------------------------------------------------------------------
def test_set_get_reset_and_the_counts_travel_with_the_tables():
    st, cols, forcing = _stepper(200, 8, 48, [(0, 20), (0, 200)], 32)
    try:
        rng = np.random.default_rng(5)
        t = rng.integers(0, 1000, st.layer_storage_words()).astype(np.int64)
        h = rng.integers(0, 1000, st.layer_storage_hist_table().shape).astype(np.int32)
        st.set_layer_storage_table(t)
        assert _same(st.layer_storage_table(), t) and st.layer_storage_overflow() == int(t[-1])
        for outside in (7, (1 << 40) + 3):                         # both words of the 64-bit count
            st.set_layer_storage_hist_table(h, outside=outside)
            assert st.layer_storage_outside() == outside and _same(st.layer_storage_hist_table(), h)
        st.reset_layer_storage()
        assert not st.layer_storage_table().any() and not st.layer_storage_hist_table().any()
        assert st.layer_storage_outside() == 0
        from hydromodel_amd import _lib as L
        with pytest.raises(L.HcError, match="the table has"):
            L.check(st.lib.hc_set_layer_storage_tables(st.h, L.lptr(t), t.size - 1))
        with pytest.raises(L.HcError, match="the table has"):      # without the count's two entries: another size
            L.check(st.lib.hc_set_layer_storage_hist_table(st.h, L.iptr(h.reshape(-1)), h.size))
    finally:
        st.close()


# ---- 6. resume -------------------------------------------------------------------------------------------------------
def test_resume_from_a_dump_gives_the_uninterrupted_tables(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(300)
    ic = golden("g1_tables_300.npz")["initial_cond"]
    layers_cm = [(0.0, 100.0), (0.0, 300.0)]
    kw = dict(seed=9, psi0=ic, profile_stride=3, storage_layers_cm=layers_cm, storage_bins=64)
    full = EnsembleSimulation(cols, forcing, 64, **kw)
    full.advance(ROWS)
    want, want_hist, want_prof = full.storage_table(), full.storage_hist_table(), full.profile_table()
    assert full.stepper.layer_storage_outside() == 0 and full.stepper.layer_storage_overflow() == 0
    full.close()
    first = EnsembleSimulation(cols, forcing, 64, **kw)
    first.advance(50)
    path = first.dump(tmp_path / "ckpt.h5")
    first.close()
    resumed = EnsembleSimulation.restore(path, cols, forcing)
    resumed.advance(ROWS - 50)
    got, got_hist, got_prof = resumed.storage_table(), resumed.storage_hist_table(), resumed.profile_table()
    stats, bands = resumed.storage_stats(), resumed.storage_distribution([0.05, 0.5, 0.95])
    outside = resumed.stepper.layer_storage_outside()
    resumed.close()
    n = ROWS // 3 + 1
    assert resumed.storage_bins == 64 and outside == 0 and np.array_equal(resumed.storage_layers_cm, layers_cm)
    assert want_hist.shape == ((forcing.dim_t - 1) // 3 + 1, 2, 64) and np.all(want_hist[:n].sum(axis=-1) == 64)
    assert _same(got, want) and _same(got_hist, want_hist) and _same(got_prof, want_prof)
    thick = (stats["nodes"][:, 1] - stats["nodes"][:, 0]) * cols.dz
    assert np.all(stats["count"][:n] == 64) and np.all(stats["mean_cm"][:n] > 0) and np.all(stats["mean_cm"][:n] < thick)
    assert np.isnan(stats["mean_cm"][n:]).all() and np.all(stats["std_cm"][:n] >= 0)
    q = bands["quantiles_cm"]
    assert q.shape == (want_hist.shape[0], 3, 2) and np.all(np.isfinite(q[:n])) and np.isnan(q[n:]).all()
    assert np.all(q[:n, 0] <= q[:n, 2])
    # the mean lies within the band's outer bins (a bin is thick / 64 wide)
    assert np.all(stats["mean_cm"][:n] >= q[:n, 0] - thick / 64 - 3 * stats["std_cm"][:n])
    assert np.all(stats["mean_cm"][:n] <= q[:n, 2] + thick / 64 + 3 * stats["std_cm"][:n])


# ---- 7. refusals -----------------------------------------------------------------------------------------------------
def test_refusals():
    from hydromodel_amd._lib import HcError
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(300)
    st = EnsembleStepper([cols, cols], forcing, 2)
    try:
        st.set_state(golden("g1_tables_300.npz")["initial_cond"])
        st.set_noise_philox(1, 0)

        def off():
            return st.layer_storage_layout()[0].shape == (0, 2) and st.layer_storage_layout()[1] == 0 and \
                len(st.storage_ranges) == 0 and st.storage_bins == 0

        with pytest.raises(HcError, match="needs the profile statistics"):
            st.set_layer_storage([(0, 10)], 32)                    # no profile statistics
        assert off()
        st.set_profile_stats(48)
        with pytest.raises(HcError, match=r"9 layers \(1 to 8"):
            st.set_layer_storage([(k, k + 1) for k in range(9)])
        assert off()
        for bad in ((5, 5), (7, 3), (-1, 4), (0, 301), (300, 301)):
            with pytest.raises(HcError, match="not a range of nodes"):
                st.set_layer_storage([(0, 10), bad], 32)
            assert off()
        for bins in (48, 16, 2048, -32):
            with pytest.raises(HcError, match="a power of two in 32 .. 1024"):
                st.set_layer_storage([(0, 10)], bins)
            assert off()
        st.set_layer_storage([(0, 10), (0, 300)], 1024)
        assert st.layer_storage_hist_table().shape == (2, (forcing.dim_t - 1) // 48 + 1, 2, 1024)
        st.set_layer_storage([(0, 10)], 0)                         # moments alone
        assert st.layer_storage_words() == 2 * ((forcing.dim_t - 1) // 48 + 1) * 6 + 1 and st.layer_storage_outside() == 0
        with pytest.raises(HcError, match="has no histogram"):
            st.layer_storage_hist_table()
        st.set_layer_storage([], 0)
        assert off()
        with pytest.raises(HcError, match="is off"):
            st.layer_storage_overflow()
        st.set_layer_storage([(0, 10)], 64)
        st.set_profile_stats(24)                                   # re-creates what the storage is keyed to: off
        assert off()
        with pytest.raises(HcError, match="is off"):
            st.layer_storage_table()
    finally:
        st.close()
    # a layer of 4096 cm or more cannot be quantised: 300 nodes of 20 cm
    coarse = copy.copy(cols)
    coarse.dz = 20.0
    st = EnsembleStepper(coarse, forcing, 2)
    try:
        st.set_profile_stats(48)
        with pytest.raises(HcError, match="6000 cm thick"):
            st.set_layer_storage([(0, 300)])
        st.set_layer_storage([(0, 204)])                           # 4080 cm
        with pytest.raises(HcError, match="4100 cm thick"):
            st.set_layer_storage([(0, 204), (95, 300)])
        assert st.layer_storage_layout()[0].shape == (0, 2)
    finally:
        st.close()


# ---- 8. the CLI ------------------------------------------------------------------------------------------------------
STORAGE_KEYS = {"storage_layers_cm", "storage_nodes", "storage_rows", "storage_count", "storage_mean_cm", "storage_std_cm",
                "storage_overflow"}
STORAGE_HIST_KEYS = {"storage_hist", "storage_hist_bins", "storage_hist_outside", "storage_quantile_levels",
                     "storage_quantile_cm"}


@pytest.mark.parametrize("n_points", [0, 2])
def test_cli_block_writes_the_datasets_and_leaves_the_rest_alone(tmp_path, monkeypatch, capsys, n_points):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    from hydromodel_amd.stepper import layer_storage_distribution
    params = cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    pts = {"Points": [{"Soil_Properties": {"n": n}} for n in (1.6, 2.4)][:n_points]} if n_points else {}
    levels = [0.05, 0.5, 0.95]
    blocks = (("plain", {}), ("moments", {"Storage": {"Layers_cm": [[0, 100], [100, 300]]}}),
              ("storage", {"Storage": {"Layers_cm": [[0, 100], [100, 300]], "Bins": 64, "Quantiles": levels}}))
    files = {}
    for tag, extra in blocks:
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 128, "Seed": 3, "Days": 2, "Profiles": 48, **pts, **extra}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        capsys.readouterr()
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = (loadResults(tmp_path / f"Run_{tag}_ensemble.h5"), capsys.readouterr().out)
    (plain, log_plain), (mom, log_mom), (stor, log_stor) = files["plain"], files["moments"], files["storage"]
    lead = (n_points,) if n_points else ()
    T = plain["moments"].shape[-1]
    R = (T - 1) // 48 + 1
    assert set(mom) - set(plain) == STORAGE_KEYS and set(stor) - set(plain) == STORAGE_KEYS | STORAGE_HIST_KEYS
    assert stor["storage_layers_cm"].tolist() == [[0, 100], [100, 300]]
    nodes = stor["storage_nodes"]
    assert nodes.shape == (2, 2) and nodes[0, 0] == 0 and nodes[0, 1] == nodes[1, 0] and nodes[1, 1] > nodes[1, 0]
    assert stor["storage_rows"].tolist() == list(range(0, T, 48))
    assert stor["storage_count"].shape == lead + (R,) and np.array_equal(stor["storage_count"], stor["profile_count"])
    assert stor["storage_mean_cm"].shape == lead + (R, 2) and stor["storage_std_cm"].shape == lead + (R, 2)
    assert stor["storage_hist"].shape == lead + (R, 2, 64) and stor["storage_hist"].dtype == np.int32
    assert int(stor["storage_hist_bins"]) == 64 and int(stor["storage_hist_outside"]) == 0 and int(stor["storage_overflow"]) == 0
    assert stor["storage_quantile_levels"].tolist() == levels and stor["storage_quantile_cm"].shape == lead + (R, 3, 2)
    assert np.all(stor["storage_hist"][..., :3, :, :].sum(axis=-1) == 128) and not stor["storage_hist"][..., 3:, :, :].any()
    # the mean storage of a layer is the sum of the per-node theta means times dz (the file already held that much)
    z_step = digest(200)[1].dz
    for l in range(2):
        from_profile = z_step * stor["theta_vol_mean"][..., :3, nodes[l, 0]:nodes[l, 1]].sum(axis=-1)
        assert np.allclose(stor["storage_mean_cm"][..., :3, l], from_profile, rtol=0, atol=1e-6)
    assert np.isnan(stor["storage_mean_cm"][..., 3:, :]).all() and np.all(stor["storage_std_cm"][..., :3, :] >= 0)
    d = layer_storage_distribution(stor["storage_hist"], nodes, z_step, levels, 48)
    assert _same(d["quantiles_cm"], stor["storage_quantile_cm"]) and np.isnan(stor["storage_quantile_cm"][..., 3:, :, :]).all()
    for k in STORAGE_KEYS:                                   # the moments do not depend on the histogram
        assert _same(mom[k], stor[k]), k
    for k in plain:                                          # every other dataset, byte for byte
        assert _same(plain[k], stor[k]) and _same(plain[k], mom[k]), k
    who = f"Sweep 2 points x128" if n_points else "Ensemble x128"
    line = f" [{who}] storage: 2 layers on 3 rows\n"
    assert line in log_stor and line in log_mom and "storage" not in log_plain


@pytest.mark.parametrize("sweep", [False, True])
def test_two_ranks_sharing_the_card_write_what_one_rank_writes(tmp_path, sweep):
    params = cli_params(tmp_path)
    ens = {"Members": 250, "Seed": 5, "Days": 2, "Profiles": 24,
           "Storage": {"Layers_cm": [[0, 100], [0, 300]], "Bins": 32, "Quantiles": [0.1, 0.5, 0.9]}}
    if sweep:                                                # three points dealt to two ranks: 2 + 1
        ens.update(Members=32, Points=[{"Soil_Properties": {"n": n}} for n in (1.6, 2.0, 2.4)])
    params["Ensemble"] = ens
    one, log1 = run_cli_ranks(tmp_path, "one", params, 1)
    two, log2 = run_cli_ranks(tmp_path, "two", params, 2)
    assert STORAGE_KEYS | STORAGE_HIST_KEYS <= set(one) and set(one) == set(two)
    assert int(one["gpus"]) == 1 and int(two["gpus"]) == 2 and int(one["storage_hist_outside"]) == 0
    members = 32 if sweep else 250
    assert np.all(one["storage_count"][..., :5] == members) and np.all(one["storage_hist"][..., :5, :, :].sum(axis=-1) == members)
    for k in one:
        if k != "gpus":
            assert _same(one[k], two[k]), k
    line = [s for s in log1.splitlines() if "storage:" in s]
    assert len(line) == 1 and line == [s for s in log2.splitlines() if "storage:" in s]


@pytest.mark.parametrize("block", [
    {"Filter": {"Stride": 48, "Sigma_cm": 8.0, "Sharded": True}},
    {"EnKF": {"Stride": 24, "Sigma_cm": 8.0, "Sharded": True}},
])
def test_with_a_sharded_filter_or_enkf_two_ranks_write_what_one_rank_writes(tmp_path, block):
    """The storage tables describe the forecast of a filtered run, and every rank's share of the one point is summed."""
    params = cli_params(tmp_path)
    params["Ensemble"] = {"Members": 512, "Seed": 5, "Days": 2, "Profiles": 24, **block,
                          "Storage": {"Layers_cm": [[0, 100], [0, 300]], "Bins": 32, "Quantiles": [0.1, 0.5, 0.9]}}
    one, log1 = run_cli_ranks(tmp_path, "one", params, 1)
    two, log2 = run_cli_ranks(tmp_path, "two", params, 2)
    assert STORAGE_KEYS | STORAGE_HIST_KEYS <= set(one) and set(one) == set(two)
    assert ("filter_sharded" if "Filter" in block else "enkf_sharded") in one
    assert int(one["gpus"]) == 1 and int(two["gpus"]) == 2 and int(one["storage_hist_outside"]) == 0
    assert np.all(one["storage_count"][:5] == 512) and np.all(one["storage_hist"][:5].sum(axis=-1) == 512)
    assert np.array_equal(one["storage_count"], one["profile_count"])
    for k in one:
        if k != "gpus":
            assert _same(one[k], two[k]), k
    assert " [Ensemble x512] storage: 2 layers on 5 rows" in log1.splitlines()
    assert " [Ensemble x512] storage: 2 layers on 5 rows" in log2.splitlines()
