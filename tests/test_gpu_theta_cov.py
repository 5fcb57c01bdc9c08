"""The ensemble covariance of theta(z) and the water table accumulated on the GPU (include/hydrocol.h hc_set_theta_cov):
the table against the NumPy restatement over hc_model_nodes' theta and find_wtd of the state, word for word, at every tile
shape; against the moments table on stepped rows; a member that is not counted; independence of chunk length, launch
length, member split and parameter points; resume; forecast semantics under the particle filter; the layer sigma against
the storage table; the CLI's "Covariance" block; the refusals.

A state cannot hold a NaN (hc_set_state refuses it), so the member that is not counted holds psi = -1e200 at a node: the
specialised cell model's 1 + (alpha psi)^2 overflows and its theta_vol -- hc_model_nodes' too -- is NaN."""
import json
from functools import lru_cache

import numpy as np
import pytest

from assimilation_scale import find_wtd
from helpers import cli_params, digest, digest_point, golden, run_cli_ranks
from test_gpu_enkf import _spread

pytestmark = pytest.mark.gpu

WELL, D = 200, 200


def _handle(N, s, psi=None, points=None, stride=48, offset=0, bases=None, generic=False, seed=7):
    """A handle on the golden column with profile statistics at `stride` and the covariance at node stride `s`; row 0
    counted from the spread initial states."""
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(WELL)
    st = EnsembleStepper(points or cols, forcing, N)
    if generic:
        st.set_generic_exponents(True)
    st.set_state(_spread_states(N) if psi is None else psi)
    st.set_noise_philox(seed, offset)
    if bases is not None:
        st.set_point_member_bases(np.asarray(bases))
    st.set_profile_stats(stride)
    if s:
        st.set_theta_cov(s)
    st.profile_snapshot(0)
    return st, cols, forcing


@lru_cache(maxsize=None)
def _spread_states(N):
    psi = _spread(golden(f"g1_tables_{WELL}.npz")["initial_cond"], N)
    psi.setflags(write=False)
    return psi


def _restated(st, cols, s, members=slice(None)):
    """(words, outside) of the handle's present states: the restatement over hc_model_nodes' theta and find_wtd."""
    from hydromodel_amd.stepper import theta_cov_of
    theta = st.model_nodes()["theta"][members]
    return theta_cov_of(theta, find_wtd(st.get_state()[members], cols.soil.psi_sat), s)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. exact against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N, s", [
    (1000, 1),          # E = 201: four column tiles, the last with 9 columns; 15 chunks of 64 members plus 40
    (1000, 3),          # E = 68: the second tile has 4 columns
    (1000, 7),          # E = 30: one tile
    (1000, D),          # E = 2
    (1, 1), (63, 1), (65, 1),
])
def test_the_snapshot_row_equals_the_restatement_word_for_word(N, s):
    from hydromodel_amd.stepper import stride_rows, theta_cov_shape
    st, cols, forcing = _handle(N, s)
    try:
        n, E, W = theta_cov_shape(D, s)
        assert st.theta_cov_layout() == (s, n, W)
        want, outside = _restated(st, cols, s)
        got = st.theta_cov_table()
        assert got.shape == (1, stride_rows(forcing.dim_t, 48), W) and got.dtype == np.int64
        assert st.theta_cov_words() == got.size + 1
        assert outside == 0 and st.theta_cov_outside() == 0 and int(got[0, 0, 0]) == N
        assert np.array_equal(got[0, 0], want)
        assert not got[0, 1:].any()
        if N > 1:
            assert len(set(find_wtd(st.get_state(), cols.soil.psi_sat).tolist())) > 3       # water tables in many cells
        st.reset_theta_cov()
        assert not st.theta_cov_table().any() and st.theta_cov_outside() == 0
        st.profile_snapshot(48)                                     # any profile row can be a snapshot
        assert np.array_equal(st.theta_cov_table()[0, 1], want)
    finally:
        st.close()


# ---- 2. against the moments table on stepped rows ----------------------------------------------------------------------
@lru_cache(maxsize=None)
def _stepped_67():
    """(covariance table, outside, moments, profile table) of 67 members after two days, profile stride 48, node stride 3."""
    st, cols, forcing = _handle(67, 3)
    try:
        st.step_rows(1, 96)
        return st.theta_cov_table(), st.theta_cov_outside(), np.asarray(st.moments()), st.profile_table()
    finally:
        st.close()


def test_the_water_table_column_equals_the_moments_table_on_stepped_rows():
    from hydromodel_amd.stepper import theta_cov_index, theta_cov_shape
    table, outside, moments, _ = _stepped_67()
    _, _, forcing = digest(WELL)
    n, E, W = theta_cov_shape(D, 3)
    assert outside == 0
    for slot, row in ((1, 48), (2, 96)):
        assert forcing.wtd_obs[row] >= 0
        t = table[0, slot]
        assert int(t[0]) == int(moments[0, row]) == 67
        assert int(t[1 + n]) == int(moments[1, row])
        assert int(t[1 + E + theta_cov_index(n, n, E)]) == int(moments[2, row])
    assert not table[0, 3:].any()


# ---- 3. a member that is not counted -----------------------------------------------------------------------------------
@pytest.mark.parametrize("node, counted", [(6, False), (7, True)])
def test_a_member_with_a_nan_theta_at_a_selected_node_is_not_counted(node, counted):
    """Node stride 3: node 6 is selected, node 7 is not."""
    N, s, bad = 130, 3, 77
    psi = np.array(_spread_states(N))
    psi[bad, node] = -1.0e200
    st, cols, _ = _handle(N, s, psi=psi)
    try:
        theta = st.model_nodes()["theta"]
        assert np.isnan(theta[bad, node]) and np.isfinite(np.delete(theta, bad, axis=0)).all()
        want, outside = _restated(st, cols, s)
        got = st.theta_cov_table()[0, 0]
        assert outside == (0 if counted else 1) and st.theta_cov_outside() == outside
        assert int(got[0]) == N - outside and np.array_equal(got, want)
        if not counted:                                             # ... the table of the others alone
            others = np.delete(np.arange(N), bad)
            assert np.array_equal(got, _restated(st, cols, s, others)[0])
    finally:
        st.close()


# ---- 4. order-freedom --------------------------------------------------------------------------------------------------
def test_a_forced_chunk_length_gives_the_unchunked_table(monkeypatch):
    """The hook is read when the handle is made: 1000 members in chunks of 192 (five full ones and 40)."""
    st, cols, _ = _handle(1000, 3)
    try:
        want = st.theta_cov_table()
        assert np.array_equal(want[0, 0], _restated(st, cols, 3)[0])
    finally:
        st.close()
    monkeypatch.setenv("HYDROCOL_COV_CHUNK_MEMBERS", "192")
    st, _, _ = _handle(1000, 3)
    try:
        assert _same(st.theta_cov_table(), want) and st.theta_cov_outside() == 0
    finally:
        st.close()


def test_one_call_and_two_calls_give_the_same_table():
    table, outside, moments, prof = _stepped_67()
    st, _, _ = _handle(67, 3)
    try:
        st.set_rows_per_launch(7)
        st.step_rows(1, 40)
        st.step_rows(41, 56)
        assert _same(st.theta_cov_table(), table) and st.theta_cov_outside() == outside
        assert _same(st.profile_table(), prof)
    finally:
        st.close()
    assert np.all(table[0, :3, 0] == 67)


def test_two_handles_sum_to_the_one_handles_table():
    N, s, bad = 1000, 7, 700
    psi = np.array(_spread_states(N))
    psi[bad, 14] = -1.0e200                                        # a selected node of the second handle's members
    got = []
    for lo, hi in ((0, N), (0, 512), (512, N)):
        st, _, _ = _handle(hi - lo, s, psi=psi[lo:hi], offset=lo)
        try:
            got.append((st.theta_cov_table(), st.theta_cov_outside()))
        finally:
            st.close()
    (whole, out), (a, out_a), (b, out_b) = got
    assert _same(a + b, whole) and (out, out_a, out_b) == (1, 0, 1) and int(whole[0, 0, 0]) == N - 1


def test_a_sweep_of_two_points_equals_the_two_single_point_tables():
    _, base, _ = digest(WELL)
    _, other, _ = digest_point("a003")
    psi = _spread_states(600)                                       # point 0: members [0, 300), point 1: [300, 600)
    both, cols, _ = _handle(600, 3, psi=psi, points=[base, other], bases=[0, 5000], generic=True)
    try:
        table = both.theta_cov_table()
        theta, state = both.model_nodes()["theta"], both.get_state()
    finally:
        both.close()
    from hydromodel_amd.stepper import theta_cov_of
    assert table.shape[0] == 2 and not _same(table[0], table[1])
    for k, pt in enumerate((base, other)):
        one, _, _ = _handle(300, 3, psi=psi[300 * k:300 * (k + 1)], points=[pt], offset=5000 * k, generic=True)
        try:
            assert _same(one.theta_cov_table()[0], table[k]), k
        finally:
            one.close()
        want, outside = theta_cov_of(theta[300 * k:300 * (k + 1)], find_wtd(state[300 * k:300 * (k + 1)], pt.soil.psi_sat), 3)
        assert outside == 0 and np.array_equal(table[k, 0], want), k


# ---- 5. checkpoint -----------------------------------------------------------------------------------------------------
def test_resume_from_a_dump_gives_the_uninterrupted_table(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(WELL)
    kw = dict(seed=9, psi0=_spread_states(64), profile_stride=24, theta_cov_stride=3)
    full = EnsembleSimulation(cols, forcing, 64, **kw)
    try:
        full.advance(96)
        want, want_prof = full.theta_cov_table(), full.profile_table()
        assert full.stepper.theta_cov_outside() == 0
    finally:
        full.close()
    first = EnsembleSimulation(cols, forcing, 64, **kw)
    try:
        first.advance(48)
        path = first.dump(tmp_path / "ckpt.h5")
    finally:
        first.close()
    resumed = EnsembleSimulation.restore(path, cols, forcing)
    try:
        assert resumed.theta_cov_stride == 3
        resumed.advance(48)
        got, got_prof, outside = resumed.theta_cov_table(), resumed.profile_table(), resumed.stepper.theta_cov_outside()
        fin = resumed.theta_covariance(sensor_sigma=0.02)
    finally:
        resumed.close()
    assert _same(got, want) and _same(got_prof, want_prof) and outside == 0
    assert np.all(want[:5, 0] == 64) and not want[5:].any()
    assert fin["theta_cov"].shape == (want.shape[0], 67, 67) and fin["rows"][:5].tolist() == [0, 24, 48, 72, 96]
    assert np.isfinite(fin["theta_cov"][:5]).all() and np.isnan(fin["theta_cov"][5:]).all()
    assert fin["nodes"].tolist() == list(range(0, D, 3)) and fin["theta_sensor_gain"].shape == (want.shape[0], 67)
    # the spread states' water tables differ: the gain of a probe is defined, and a fraction below one
    gain = fin["theta_sensor_gain"][:5]
    assert np.all(fin["wtd_var_cm2"][:5] > 0) and np.all((gain >= 0.0) & (gain < 1.0)) and gain.max() > 0.1
    assert np.all(np.abs(fin["theta_wtd_corr"][:5][np.isfinite(fin["theta_wtd_corr"][:5])]) <= 1.0 + 1e-12)


# ---- 6. forecast semantics ---------------------------------------------------------------------------------------------
def test_with_a_particle_filter_the_table_describes_the_forecast():
    """The tables are filled before the resampling: row 48 of a filtered run is row 48 of the same run without the filter."""
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(WELL)
    assert forcing.wtd_obs[48] >= 0
    tables = []
    for fkw in ({}, dict(filter_stride=48, filter_sigma_cm=2.0 * cols.dz)):
        sim = EnsembleSimulation(cols, forcing, 96, seed=6, psi0=_spread_states(96), profile_stride=48, theta_cov_stride=4,
                                 **fkw)
        try:
            sim.advance(60)
            tables.append(sim.theta_cov_table())
            if fkw:
                assert sim.filter_summary()["survivors"][0] < 96   # it did resample
        finally:
            sim.close()
    plain, filtered = tables
    assert int(plain[1, 0]) == 96 and _same(filtered[:2], plain[:2])


# ---- 7. against the storage table --------------------------------------------------------------------------------------
def test_the_layer_sigma_agrees_with_the_storage_table_and_not_with_the_summed_variances(capsys):
    """layer_std_cm forms a layer's sigma from the covariance of theta quantised to 2^-20, the storage table from the
    members' own sums: a member's sum moves by at most n_layer dz 2^-21 cm, the storage's quantisation by 2^-29, and a
    sigma by no more than its values do.  The root of the summed per-node variances ignores that the nodes covary."""
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(WELL)
    layers = [(0.0, 100.0), (100.0, 300.0)]
    sim = EnsembleSimulation(cols, forcing, 64, seed=9, psi0=_spread_states(64), profile_stride=48, theta_cov_stride=1,
                             storage_layers_cm=layers)
    try:
        sim.advance(96)
        got, stats, cov = sim.layer_std_cm(layers), sim.storage_stats(), sim.theta_covariance()
        with pytest.raises(ValueError, match="theta_cov_stride = 1"):
            sim.theta_cov_stride = 2
            sim.layer_std_cm(layers)
    finally:
        sim.close()
    dz, z0 = cols.dz, float(cols.z[0])
    seen = 0
    for l, (i0, i1) in enumerate(stats["nodes"]):
        bound = (i1 - i0) * dz * 2.0 ** -21 + 2.0 ** -28
        worst = float(np.abs(got[:3, l] - stats["std_cm"][:3, l]).max())
        with capsys.disabled():
            print(f"\n layer {l} [{i0}, {i1}): |layer_std_cm - storage_std_cm| <= {worst:.3e} cm (bound {bound:.3e})")
        assert worst <= bound
        naive = dz * np.sqrt(np.einsum("rii->ri", cov["theta_cov"][:3])[:, i0:i1].sum(axis=1))
        wtd_cm = z0 + dz * cov["wtd_mean_idx"][:3]
        inside = (wtd_cm >= z0 + i0 * dz) & (wtd_cm < z0 + i1 * dz)
        with capsys.disabled():
            print(f" layer {l}: sigma / sqrt(sum sigma^2) = {(got[:3, l] / naive).tolist()}, water table inside: {inside.tolist()}")
        seen += int(inside.sum())                                   # the rows the README's argument rests on
        assert np.all(got[:3, l][inside] > 2.0 * naive[inside])
    assert seen >= 1 and np.isnan(got[3:]).all()


# ---- 8. the CLI --------------------------------------------------------------------------------------------------------
COV_KEYS = {"theta_cov_node_stride", "theta_cov_nodes", "theta_cov_depth_cm", "theta_cov_rows", "theta_cov_count",
            "theta_cov_outside", "theta_cov", "wtd_theta_cov_cm", "wtd_var_cm2", "theta_wtd_corr"}
GAIN_KEYS = {"theta_sensor_sigma", "theta_sensor_gain"}


@pytest.mark.parametrize("n_points", [0, 2])
def test_cli_block_writes_the_datasets_and_leaves_the_rest_alone(tmp_path, monkeypatch, capsys, n_points):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    params = cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    pts = {"Points": [{"Soil_Properties": {"n": n}} for n in (1.6, 2.4)]} if n_points else {}
    lead = (n_points,) if n_points else ()
    blocks = (("plain", {}), ("nogain", {"Covariance": {"Node_Stride": 4}}),
              ("cov", {"Covariance": {"Node_Stride": 4, "Sensor_Sigma": 0.02}}))
    files = {}
    for tag, extra in blocks:
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 64, "Seed": 3, "Days": 2, "Profiles": 48, **pts, **extra}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        capsys.readouterr()
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = (loadResults(tmp_path / f"Run_{tag}_ensemble.h5"), capsys.readouterr().out)
    (plain, log_plain), (nogain, _), (cov, log_cov) = files["plain"], files["nogain"], files["cov"]
    T = plain["moments"].shape[-1]
    R, n = (T - 1) // 48 + 1, 50
    assert set(nogain) - set(plain) == COV_KEYS and set(cov) - set(plain) == COV_KEYS | GAIN_KEYS
    assert int(cov["theta_cov_node_stride"]) == 4 and cov["theta_cov_nodes"].tolist() == list(range(0, D, 4))
    z = digest(WELL)[1].z
    assert _same(cov["theta_cov_depth_cm"], np.asarray(z, dtype=np.float64)[::4])
    assert cov["theta_cov_rows"].tolist() == list(range(0, T, 48)) and int(cov["theta_cov_outside"]) == 0
    assert cov["theta_cov_count"].shape == lead + (R,) and np.array_equal(cov["theta_cov_count"], cov["profile_count"])
    for key, shape in (("theta_cov", (R, n, n)), ("wtd_theta_cov_cm", (R, n)), ("wtd_var_cm2", (R,)), ("theta_wtd_corr", (R, n)),
                       ("theta_sensor_gain", (R, n))):
        assert cov[key].shape == lead + shape and cov[key].dtype == np.float64, key
    for key in ("theta_cov_node_stride", "theta_cov_nodes", "theta_cov_rows", "theta_cov_count", "theta_cov_outside"):
        assert cov[key].dtype == np.int64, key
    assert float(cov["theta_sensor_sigma"]) == 0.02
    C = cov["theta_cov"][..., :3, :, :]
    assert _same(C, np.swapaxes(C, -1, -2)) and np.isnan(cov["theta_cov"][..., 3:, :, :]).all()
    var = np.einsum("...ii->...i", C)
    assert np.all(var >= 0.0)
    # the diagonal against the profile statistics' sigma: theta is quantised to 2^-20 here (each value moves by at most
    # 2^-21) and to 2^-40 there, a sigma moves by no more than its values do
    sd = cov["theta_vol_std"][..., :3, ::4]
    assert np.all(np.abs(np.sqrt(var) - sd) <= 2.0 ** -21 + 2.0 ** -41 + 1e-12)
    # in [0, 1) wherever it is defined.  (These members leave one spin-up and share one water-table node for two days, so
    # here var wtd = 0 and the gain is NaN; the resume test asserts the range on spread states, where it is defined.)
    gain = cov["theta_sensor_gain"][..., :3, :]
    moving = cov["wtd_var_cm2"][..., :3] > 0
    assert np.all((gain[moving] >= 0.0) & (gain[moving] < 1.0)) and np.isnan(gain[~moving]).all()
    assert np.all(cov["wtd_var_cm2"][..., :3] >= 0.0) and np.isnan(cov["theta_wtd_corr"][..., :3, :][~moving]).all()
    assert np.isnan(cov["theta_sensor_gain"][..., 3:, :]).all()
    if n_points:
        assert not _same(cov["theta_cov"][0], cov["theta_cov"][1])  # the points differ
    for k in COV_KEYS:
        assert _same(nogain[k], cov[k]), k
    for k in plain:                                                 # every other dataset, byte for byte
        assert _same(plain[k], cov[k]) and _same(plain[k], nogain[k]), k
    who = "Sweep 2 points x64" if n_points else "Ensemble x64"
    assert f" [{who}] covariance: 50 nodes on 3 rows\n" in log_cov and "covariance" not in log_plain


def test_two_ranks_sharing_the_card_write_what_one_rank_writes(tmp_path):
    params = cli_params(tmp_path)
    params["Ensemble"] = {"Members": 250, "Seed": 5, "Days": 1, "Profiles": 24,
                          "Covariance": {"Node_Stride": 4, "Sensor_Sigma": 0.02}}
    one, log1 = run_cli_ranks(tmp_path, "one", params, 1)
    two, log2 = run_cli_ranks(tmp_path, "two", params, 2)
    assert COV_KEYS | GAIN_KEYS <= set(one) and set(one) == set(two)
    assert int(one["gpus"]) == 1 and int(two["gpus"]) == 2 and np.all(one["theta_cov_count"][:3] == 250)
    for k in one:
        if k != "gpus":
            assert _same(one[k], two[k]), k
    line = [s for s in log1.splitlines() if "covariance:" in s]
    assert line == [" [Ensemble x250] covariance: 50 nodes on 3 rows"] and line == [s for s in log2.splitlines() if "covariance:" in s]


# ---- 9. refusals through the handle ------------------------------------------------------------------------------------
def test_refusals():
    from hydromodel_amd._lib import HcError
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(WELL)
    st = EnsembleStepper(cols, forcing, 2)
    try:
        st.set_state(golden(f"g1_tables_{WELL}.npz")["initial_cond"])
        st.set_noise_philox(1, 0)

        def off():
            return st.theta_cov_layout() == (0, 0, 0) and st.theta_cov_stride == 0

        with pytest.raises(HcError, match="needs the profile statistics"):
            st.set_theta_cov(1)                                     # no profile statistics
        assert off()
        st.set_profile_stats(48)
        st.set_theta_cov(0)                                         # 0 = off, no error
        assert off()
        with pytest.raises(HcError, match="is off"):
            st.theta_cov_table()
        for bad, message in ((-1, r"node stride -1 \(>= 1; 0 = off\)"), (D + 1, "node stride 201 exceeds the column's 200 nodes")):
            with pytest.raises(HcError, match=message):
                st.set_theta_cov(bad)
            assert off()
        st.set_theta_cov(D)                                         # the largest stride: one node and the water table
        assert st.theta_cov_layout() == (D, 1, 6)
        st.set_theta_cov(5)
        assert st.theta_cov_layout()[:2] == (5, 40)
        st.set_profile_stats(24)                                    # re-creates what the table is keyed to: off
        assert off()
        st.set_theta_cov(5)
        st.set_profile_stats(0)
        assert off()
        with pytest.raises(HcError, match="is off"):
            st.theta_cov_outside()
    finally:
        st.close()
    # the words cap: 581 nodes at node stride 1 are 170 236 words a row, 8761 rows of them are beyond 2^30 words
    _, deep, f581 = digest(581)
    st = EnsembleStepper(deep, f581, 2)
    try:
        st.set_profile_stats(2)
        with pytest.raises(HcError, match="exceed HC_THETA_COV_MAX_WORDS.*larger node stride or a larger profile stride"):
            st.set_theta_cov(1)
        assert st.theta_cov_layout() == (0, 0, 0)
        st.set_theta_cov(8)                                         # the first way out
        assert st.theta_cov_layout()[:2] == (8, 73)
    finally:
        st.close()
