"""Ensemble soil-moisture histograms counted on the GPU (include/hydrocol.h hc_set_theta_hist): the int32 table against the
NumPy restatement of the binning over hc_model_nodes' theta, its independence of launch length, member split, parameter
points and handles, no side effects on the run or on the profile statistics, the outside count, resume, the refusals and
the CLI's "Ensemble": {"Profile_Distribution": ...} block.  Every input keeps theta inside [0, 1], and every test says so:
the outside count is 0 wherever the kernel ran."""
import json
from functools import lru_cache

import numpy as np
import pytest

from helpers import cli_params, digest, digest_point, golden, run_cli_ranks
from test_gpu_enkf import _spread

pytestmark = pytest.mark.gpu

ROWS = 96                                                   # two days


def _stepper(well, N, stride, bins, points=None, seed=7, offset=0, bases=None, psi=None):
    """A handle on `well` with profile statistics at `stride` and, for bins > 0, the theta histograms; row 0 counted."""
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(well)
    st = EnsembleStepper(points or cols, forcing, N)
    st.set_state(_spread(golden(f"g1_tables_{well}.npz")["initial_cond"], N) if psi is None else psi)
    st.set_noise_philox(seed, offset)
    if bases is not None:
        st.set_point_member_bases(np.asarray(bases))
    st.set_profile_stats(stride)
    if bins:
        st.set_theta_hist(bins)
    st.profile_snapshot(0)
    return st, cols, forcing


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1, 2. exactness -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("well, N, rows, B", [
    (200, 67, 4, 32), (200, 67, 4, 128),        # three full node tiles and one of 8 lanes; 67 = 16 rounds of 4 waves + 3
    (300, 3, 2, 64),                            # fewer members than waves
])
def test_every_row_equals_the_restated_binning_of_the_models_theta(well, N, rows, B):
    from hydromodel_amd.stepper import theta_hist_of
    st, cols, forcing = _stepper(well, N, 1, B)
    try:
        want, outside = theta_hist_of(st.model_nodes()["theta"], B)      # row 0: the initial state
        assert outside == 0
        table = st.theta_hist_table()
        assert table.shape == (1, forcing.dim_t, cols.dim_d, B) and table.dtype == np.int32
        assert np.array_equal(table[0, 0], want) and not table[0, 1:].any()
        assert len({tuple(r) for r in want}) > 2                         # the nodes' members sit in different bins
        for r in range(1, rows + 1):
            assert forcing.wtd_obs[r] >= 0
            st.step_rows(r, 1)
            want, outside = theta_hist_of(st.model_nodes()["theta"], B)
            table = st.theta_hist_table()
            assert outside == 0 and np.array_equal(table[0, r], want), r
            assert not table[0, r + 1:].any()
        count = st.profile_stats()["count"]
        assert np.all(count[:rows + 1] == N) and np.array_equal(table[0].sum(axis=-1), np.broadcast_to(count[:, None], table.shape[1:3]))
        assert st.theta_hist_outside() == 0
    finally:
        st.close()


# ---- 3. independence of the split ------------------------------------------------------------------------------------
def _run(N, bins, rpl=0, offset=0, points=None, bases=None, psi=None):
    """(theta table, profile table) after two days at stride 48 on well 200."""
    st, _, _ = _stepper(200, N, 48, bins, offset=offset, points=points, bases=bases, psi=psi)
    try:
        if rpl:
            st.set_rows_per_launch(rpl)
        st.step_rows(1, ROWS)
        assert st.profile_overflow() == 0
        if not bins:
            return None, st.profile_table()
        assert st.theta_hist_outside() == 0
        return st.theta_hist_table(), st.profile_table()
    finally:
        st.close()


@lru_cache(maxsize=None)
def _spread_1000():
    psi = _spread(golden("g1_tables_200.npz")["initial_cond"], 1000)
    psi.setflags(write=False)
    return psi


@lru_cache(maxsize=None)
def _whole_1000():
    return _run(1000, 128, psi=_spread_1000())


def test_the_table_does_not_depend_on_the_launch_length():
    hist, prof = _whole_1000()
    assert hist.shape == (1, (digest(200)[2].dim_t - 1) // 48 + 1, 200, 128)
    assert np.all(hist[0, :3].sum(axis=-1) == 1000) and not hist[0, 3:].any()
    short, prof_short = _run(1000, 128, rpl=7, psi=_spread_1000())
    assert _same(short, hist) and _same(prof_short, prof)
    assert _same(_run(1000, 0, psi=_spread_1000())[1], prof)        # the profile table of a run without the histogram


def test_one_handle_equals_two_handles_summed():
    hist, prof = _whole_1000()
    psi = _spread_1000()
    a, prof_a = _run(512, 128, rpl=5, offset=0, psi=psi[:512])
    b, prof_b = _run(488, 128, rpl=11, offset=512, psi=psi[512:])
    assert _same(a + b, hist) and _same(prof_a + prof_b, prof)


def test_two_parameter_points_one_handle_equals_two_handles_summed():
    _, base, _ = digest(200)
    _, other, _ = digest_point("a003")
    pts = [base, other]
    psi = _spread_1000()                                           # point 0: members [0, 500), point 1: [500, 1000)

    def members(lo, hi):
        return np.concatenate([psi[lo:hi], psi[500 + lo:500 + hi]])

    whole, prof = _run(1000, 64, points=pts, bases=[0, 5000], psi=psi)
    a, prof_a = _run(512, 64, rpl=5, points=pts, bases=[0, 5000], psi=members(0, 256))
    b, prof_b = _run(488, 64, rpl=11, points=pts, bases=[256, 5256], psi=members(256, 500))
    assert whole.shape[0] == 2 and np.all(whole[:, :3].sum(axis=-1) == 500)
    assert not _same(whole[0], whole[1])                           # the points differ
    assert _same(a + b, whole) and _same(prof_a + prof_b, prof)
    assert _same(_run(1000, 0, points=pts, bases=[0, 5000], psi=psi)[1], prof)


# ---- 4. the run is left alone ----------------------------------------------------------------------------------------
def test_the_histogram_leaves_the_run_alone():
    """States, wtd_out, moments, counters and the profile table with the histogram on equal those with it off."""
    res = []
    for bins in (0, 128):
        st, _, _ = _stepper(300, 64, 3, bins, seed=3)
        try:
            out = st.step_rows(1, ROWS, want_wtd=True)
            res.append((st.get_state(), out["wtd"], st.moments(), st.counters(), st.profile_table()))
            if bins:
                assert st.theta_hist_outside() == 0 and np.all(st.theta_hist_table()[0, :ROWS // 3 + 1].sum(axis=-1) == 64)
        finally:
            st.close()
    (a_psi, a_w, a_m, a_c, a_p), (b_psi, b_w, b_m, b_c, b_p) = res
    assert _same(a_psi, b_psi) and _same(a_w, b_w) and np.array_equal(a_m, b_m) and a_c == b_c and _same(a_p, b_p)


# ---- 5. the outside count --------------------------------------------------------------------------------------------
def test_the_outside_count_travels_with_the_table():
    st, cols, forcing = _stepper(200, 8, 48, 32)
    try:
        assert st.theta_hist_outside() == 0
        t = np.random.default_rng(5).integers(0, 1000, st.theta_hist_table().shape).astype(np.int32)
        for outside in (7, (1 << 40) + 3):                         # both words of the 64-bit count
            st.set_theta_hist_table(t, outside=outside)
            assert st.theta_hist_outside() == outside and _same(st.theta_hist_table(), t)
        st.set_theta_hist_table(t)
        assert st.theta_hist_outside() == 0 and _same(st.theta_hist_table(), t)
        st.set_theta_hist_table(t, outside=9)
        st.reset_theta_hist()
        assert st.theta_hist_outside() == 0 and not st.theta_hist_table().any()
        from hydromodel_amd import _lib as L
        with pytest.raises(L.HcError, match="the table has"):      # without the count's two entries: another size
            L.check(st.lib.hc_set_theta_hist_table(st.h, L.iptr(t.reshape(-1)), t.size))
    finally:
        st.close()


# ---- 6. resume -------------------------------------------------------------------------------------------------------
def test_resume_from_a_dump_gives_the_uninterrupted_table(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(300)
    ic = golden("g1_tables_300.npz")["initial_cond"]
    kw = dict(seed=9, psi0=ic, profile_stride=3, theta_hist_bins=64)
    full = EnsembleSimulation(cols, forcing, 64, **kw)
    full.advance(ROWS)
    want, want_prof = full.theta_hist_table(), full.profile_table()
    assert full.stepper.theta_hist_outside() == 0
    full.close()
    first = EnsembleSimulation(cols, forcing, 64, **kw)
    first.advance(50)
    path = first.dump(tmp_path / "ckpt.h5")
    first.close()
    resumed = EnsembleSimulation.restore(path, cols, forcing)
    resumed.advance(ROWS - 50)
    got, got_prof, outside = resumed.theta_hist_table(), resumed.profile_table(), resumed.stepper.theta_hist_outside()
    bands = resumed.theta_distribution([0.05, 0.5, 0.95])
    resumed.close()
    assert resumed.theta_hist_bins == 64 and outside == 0
    assert want.shape == ((forcing.dim_t - 1) // 3 + 1, cols.dim_d, 64) and np.all(want[:ROWS // 3 + 1].sum(axis=-1) == 64)
    assert _same(got, want) and _same(got_prof, want_prof)
    q = bands["quantiles"]
    assert q.shape == (want.shape[0], 3, cols.dim_d) and np.all(np.isfinite(q[:ROWS // 3 + 1])) and np.isnan(q[ROWS // 3 + 1:]).all()
    assert np.all(q[:ROWS // 3 + 1, 0] <= q[:ROWS // 3 + 1, 2]) and np.all(bands["count"][:ROWS // 3 + 1] == 64)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------
def _bins(st):
    import ctypes as C
    n = C.c_int32(-1)
    assert st.lib.hc_get_theta_hist_bins(st.h, C.byref(n)) == 0
    return int(n.value)


def test_refusals():
    from hydromodel_amd._lib import HcError
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(300)
    st = EnsembleStepper([cols, cols], forcing, 2)
    try:
        st.set_state(golden("g1_tables_300.npz")["initial_cond"])
        st.set_noise_philox(1, 0)
        with pytest.raises(HcError, match="need the profile statistics"):
            st.set_theta_hist(128)                                 # no profile statistics
        assert _bins(st) == 0 and st.theta_hist_bins == 0
        st.set_profile_stats(48)
        for bad in (48, 16, 256, -32):
            with pytest.raises(HcError, match="32, 64 or 128"):
                st.set_theta_hist(bad)
            assert _bins(st) == 0
        st.set_theta_hist(32)
        assert _bins(st) == 32 and st.theta_hist_table().shape == (2, (forcing.dim_t - 1) // 48 + 1, 300, 32)
        st.set_theta_hist(0)
        assert _bins(st) == 0
        with pytest.raises(HcError, match="are off"):
            st.theta_hist_outside()
        st.set_theta_hist(64)
        st.set_profile_stats(24)                                   # re-creates what the histogram is keyed to: off
        assert _bins(st) == 0 and st.theta_hist_bins == 0
        with pytest.raises(HcError, match="are off"):
            st.theta_hist_outside()
        # a table over the cap: 2 points x 17 521 rows x 300 nodes x 128 bins > 2^30 entries; the argument check alone
        st.set_profile_stats(1)
        assert 2 * forcing.dim_t * 300 * 128 > 1 << 30
        with pytest.raises(HcError, match="exceed HC_WTD_HIST_MAX_ENTRIES"):
            st.set_theta_hist(128)
        assert _bins(st) == 0
    finally:
        st.close()


# ---- 8. the CLI ------------------------------------------------------------------------------------------------------
THETA_KEYS = {"theta_hist", "theta_hist_rows", "theta_hist_count", "theta_hist_bins", "theta_hist_outside",
              "theta_quantile_levels", "theta_quantile"}


@pytest.mark.parametrize("n_points", [0, 2])
def test_cli_block_writes_the_datasets_and_leaves_the_rest_alone(tmp_path, monkeypatch, capsys, n_points):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    from hydromodel_amd.stepper import theta_distribution
    params = cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    pts = {"Points": [{"Soil_Properties": {"n": n}} for n in (1.6, 2.4)][:n_points]} if n_points else {}
    levels = [0.05, 0.5, 0.95]
    files = {}
    for tag, extra in (("plain", {}), ("theta", {"Profile_Distribution": {"Bins": 64, "Quantiles": levels}})):
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 128, "Seed": 3, "Days": 2, "Profiles": 48, **pts, **extra}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        capsys.readouterr()
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = (loadResults(tmp_path / f"Run_{tag}_ensemble.h5"), capsys.readouterr().out)
    (plain, log_plain), (theta, log_theta) = files["plain"], files["theta"]
    lead = (n_points,) if n_points else ()
    T, D = plain["moments"].shape[-1], plain["initial_cond"].shape[-1]
    R = (T - 1) // 48 + 1
    assert set(theta) - set(plain) == THETA_KEYS
    assert theta["theta_hist"].shape == lead + (R, D, 64) and theta["theta_hist"].dtype == np.int32
    assert theta["theta_hist_rows"].tolist() == list(range(0, T, 48))
    assert theta["theta_hist_count"].shape == lead + (R,) and int(theta["theta_hist_bins"]) == 64
    assert int(theta["theta_hist_outside"]) == 0 and theta["theta_quantile_levels"].tolist() == levels
    assert theta["theta_quantile"].shape == lead + (R, 3, D)
    assert np.array_equal(theta["theta_hist_count"], theta["profile_count"])
    assert np.all(theta["theta_hist"][..., :3, :, :].sum(axis=-1) == 128) and not theta["theta_hist"][..., 3:, :, :].any()
    d = theta_distribution(theta["theta_hist"], levels, 64, 48)
    assert _same(d["quantiles"], theta["theta_quantile"]) and np.isnan(theta["theta_quantile"][..., 3:, :, :]).all()
    # the median's bin holds the mean wherever the members share one bin
    one_bin = (theta["theta_hist"][..., :3, :, :] == 128).any(axis=-1)
    assert one_bin.any()
    assert np.all(np.abs(theta["theta_quantile"][..., :3, 1, :] - theta["theta_vol_mean"][..., :3, :])[one_bin] <= 0.5 / 64)
    for k in plain:                                          # every other dataset, byte for byte
        assert _same(plain[k], theta[k]), k
    who = f"Sweep 2 points x128" if n_points else "Ensemble x128"
    assert f" [{who}] theta bands: 3 levels on 3 rows, 64 bins\n" in log_theta and "theta bands" not in log_plain


@pytest.mark.parametrize("sweep", [False, True])
def test_two_ranks_sharing_the_card_write_the_bands_one_rank_writes(tmp_path, sweep):
    params = cli_params(tmp_path)
    ens = {"Members": 250, "Seed": 5, "Days": 2, "Profiles": 24,
           "Profile_Distribution": {"Bins": 32, "Quantiles": [0.1, 0.5, 0.9]}}
    if sweep:                                                # three points dealt to two ranks: 2 + 1
        ens.update(Members=32, Points=[{"Soil_Properties": {"n": n}} for n in (1.6, 2.0, 2.4)])
    params["Ensemble"] = ens
    one, log1 = run_cli_ranks(tmp_path, "one", params, 1)
    two, log2 = run_cli_ranks(tmp_path, "two", params, 2)
    assert THETA_KEYS <= set(one) and set(one) == set(two)
    assert int(one["gpus"]) == 1 and int(two["gpus"]) == 2 and int(one["theta_hist_outside"]) == 0
    members = 32 if sweep else 250
    assert np.all(one["theta_hist"][..., :5, :, :].sum(axis=-1) == members)
    for k in one:
        if k != "gpus":
            assert _same(one[k], two[k]), k
    line = [s for s in log1.splitlines() if "theta bands" in s]
    assert len(line) == 1 and line == [s for s in log2.splitlines() if "theta bands" in s]
