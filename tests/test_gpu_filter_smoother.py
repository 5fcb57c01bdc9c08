"""The fixed-lag smoother of the water table by ancestry on the GPU (include/hydrocol.h hc_set_filter_smoother): off means
off and on leaves the run alone; the tables against the NumPy restatement (stepper.filter_smoother_of) fed a twin handle's
rows and ancestors, as bytes; invariance under launch length, point order and the dealing of a sweep's points; the neutral
filter against hc_set_wtd_hist; K = 0; the edges of the distinct count and the gather; unobserved rows; the other filter
options and the period totals; the checkpoint; the ring; the refusals; the CLI's "Smoother" block on one and two ranks.
Every case calls the smoother's entry points, so none passes without them.

Shapes: well 1 (D = 101), 96 rows, filter stride 12, smoother stride 6, K = 4, sigma = 1.5 dz, 200 members unless stated."""
import json
import re

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the refusals below set a shard, whose buffer is torch's)

from helpers import WELLS, digest, forcing_frame, golden
from helpers import cli_params as _cli_params, run_cli_ranks as _run_ranks

pytestmark = pytest.mark.gpu
FS, S, K, ROWS = 12, 6, 4, 96
NODES, VALUES, SIGMAS = [6, 45], [0.24, 0.36], np.array([0.05, 0.08])


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _spread(psi0, N, seed=12, width=60.0):
    """[N][D]: the initial profile shifted by a per-member offset, uniform over +-width cm (as test_gpu_filter_window's)"""
    return np.asarray(psi0)[None, :] + np.random.default_rng(seed).uniform(-width, width, size=N)[:, None]


def _handle(N, P=1, sigma_dz=1.5, setup=None, unobserved=()):
    """Well 1, P copies of the point, the members spread, Philox noise, the filter on at stride 12, then ``setup(st)``
    (the other options) and the rows that lose their observation."""
    from hydromodel_amd import _lib as L
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(1)
    assert (np.asarray(forcing.wtd_obs[1:ROWS + 1]) >= 0).all()
    st = EnsembleStepper([cols] * P if P > 1 else cols, forcing, N)
    st.set_state(_spread(golden("g1_tables_1.npz")["initial_cond"], N))
    st.set_noise_philox(7, 0)
    st.set_filter(FS, sigma_dz * cols.dz, 3)
    if setup is not None:
        setup(st)
    for r in unobserved:
        L.check(st.lib.hc_set_forcing_row(st.h, r, float(forcing.precip[r]), float(forcing.atm[r]),
                                          int(forcing.daylight[r]), -1))
    obs = np.array(forcing.wtd_obs, dtype=np.int32)
    obs[list(unobserved)] = -1
    return st, obs


def _twin(N, P=1, rows=ROWS, **kw):
    """A handle without the smoother stepped one row at a time: every row's water-table indices and, wherever the filter's
    table counted members, the row's ancestors -- what the restatement is fed."""
    st, obs = _handle(N, P, **kw)
    try:
        w, anc = np.zeros((st.T, N), dtype=np.int32), {}
        for r in range(1, rows + 1):
            w[r] = st.step_rows(r, 1, want_wtd=True)["wtd"][0]
            if r % FS == 0 and st.filter_table()[0, r // FS, 0] > 0:
                anc[r] = st.filter_ancestors()
        return dict(w=w, anc=anc, obs=obs, psi=st.get_state(), base=st.filter_base(), table=st.filter_table(),
                    moments=np.asarray(st.moments()))
    finally:
        st.close()


def _want(twin, Np, D=101, stride=S, lag=K, rows=ROWS):
    from hydromodel_amd.stepper import filter_smoother_of
    return filter_smoother_of(twin["w"], twin["anc"], stride, lag, Np, D, twin["obs"], rows)


def _run(N, P=1, stride=S, lag=K, launch=0, rows=ROWS, **kw):
    """The handle under test: the smoother on, ``rows`` rows in one call (``launch`` = 0) or in calls of ``launch`` rows"""
    st, _ = _handle(N, P, **kw)
    try:
        st.set_filter_smoother(stride, lag)
        assert st.filter_smoother_layout() == (stride, lag, (st.T - 1) // stride + 1)
        if launch:
            for r in range(1, rows + 1, launch):
                st.step_rows(r, min(launch, rows + 1 - r))
        else:
            st.step_rows(1, rows)
        got = dict(hist=st.filter_smoother_hist(), paths=st.filter_smoother_paths(), psi=st.get_state(),
                   base=st.filter_base(), table=st.filter_table(), moments=np.asarray(st.moments()))
        got["ring_w"], got["ring_id"], got["ring_rows"], got["last"] = st.filter_smoother_ring()
        st.filter_smoother_flush()
        got.update(hist_flushed=st.filter_smoother_hist(), paths_flushed=st.filter_smoother_paths())
        st.filter_smoother_flush()                                    # a second flush counts nothing twice
        assert _same(got["hist_flushed"], st.filter_smoother_hist()) and st.filter_smoother_ring()[2].tolist() == [-1] * (lag + 1)
        return got
    finally:
        st.close()


def _check(got, want, ring=True):
    for k in ("hist", "paths", "hist_flushed", "paths_flushed") + (("ring_w", "ring_id", "ring_rows") if ring else ()):
        assert _same(got[k], want[k]), k


@pytest.fixture(scope="module")
def twin200():
    return _twin(200)


@pytest.fixture(scope="module")
def run200():
    return _run(200)


# ---- 1. off and on leave the run alone ------------------------------------------------------------------------------------
def test_off_and_on_leave_the_run_alone(twin200, run200):
    from hydromodel_amd._lib import HcError

    def plain(off):
        st, _ = _handle(200)
        try:
            st.set_wtd_hist(S)
            if off:
                st.set_filter_smoother(S, K)
                st.set_filter_smoother(0)
                assert st.filter_smoother_layout() == (0, 0, 0)
                with pytest.raises(HcError, match="smoother is off"):
                    st.filter_smoother_hist()
            st.step_rows(1, ROWS)
            return dict(psi=st.get_state(), base=st.filter_base(), table=st.filter_table(), moments=np.asarray(st.moments()),
                        hist=st.wtd_hist_table(), anc=st.filter_ancestors())
        finally:
            st.close()

    never, off = plain(False), plain(True)
    for k in never:
        assert _same(never[k], off[k]), k
    for k in ("psi", "base", "table", "moments"):
        assert _same(never[k], run200[k]) and _same(never[k], twin200[k]), k
    assert run200["hist_flushed"].sum() > 0


# ---- 2. exact against the restatement -------------------------------------------------------------------------------------
def test_tables_equal_the_restatement_before_and_after_the_flush(twin200, run200):
    assert sorted(twin200["anc"]) == list(range(FS, ROWS + 1, FS))
    assert any(np.unique(a).size < 200 for a in twin200["anc"].values())          # the filter really resampled
    want = _want(twin200, 200)
    _check(run200, want)
    assert run200["last"] == ROWS
    assert run200["paths"][0, 1:13, 1].tolist() == [6 * (j + K) for j in range(1, 13)]
    assert (run200["paths"][0, 13:, 1] == -1).all() and run200["paths_flushed"][0, 13:17, 1].tolist() == [ROWS] * 4
    assert (run200["hist"][0, 1:13].sum(axis=-1) == 200).all() and run200["hist"][0, 0].sum() == 0
    assert run200["paths"][0, 1:13, 0].min() < 200 and run200["paths_flushed"][0, 16, 0] <= 200


# ---- 3. launch length -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("launch", [1, 7])
def test_launch_length_changes_no_byte(run200, launch):
    other = _run(200, launch=launch)
    _check(other, run200)


# ---- 4. the neutral filter ------------------------------------------------------------------------------------------------
def test_flat_weights_give_the_forecast_histograms_and_every_path():
    st, _ = _handle(200)
    try:
        st.set_filter(FS, 1e30, 3)
        st.set_wtd_hist(S)
        st.set_filter_smoother(S, K)
        st.step_rows(1, ROWS)
        before, forecast = st.filter_smoother_hist(), st.wtd_hist_table()
        assert _same(before[:, 1:13], forecast[:, 1:13]) and before[:, 13:].sum() == 0
        assert (st.filter_smoother_paths()[0, 1:13, 0] == 200).all()
        st.filter_smoother_flush()
        assert _same(st.filter_smoother_hist(), forecast) and (st.filter_smoother_paths()[0, 1:17, 0] == 200).all()
    finally:
        st.close()


# ---- 5. K = 0 -------------------------------------------------------------------------------------------------------------
def test_lag_zero_is_the_analysis_of_the_row_itself(twin200):
    got = _run(200, lag=0)
    D = 101
    for j in range(1, 17):
        r = S * j
        v = twin200["w"][r][twin200["anc"][r]] if r in twin200["anc"] else twin200["w"][r]
        assert np.array_equal(got["hist"][0, j], np.bincount(v[v < D], minlength=D)), r
        assert got["paths"][0, j].tolist() == [np.unique(twin200["anc"][r]).size if r in twin200["anc"] else 200, r]
    assert _same(got["hist"], got["hist_flushed"]) and got["ring_rows"].tolist() == [-1]
    _check(got, _want(twin200, 200, lag=0))


# ---- 6. the edges of the distinct count and the gather --------------------------------------------------------------------
@pytest.mark.parametrize("P, Np", [(3, 100), (2, 1), (1, 65), (1, 257), (1, 4100)])
def test_point_boundaries_wave_block_and_slice_edges(P, Np):
    twin = _twin(P * Np, P)
    got = _run(P * Np, P)
    _check(got, _want(twin, Np))
    emitted = got["paths_flushed"][:, 1:17, 0]
    assert emitted.min() >= 1 and emitted.max() <= Np
    if Np > 1:
        assert emitted.min() < Np                                   # the ancestry merged paths


# ---- 7. a sweep -----------------------------------------------------------------------------------------------------------
SWEEP_N, SWEEP_MPP = (1.6, 2.0, 2.4), 70


def _sweep_handle(ids, psi_all):
    from hydromodel_amd.digest import ColumnTables, ForcingDigest
    from hydromodel_amd.stepper import EnsembleStepper
    from hydromodel_amd.synthetic import default_parameters
    pts = []
    for k in ids:
        params = default_parameters()
        params["Soil_Properties"]["n"] = SWEEP_N[k]
        cols = ColumnTables(params, WELLS[1])
        pts.append((cols, ForcingDigest(params, forcing_frame(1), cols)))
    st = EnsembleStepper([c for c, _ in pts], pts[0][1], len(ids) * SWEEP_MPP)
    try:
        st.set_generic_exponents(True)
        st.set_state(np.concatenate([psi_all[k * SWEEP_MPP:(k + 1) * SWEEP_MPP] for k in ids]))
        st.set_noise_philox(21, ids[0] * SWEEP_MPP)
        if len(ids) > 1:
            st.set_point_member_bases(np.array(ids, dtype=np.int64) * SWEEP_MPP)
        st.set_filter(FS, 2.0 * st.cols.dz, 8)
        st.set_filter_smoother(S, K)
        st.step_rows(1, 72)
        out = dict(hist=st.filter_smoother_hist(), paths=st.filter_smoother_paths(), table=st.filter_table())
        st.filter_smoother_flush()
        out.update(hist_flushed=st.filter_smoother_hist(), paths_flushed=st.filter_smoother_paths())
        return out
    finally:
        st.close()


def test_a_sweep_in_one_handle_in_the_other_order_and_dealt_to_two(monkeypatch):
    psi_all = _spread(golden("g1_tables_1.npz")["initial_cond"], 3 * SWEEP_MPP, seed=4)
    monkeypatch.delenv("HYDROCOL_POINT_ORDER", raising=False)
    whole = _sweep_handle([0, 1, 2], psi_all)
    assert (whole["paths"][:, 1:9, 1] > 0).all() and whole["paths_flushed"][:, 1:13, 0].min() < SWEEP_MPP
    assert not _same(whole["hist"][0], whole["hist"][2])
    monkeypatch.setenv("HYDROCOL_POINT_ORDER", "fixed")
    other = _sweep_handle([0, 1, 2], psi_all)
    monkeypatch.delenv("HYDROCOL_POINT_ORDER", raising=False)
    for k in whole:
        assert _same(whole[k], other[k]), k
    for ids in ([0, 2], [1]):
        part = _sweep_handle(ids, psi_all)
        for j, k in enumerate(ids):
            for key in whole:
                assert whole[key][k].tobytes() == part[key][j].tobytes(), (ids, k, key)


# ---- 8. unobserved rows ---------------------------------------------------------------------------------------------------
def test_unobserved_record_and_assimilation_rows():
    lost = (18, 48, 54)                      # a record row, an assimilation row (a record row too) and the row after it
    twin = _twin(200, unobserved=lost)
    assert sorted(twin["anc"]) == [12, 24, 36, 60, 72, 84, 96]        # no resampling, so no gather, on row 48
    got = _run(200, unobserved=lost)
    _check(got, _want(twin, 200))
    for r in lost:
        assert got["hist_flushed"][0, r // S].sum() == 0 and got["paths_flushed"][0, r // S].tolist() == [0, -1]
    assert got["paths_flushed"][0, 42 // S].tolist()[1] == 42 + S * K


# ---- 9. together with the other options -----------------------------------------------------------------------------------
def _record(T, rows=(48, 96)):
    v = np.full((T, 2), np.nan)
    for r in rows:
        v[r] = VALUES
    return v


OPTIONS = {
    "soil_moisture": lambda st: st.set_filter_soil_moisture(NODES, _record(st.T), SIGMAS),
    "tempering": lambda st: st.set_filter_tempering(0.5),
    "window": lambda st: st.set_filter_window((3, 6)),
    "rejuvenation": lambda st: st.set_filter_rejuvenation(0.95),
    "periods": lambda st: st.set_period_totals([48, 96]),
}


@pytest.mark.parametrize("option", sorted(OPTIONS))
def test_with_the_other_options_the_tables_follow_the_runs_ancestors(option, twin200):
    twin = _twin(200, setup=OPTIONS[option])
    got = _run(200, setup=OPTIONS[option])
    _check(got, _want(twin, 200))
    for k in ("psi", "base", "table", "moments"):
        assert _same(got[k], twin[k]), k
    if option in ("soil_moisture", "tempering", "window"):
        assert any(not np.array_equal(twin["anc"][r], twin200["anc"][r]) for r in twin["anc"])   # the option mattered


def test_period_accumulators_are_those_of_the_run_without_the_smoother():
    def run(smoother):
        st, _ = _handle(200, setup=OPTIONS["periods"])
        try:
            if smoother:
                st.set_filter_smoother(S, K)
            st.step_rows(1, 60)
            mid = st.period_totals_acc()
            st.step_rows(61, 36)
            return mid, st.period_totals_acc(), st.period_totals_table()
        finally:
            st.close()

    for a, b in zip(run(False), run(True)):
        assert _same(a, b)


# ---- 10. checkpoint -------------------------------------------------------------------------------------------------------
def test_dump_between_a_store_and_its_emission_resumes_bit_for_bit(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(1)
    psi0 = _spread(golden("g1_tables_1.npz")["initial_cond"], 96)
    kw = dict(seed=6, psi0=psi0, filter_stride=FS, filter_sigma_cm=1.5 * cols.dz, filter_smoother={"stride": S, "lag_rows": S * K})

    def state(sim):
        return [sim.stepper.get_state(), sim.filter_table(), sim.moments(), sim.stepper.filter_base(),
                sim.stepper.filter_smoother_hist(), sim.stepper.filter_smoother_paths(), *sim.stepper.filter_smoother_ring()[:3]]

    whole = EnsembleSimulation(cols, forcing, 96, **kw)
    try:
        whole.advance(40)
        ring = whole.stepper.filter_smoother_ring()
        assert sorted(ring[2].tolist()) == [-1, 18, 24, 30, 36] and ring[3] == 40          # row 12 left on row 36
        path = whole.dump(tmp_path / "ck.h5")
        whole.advance(56)
        want = state(whole)
        smoothed = whole.filter_smoothed((0.05, 0.5, 0.95))
    finally:
        whole.close()
    back = EnsembleSimulation.restore(path, cols, forcing)
    try:
        assert back.next_row == 41 and back.filter_smoother == (S, K)
        for a, b in zip(ring, back.stepper.filter_smoother_ring()):
            assert _same(a, b) if isinstance(a, np.ndarray) else a == b
        back.advance(56)
        got = state(back)
        again = back.filter_smoothed((0.05, 0.5, 0.95))
    finally:
        back.close()
    for a, c in zip(want, got):
        assert _same(a, c)
    for k in smoothed:
        assert _same(smoothed[k], again[k]), k
    assert smoothed["rows"].tolist() == list(range(0, forcing.dim_t, S)) and smoothed["lag_rows"][1:17].tolist() == [24] * 12 + [18, 12, 6, 0]
    assert (smoothed["count"][1:17] == 96).all() and np.isfinite(smoothed["crps_cm"][1:17]).all()
    assert (smoothed["unique_paths"][1:17] >= 1).all() and smoothed["quantile_cm"].shape == (smoothed["rows"].size, 3)
    plain = EnsembleSimulation(cols, forcing, 96, **{k: v for k, v in kw.items() if k != "filter_smoother"})
    try:
        plain.advance(8)
        keys = set(dict(np.load(plain.dump(tmp_path / "plain.npz"))))
    finally:
        plain.close()
    assert not any("smoother" in k for k in keys)


# ---- 11. the ring ---------------------------------------------------------------------------------------------------------
def test_ring_ids_are_non_decreasing_within_every_point_after_three_resamplings():
    st, _ = _handle(300, 3)
    try:
        st.set_filter_smoother(S, 6)                                         # rows 6 and 12 stay until rows 42 and 48
        st.step_rows(1, 40)
        w, ids, rows, last = st.filter_smoother_ring()
        assert sorted(rows.tolist()) == [-1, 6, 12, 18, 24, 30, 36] and last == 40
        live = ids[rows >= 0].reshape(-1, 3, 100)
        assert (np.diff(live, axis=-1) >= 0).all() and live.min() == 0 and live.max() <= 99
        assert np.unique(ids[list(rows).index(12)][:100]).size < 100      # row 12 has met three resamplings
        assert (w[rows < 0] == 0).all() and (ids[rows < 0] == 0).all() and w.max() < 101
        st.set_filter_smoother_ring(w, ids, rows, last)                      # what came out goes back in
        for a, b in zip((w, ids, rows, last), st.filter_smoother_ring()):
            assert _same(a, b) if isinstance(a, np.ndarray) else a == b
        st.reset_filter_smoother()
        assert st.filter_smoother_ring()[2].tolist() == [-1] * 7 and st.filter_smoother_hist().sum() == 0
        assert (st.filter_smoother_paths() == np.array([0, -1])).all()
    finally:
        st.close()


# ---- 12. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_and_what_turns_the_smoother_off():
    from hydromodel_amd._lib import HcError, check, iptr, lptr
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(1)
    st = EnsembleStepper(cols, forcing, 64)
    st.set_state(_spread(golden("g1_tables_1.npz")["initial_cond"], 64))
    st.set_noise_philox(7, 0)

    def raw(stride, lag):
        return check(st.lib.hc_set_filter_smoother(st.h, stride, lag))

    try:
        with pytest.raises(HcError, match="the particle filter is off"):
            raw(S, K)
        st.set_enkf(48, 5.0, 0.0, 1)
        with pytest.raises(HcError, match="the EnKF is on"):
            raw(S, K)
        st.set_enkf(0)
        st.set_filter(FS, 5.0, 1)
        with pytest.raises(HcError, match=r"lag = 65 outside \[0, 64\]"):
            raw(S, 65)
        with pytest.raises(HcError, match="lag = -1 outside"):
            raw(S, -1)
        with pytest.raises(HcError, match="stride = -1 must be >= 0"):
            raw(-1, 0)
        with pytest.raises(ValueError, match="lag must lie in"):
            st.set_filter_smoother(S, 65)
        assert st.filter_smoother == (0, 0) and st.filter_smoother_layout() == (0, 0, 0)
        st.set_filter_shard([0, 64], 0, None)
        with pytest.raises(HcError, match="do not carry the smoother's ring"):
            raw(S, K)                                                    # a shard set before the smoother
        st.set_filter_shard(None)
        st.set_filter_smoother(S, 64)
        assert st.filter_smoother_layout() == (S, 64, (st.T - 1) // S + 1)
        with pytest.raises(HcError, match="do not carry its ring"):
            st.set_filter_shard([0, 64], 0, None)                        # ... and the smoother set before a shard
        assert st.get_filter_shard() == (0, 0, 0)
        n = st.filter_smoother_hist().size
        bad = np.zeros(n + 1, dtype=np.int32)
        with pytest.raises(HcError, match=f"the table has {n} entries, not {n + 1}"):
            check(st.lib.hc_get_filter_smoother_hist(st.h, iptr(bad), n + 1))
        with pytest.raises(HcError, match="the table has"):
            check(st.lib.hc_set_filter_smoother_hist_table(st.h, iptr(bad), n + 1))
        with pytest.raises(HcError, match="the table has"):
            check(st.lib.hc_get_filter_smoother_paths(st.h, lptr(np.zeros(3, dtype=np.int64)), 3))
        w, ids, rows, _ = st.filter_smoother_ring()
        rows[1] = S
        w[1, 5] = 65536
        with pytest.raises(HcError, match=r"index 65536 \(plane 1, member 5\) outside \[0, 65535\]"):
            st.set_filter_smoother_ring(w, ids, rows)
        w[1, 5], ids[1, 5] = 3, 64
        with pytest.raises(HcError, match=r"id 64 \(plane 1, member 5\) outside \[0, 64\)"):
            st.set_filter_smoother_ring(w, ids, rows)
        ids[1, 5], rows[1] = 5, 2 * S
        with pytest.raises(HcError, match="row 12 is not a record row of plane 1"):
            st.set_filter_smoother_ring(w, ids, rows)
        st.set_filter(FS, 5.0, 1)                                        # hc_set_filter removes the smoother
        assert st.filter_smoother == (0, 0) and st.filter_smoother_layout() == (0, 0, 0)
        st.set_filter_smoother(S, K)
        st.set_noise_philox(9, 0)                                        # a new noise source turns the filter off
        assert st.filter_smoother == (0, 0) and st.filter_smoother_layout() == (0, 0, 0)
        with pytest.raises(HcError, match="smoother is off"):
            st.filter_smoother_flush()
    finally:
        st.close()


# ---- 13. the CLI ----------------------------------------------------------------------------------------------------------
SMOOTH_KEYS = {"smooth_rows", "smooth_count", "smooth_hist", "smooth_lag_rows", "smooth_unique_paths", "smooth_quantile_levels",
               "smooth_quantile_cm", "smooth_crps_cm", "smooth_crps_mean_cm", "smooth_stride", "smooth_lag"}


def test_cli_smoother_block_writes_the_datasets_and_the_closing_line(tmp_path, monkeypatch, capsys):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    params = _cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    files, logs = {}, {}
    filt = {"Stride": 24, "Sigma_cm": 10.0}
    for tag, extra in (("well", {"Filter": filt}),
                       ("ens", {"Filter": {**filt, "Smoother": {"Stride": 12, "Lag_rows": 36, "Quantiles": [0.1, 0.9]}}})):
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 64, "Seed": 3, "Days": 2, **extra}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = loadResults(tmp_path / f"Run_{tag}_ensemble.h5")
        logs[tag] = capsys.readouterr().out
    well, ens = files["well"], files["ens"]
    assert "smoother:" not in logs["well"] and not any(k.startswith("smooth_") for k in well)
    assert set(ens) - set(well) == SMOOTH_KEYS
    for k in well:
        assert _same(well[k], ens[k]), k
    assert ens["smooth_rows"].tolist() == list(range(12, 97, 12)) and int(ens["smooth_stride"]) == 12 and int(ens["smooth_lag"]) == 3
    assert ens["smooth_lag_rows"].tolist() == [36] * 5 + [24, 12, 0] and (ens["smooth_count"] == 64).all()
    assert ens["smooth_hist"].shape == (8, 200) and ens["smooth_hist"].dtype == np.int32
    assert ens["smooth_quantile_cm"].shape == (8, 2) and ens["smooth_quantile_levels"].tolist() == [0.1, 0.9]
    assert np.isfinite(ens["smooth_crps_cm"]).all() and 1 <= ens["smooth_unique_paths"].min() <= 64
    line = re.search(r"\[Ensemble x64\] smoother: CRPS = (\S+) cm at lag 36 rows over 8 rows, fewest paths (\d+)\n", logs["ens"])
    assert line and int(line.group(2)) == ens["smooth_unique_paths"].min()
    assert abs(float(line.group(1)) - ens["smooth_crps_cm"].mean()) < 1e-3


def test_a_smoothed_sweep_on_two_ranks_writes_what_one_rank_writes(tmp_path):
    params = _cli_params(tmp_path)
    params["Ensemble"] = {"Members": 40, "Seed": 5, "Days": 2,
                          "Points": [{"Soil_Properties": {"n": n}} for n in (1.6, 2.4)],
                          "Filter": {"Stride": 24, "Sigma_cm": 8.0, "Smoother": {"Stride": 12, "Lag_rows": 24}}}
    one, log1 = _run_ranks(tmp_path, "one", params, 1)
    two, log2 = _run_ranks(tmp_path, "two", params, 2)
    assert set(one) == set(two) and SMOOTH_KEYS <= set(one)
    for k in sorted(set(one) - {"gpus"}):
        assert _same(one[k], two[k]), k
    assert one["smooth_hist"].shape == (2, 8, 200) and one["smooth_lag_rows"].shape == (2, 8)
    line = [s for s in log1.splitlines() if "smoother:" in s]
    assert len(line) == 1 and line == [s for s in log2.splitlines() if "smoother:" in s]
    assert "[Sweep 2 points x40] smoother: CRPS = " in line[0] and "at lag 24 rows over 8 rows" in line[0]


def test_cli_refuses_a_smoother_with_a_sharded_single_point_filter(tmp_path, monkeypatch, capsys):
    from hydromodel_amd import cli
    params = _cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    params["Ensemble"] = {"Members": 64, "Days": 1, "Filter": {"Sigma_cm": 10.0, "Sharded": True, "Smoother": {"Stride": 12}}}
    (tmp_path / "p.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as status:
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "p.json")])
    out = capsys.readouterr().out
    assert status.value.code == 1 and "Filter.Smoother is not available with \"Sharded\": true" in out
    assert not (tmp_path / "Sim_01_ensemble.h5").exists() and "Saving" not in out
