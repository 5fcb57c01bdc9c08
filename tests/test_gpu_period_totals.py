"""Period totals per member reduced on the GPU (include/hydrocol.h hc_set_period_totals): the accumulators, the moments
table and both histograms against the NumPy restatement fed with the diag / wtd a twin handle WITHOUT the feature returns
(integers: no tolerance), no side effects on the run, independence of launch length, member split, parameter points and
handles, resume in the middle of a period, skipped rows, the particle filter's ancestry, the EnKF, the refusals and the
CLI's "Ensemble": {"Periods": ...} block.  Every case sets the period totals, so none can pass without them."""
import copy
import json
from functools import lru_cache

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the refusal test makes a sharded filter, whose buffer is torch's)

from helpers import cli_params, digest, digest_point, golden, run_cli_ranks

pytestmark = pytest.mark.gpu

ROWS = 96                                # two days
# a period that ends inside a launch's natural length, one that ends on a refresh row, a one-row period and one that
# spans the day boundary
ENDS = [5, 48, 49, 96]


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@lru_cache(maxsize=None)
def _psi(well, N):
    """[N][D]: the initial profile raised by a per-member offset, uniform over 10 .. 50 cm: water tables in many cells, all
    of them above the well's (index 60 on these rows) -- the lateral flow is zero for a member whose water table stands
    below the observed one (richards_pde.py:352-376), and every member's total must be > 0."""
    ic = np.asarray(golden(f"g1_tables_{well}.npz")["initial_cond"])
    psi = ic[None, :] + np.random.default_rng(12).uniform(10.0, 50.0, size=N)[:, None]
    psi.setflags(write=False)
    return psi


def _handle(well, N, forcing=None, points=None, psi=None, seed=7, offset=0, bases=None, rpl=0):
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, f0 = digest(well)
    st = EnsembleStepper(points or cols, f0 if forcing is None else forcing, N)
    st.set_state(_psi(well, N) if psi is None else psi)
    st.set_noise_philox(seed, offset)
    if bases is not None:
        st.set_point_member_bases(np.asarray(bases))
    if rpl:
        st.set_rows_per_launch(rpl)
    return st


@lru_cache(maxsize=None)
def _twin(well, N, skipped=()):
    """Two days of a handle without the feature: (diag [96][N][2], wtd [96][N], state, moments, counters, forcing)."""
    forcing = _forcing(well, skipped)
    st = _handle(well, N, forcing)
    try:
        out = st.step_rows(1, ROWS, want_diag=True, want_wtd=True)
        return out["diag"], out["wtd"], st.get_state(), st.moments(), st.counters(), forcing
    finally:
        st.close()


@lru_cache(maxsize=None)
def _forcing(well, skipped=()):
    """The well's forcing, with the rows `skipped` unobserved (wtd_obs = -1, set before any handle is made)."""
    forcing = digest(well)[2]
    if skipped:
        forcing = copy.copy(forcing)
        forcing.wtd_obs = np.array(forcing.wtd_obs)
        forcing.wtd_obs[list(skipped)] = -1
        forcing.refresh = np.array(forcing.refresh)
        forcing.refresh[list(skipped)] = 0                           # a skipped row draws nothing (as the digest has it)
    return forcing


def _setup(diag, wtd):
    """Threshold nodes the members' water tables straddle and the flux exponents, from the twin's output alone: the
    smallest power of two above the largest total any member has over any run of rows within a day (the periods of
    ENDS lie within a day)."""
    thr = [int(np.quantile(wtd, 0.25)), int(np.quantile(wtd, 0.6))]
    for t in thr:
        assert (wtd <= t).any() and (wtd > t).any()
    total = diag.sum(axis=0)                                        # [N][2]
    assert np.all(total > 0) and len(set(total[:, 1].tolist())) > 1  # every flux total > 0, lateral flow not all equal
    run = [np.concatenate([np.zeros((1,) + d.shape[1:]), np.cumsum(d, axis=0)]) for d in (diag[:48], diag[48:])]
    day = np.maximum(*[(c - np.minimum.accumulate(c, axis=0)).max(axis=0) for c in run])        # [N][2]
    fexp = [int(np.floor(np.log2(day[:, q].max()))) + 1 for q in range(2)]
    assert all(-8 <= e <= 12 for e in fexp)
    return thr, fexp


def _tables(st):
    hf, hw = st.period_totals_hists() if st.period_bins else (None, None)
    return st.period_totals_table(), hf, hw


# ---- 1. exactness, period by period; no side effects ------------------------------------------------------------------
@pytest.mark.parametrize("well, N, B", [(200, 67, 32), (200, 67, 1024), (300, 3, 32)])
def test_every_period_equals_the_restatement_of_the_twins_rows(well, N, B):
    from hydromodel_amd.stepper import period_totals_of, split_period_totals_table
    diag, wtd, psi_twin, mom_twin, cnt_twin, forcing = _twin(well, N)
    thr, fexp = _setup(diag, wtd)
    D = digest(well)[1].dim_d
    st = _handle(well, N)
    try:
        st.set_period_totals(ENDS, thr, B, fexp)
        ends, got_thr, got_b, got_f = st.period_totals_layout()
        assert ends.tolist() == ENDS and got_thr.tolist() == thr and got_b == B and got_f == tuple(fexp)
        # the stops: after every end row, and in the middle of two periods
        done = 0
        for upto in (3, 5, 30, 48, 49, 70, 96):
            st.step_rows(done + 1, upto - done)
            done = upto
            want = period_totals_of(diag[:upto], wtd[:upto], forcing.wtd_obs, ENDS, thr, B, fexp, D=D)
            table, hf, hw = _tables(st)
            assert _same(table, want["table"]), upto
            assert _same(hf[0], want["hist_flux"]) and _same(hw[0], want["hist_wtd"]), upto
            assert _same(st.period_totals_acc(), want["acc"]), upto
            assert want["overflow"] == 0 and want["outside"] == 0
            assert st.period_totals_overflow() == 0 and st.period_totals_outside() == 0
        parts = split_period_totals_table(table, 1, len(ENDS), 6)
        assert np.all(parts["pcnt"] == N) and np.all(hf.sum(axis=-1) == N) and np.all(hw.sum(axis=-1) == N)
        occupied = (want["hist_flux"][:, 1] > 0).sum(axis=-1)
        print(f"well {well} N {N} B {B}: thresholds {thr}, exponents {fexp}, occupied lateral-flow bins {occupied.tolist()}")
        assert N < 4 or occupied.max() > 1                          # more than one lateral-flow bin is occupied
        # the accumulators of each period as they stood at its end: the restatement's, by the members' own rows
        assert np.array_equal(want["acc_at_end"][3, 2], wtd[49:96].min(axis=0))
        assert np.array_equal(want["acc_at_end"][3, 3], wtd[49:96].max(axis=0))
        assert np.array_equal(want["acc_at_end"][1, 4], (wtd[5:48] <= thr[0]).sum(axis=0))
        # the run itself is the twin's, to the bit
        assert _same(st.get_state(), psi_twin) and np.array_equal(st.moments(), mom_twin) and st.counters() == cnt_twin
    finally:
        st.close()


def test_the_profile_table_and_the_outputs_are_those_of_a_run_without_the_feature():
    res = []
    for on in (False, True):
        st = _handle(200, 67)
        try:
            st.set_profile_stats(24)
            if on:
                st.set_period_totals(ENDS, [60], 32, [0, 0])
            st.profile_snapshot(0)
            out = st.step_rows(1, ROWS, want_wtd=True, want_diag=True)
            res.append((st.get_state(), out["wtd"], out["diag"], st.moments(), st.counters(), st.profile_table()))
        finally:
            st.close()
    a, b = res
    assert all(_same(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))
    assert _same(a[2], _twin(200, 67)[0])                            # ... and the diag of a run without the profiles


# ---- 2. independence of the run's shape --------------------------------------------------------------------------------
def _run(N, well=200, B=128, wider=0, **kw):
    diag, wtd = _twin(200, 67)[:2]
    thr, fexp = _setup(diag, wtd)
    fexp = [e + wider for e in fexp]                                 # (another parameter point: room for its fluxes)
    st = _handle(well, N, **kw)
    try:
        st.set_period_totals(ENDS, thr, B, fexp)
        st.step_rows(1, ROWS)
        assert st.period_totals_overflow() == 0 and st.period_totals_outside() == 0
        return _tables(st)
    finally:
        st.close()


@lru_cache(maxsize=None)
def _whole_67():
    return _run(67)


def test_the_tables_do_not_depend_on_the_launch_length():
    assert all(_same(g, w) for g, w in zip(_run(67, rpl=7), _whole_67()))


def test_one_handle_equals_two_handles_summed():
    psi = _psi(200, 67)
    a = _run(30, rpl=5, offset=0, psi=psi[:30])
    b = _run(37, rpl=11, offset=30, psi=psi[30:])
    assert all(_same(x + y, w) for x, y, w in zip(a, b, _whole_67()))


def test_two_parameter_points_one_handle_equals_two_handles():
    from hydromodel_amd.stepper import split_period_totals_table
    pts = [digest(200)[1], digest_point("a003")[1]]
    psi = _psi(200, 67)
    table, hf, hw = _run(134, B=64, wider=2, points=pts, bases=[0, 5000], psi=np.concatenate([psi, psi]))
    parts = split_period_totals_table(table, 2, len(ENDS), 6)
    assert np.all(parts["pcnt"] == 67) and not _same(parts["pmom"][0], parts["pmom"][1])       # the points differ
    for k, (pt, offset) in enumerate(zip(pts, (0, 5000))):
        t1, hf1, hw1 = _run(67, B=64, wider=2, points=pt, offset=offset, psi=psi)
        one = split_period_totals_table(t1, 1, len(ENDS), 6)
        assert _same(one["pmom"][0], parts["pmom"][k]) and _same(one["pcnt"][0], parts["pcnt"][k])
        assert _same(hf1[0], hf[k]) and _same(hw1[0], hw[k])


# ---- 3. skipped rows ---------------------------------------------------------------------------------------------------
def test_a_skipped_row_adds_nothing_and_a_period_of_skipped_rows_counts_nobody():
    from hydromodel_amd.stepper import period_solved_rows, period_totals_of, split_period_totals_table
    diag, wtd, _, _, _, forcing = _twin(200, 67, skipped=(20, 49))
    assert forcing.wtd_obs[20] == -1 and forcing.wtd_obs[49] == -1 and digest(200)[2].wtd_obs[49] >= 0
    thr, fexp = _setup(*_twin(200, 67)[:2])
    st = _handle(200, 67, forcing)
    try:
        st.set_period_totals(ENDS, thr, 32, fexp)
        st.step_rows(1, ROWS)
        want = period_totals_of(diag, wtd, forcing.wtd_obs, ENDS, thr, 32, fexp, D=200)
        table, hf, hw = _tables(st)
        assert _same(table, want["table"]) and _same(hf[0], want["hist_flux"]) and _same(hw[0], want["hist_wtd"])
        parts = split_period_totals_table(table, 1, len(ENDS), 6)
        assert parts["pcnt"][0].tolist() == [67, 67, 0, 67]          # the one-row period counts nobody
        assert not parts["pmom"][0, 2].any() and not hf[0, 2].any() and not hw[0, 2].any()
        assert period_solved_rows(forcing.wtd_obs, ENDS).tolist() == [5, 42, 0, 47]
        assert period_solved_rows(digest(200)[2].wtd_obs, ENDS).tolist() == [5, 43, 1, 47]
        assert st.period_totals_overflow() == 0 and st.period_totals_outside() == 0
    finally:
        st.close()


# ---- 4. the filters ----------------------------------------------------------------------------------------------------
def test_the_particle_filters_resampling_carries_the_accumulators_to_the_slots():
    from hydromodel_amd.stepper import period_totals_of
    ends = [72, 96]

    def run(feature):
        st = _handle(200, 67)
        try:
            st.set_filter(48, 8.0, seed=11)
            if feature:
                st.set_period_totals(ends, feature[0], 32, feature[1])
            a = st.step_rows(1, 48, want_diag=True, want_wtd=True)
            anc = st.filter_ancestors()
            b = st.step_rows(49, 48, want_diag=True, want_wtd=True)
            diag, wtd = np.concatenate([a["diag"], b["diag"]]), np.concatenate([a["wtd"], b["wtd"]])
            return diag, wtd, anc, st.get_state(), (_tables(st) if feature else None), \
                (st.period_totals_overflow(), st.period_totals_outside()) if feature else None
        finally:
            st.close()

    diag, wtd, anc, psi, _, _ = run(None)
    thr, fexp = _setup(diag, wtd)
    fexp = [e + 1 for e in fexp]             # a slot's path total joins two members' rows: room above the slots' own totals
    assert len(set(anc.tolist())) < 67 and not np.array_equal(anc, np.arange(67))     # members were dropped and copied
    assert len({tuple(r) for r in diag[:48].sum(axis=0).tolist()}) > 1                # and differed before the resampling
    got_diag, got_wtd, got_anc, got_psi, (table, hf, hw), counts = run((thr, fexp))
    assert _same(got_diag, diag) and _same(got_wtd, wtd) and _same(got_anc, anc) and _same(got_psi, psi)
    forcing = digest(200)[2]
    want = period_totals_of(diag, wtd, forcing.wtd_obs, ends, thr, 32, fexp, ancestors={48: anc}, D=200)
    assert _same(table, want["table"]) and _same(hf[0], want["hist_flux"]) and _same(hw[0], want["hist_wtd"])
    assert counts == (0, 0) and want["overflow"] == 0 and want["outside"] == 0
    plain = period_totals_of(diag, wtd, forcing.wtd_obs, ends, thr, 32, fexp, D=200)
    assert not _same(plain["table"], want["table"])                  # the ancestry matters to the tables


def test_enkf_members_persist_and_the_tables_are_the_forecasts():
    from hydromodel_amd.stepper import period_totals_of
    ends = [48, 72, 96]                                              # the first period ends on the analysis row
    thr, fexp = _setup(*_twin(200, 67)[:2])
    st = _handle(200, 67)
    try:
        st.set_enkf(48, 8.0, seed=11)
        st.set_period_totals(ends, thr, 32, fexp)
        out = st.step_rows(1, ROWS, want_diag=True, want_wtd=True)
        want = period_totals_of(out["diag"], out["wtd"], digest(200)[2].wtd_obs, ends, thr, 32, fexp, D=200)
        table, hf, hw = _tables(st)
        assert _same(table, want["table"]) and _same(hf[0], want["hist_flux"]) and _same(hw[0], want["hist_wtd"])
        assert _same(st.period_totals_acc(), want["acc"])
        assert st.period_totals_overflow() == 0 and st.period_totals_outside() == want["outside"]
    finally:
        st.close()


def test_refusals():
    from hydromodel_amd._lib import HcError
    st = _handle(300, 4)
    T = digest(300)[2].dim_t
    try:
        def off():
            return st.period_totals_layout()[0].size == 0 and st.period_ends.size == 0 and st.period_bins == 0

        for bad in ([5, 5], [7, 3], [0, 4], [4, T], [-1]):
            with pytest.raises(HcError, match=r"ascending rows in \[1, "):
                st.set_period_totals(bad)
            assert off()
        with pytest.raises(HcError, match=r"4097 periods \(1 to 4096"):
            st.set_period_totals(np.arange(1, 4098))
        with pytest.raises(HcError, match="5 thresholds"):
            st.set_period_totals([48], [1, 2, 3, 4, 5])
        for node in (-1, 300):
            with pytest.raises(HcError, match="outside the column's 300 nodes"):
                st.set_period_totals([48], [10, node])
            assert off()
        for bins in (48, 16, 2048, -32):
            with pytest.raises(HcError, match="a power of two in 32 .. 1024"):
                st.set_period_totals([48], [], bins)
        for e in (-9, 13):
            with pytest.raises(HcError, match=r"-8 \.\. 12"):
                st.set_period_totals([48], [], 32, [0, e])
        assert off()
        st.set_period_totals([48], [10], 0)                        # moments alone
        assert st.period_totals_words() == 5 * 5 + 1 + 1
        with pytest.raises(HcError, match="no histograms"):
            st.period_totals_hist_raw()
        acc = st.period_totals_acc()
        assert acc.shape == (5, 4) and acc[2].tolist() == [65535] * 4 and not acc[[0, 1, 3, 4]].any()
        # the accumulators and the tables travel (checkpoints)
        st.set_period_totals_acc(np.arange(20))
        assert st.period_totals_acc().reshape(-1).tolist() == list(range(20))
        t = np.arange(27, dtype=np.int64)
        st.set_period_totals_table(t)
        assert _same(st.period_totals_table(), t) and st.period_totals_overflow() == 26
        st.reset_period_totals()
        assert not st.period_totals_table().any() and _same(st.period_totals_acc(), acc)
        # a sharded particle filter routes columns, not accumulators: refused either way round
        st.set_filter(48, 8.0, seed=1)
        with pytest.raises(HcError, match="period totals are set"):
            st.set_filter_shard([0, 4], 0)
        st.set_period_totals([])
        assert off()
        with pytest.raises(HcError, match="are off"):
            st.period_totals_table()
        st.set_filter_shard([0, 4], 0)
        with pytest.raises(HcError, match="sharded particle filter"):
            st.set_period_totals([48])
        assert off()
    finally:
        st.close()


# ---- 5. resume ---------------------------------------------------------------------------------------------------------
def test_resume_in_the_middle_of_a_period_gives_the_uninterrupted_tables(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(200)
    thr, fexp = _setup(*_twin(200, 67)[:2])
    kw = dict(seed=7, psi0=_psi(200, 67),       # (the twin's members and streams)
              period_ends=ENDS, period_thresholds_cm=[float(cols.z[t]) for t in thr],
              period_bins=64, period_flux_max_cm=[2.0 ** e for e in fexp])
    full = EnsembleSimulation(cols, forcing, 67, **kw)
    full.advance(ROWS)
    want, (want_hf, want_hw) = full.period_table(), full.period_hists()
    assert full.stepper.period_threshold_nodes.tolist() == thr
    assert full.stepper.period_totals_outside() == 0 and full.stepper.period_totals_overflow() == 0
    full.close()
    first = EnsembleSimulation(cols, forcing, 67, **kw)
    first.advance(30)                                                # period 1 is (5, 48]: its accumulators are half full
    acc = first.stepper.period_totals_acc()
    assert acc[0].any() and acc[1].any() and (acc[2] != 65535).all()
    path = first.dump(tmp_path / "ckpt.h5")
    first.close()
    resumed = EnsembleSimulation.restore(path, cols, forcing)
    assert _same(resumed.stepper.period_totals_acc(), acc)
    resumed.advance(ROWS - 30)
    got, (got_hf, got_hw) = resumed.period_table(), resumed.period_hists()
    stats, dist = resumed.period_stats(), resumed.period_distribution([0.05, 0.5, 0.95])
    resumed.close()
    assert resumed.period_bins == 64 and resumed.period_ends.tolist() == ENDS
    assert _same(got, want) and _same(got_hf, want_hf) and _same(got_hw, want_hw)
    assert want_hf.shape == (4, 2, 64) and want_hw.shape == (4, 2, 200) and np.all(want_hf.sum(axis=-1) == 67)
    assert stats["count"].tolist() == [67] * 4 and stats["solved_rows"].tolist() == [5, 43, 1, 47]
    assert np.all(stats["transpiration_mean_cm"][[1, 3]] > 0) and np.all(stats["lateral_flow_std_cm"] >= 0)
    assert np.all(stats["transpiration_mean_cm"][[0, 2]] == 0)       # rows 1 .. 5 and row 49 are night rows
    assert np.all(stats["wtd_shallowest_mean_cm"] <= stats["wtd_deepest_mean_cm"])
    assert np.all(stats["wtd_shallowest_mean_cm"][2] == stats["wtd_deepest_mean_cm"][2])      # the one-row period
    assert np.all((stats["below_fraction_mean"] >= 0) & (stats["below_fraction_mean"] <= 1))
    assert np.all(stats["below_fraction_mean"][:, 0] <= stats["below_fraction_mean"][:, 1])   # the deeper threshold holds more
    q = dist["lateral_flow_quantile_cm"]
    assert q.shape == (4, 3) and np.all(q[:, 0] <= q[:, 2])
    width = 2.0 ** fexp[1] / 64                                      # the mean lies within the outer quantiles' bins
    assert np.all(stats["lateral_flow_mean_cm"] >= q[:, 0] - width - 3 * stats["lateral_flow_std_cm"])
    assert np.all(stats["lateral_flow_mean_cm"] <= q[:, 2] + width + 3 * stats["lateral_flow_std_cm"])


def test_the_simulation_refuses_a_sharded_particle_filter():
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(200)
    with pytest.raises(ValueError, match="period_ends and filter_shard exclude each other"):
        EnsembleSimulation(cols, forcing, 8, psi0=_psi(200, 8), period_ends=[48], filter_stride=48, filter_sigma_cm=8.0,
                           filter_shard=([0, 8], 0, None))


# ---- 6. the CLI --------------------------------------------------------------------------------------------------------
NAMES = ("transpiration", "lateral_flow", "wtd_shallowest", "wtd_deepest")
PERIOD_KEYS = {"period_end_rows", "period_solved_rows", "period_count", "period_thresholds_cm", "period_threshold_nodes",
               "period_overflow", "period_below_rows_mean", "period_below_rows_std", "period_below_fraction_mean"} | \
    {f"period_{n}_{w}_cm" for n in NAMES for w in ("mean", "std")}
PERIOD_HIST_KEYS = {"period_hist_flux", "period_hist_wtd", "period_hist_bins", "period_hist_flux_max_cm", "period_hist_outside",
                    "period_quantile_levels"} | {f"period_{n}_quantile_cm" for n in NAMES}
BLOCK = {"Rows": 36, "Shallower_than_cm": [100, 400], "Bins": 64, "Transpiration_max_cm": 4, "Lateral_flow_max_cm": 1,
         "Quantiles": [0.05, 0.5, 0.95]}


@pytest.mark.parametrize("n_points", [0, 2])
def test_cli_block_writes_the_datasets_and_leaves_the_rest_alone(tmp_path, monkeypatch, capsys, n_points):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    from hydromodel_amd.stepper import period_totals_distribution
    params = cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    pts = {"Points": [{"Soil_Properties": {"n": n}} for n in (1.6, 2.4)][:n_points]} if n_points else {}
    blocks = (("plain", {}), ("moments", {"Periods": {k: BLOCK[k] for k in ("Rows", "Shallower_than_cm")}}),
              ("periods", {"Periods": BLOCK}))
    files = {}
    for tag, extra in blocks:
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 128, "Seed": 3, "Days": 2, "Profiles": 48, **pts, **extra}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        capsys.readouterr()
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = (loadResults(tmp_path / f"Run_{tag}_ensemble.h5"), capsys.readouterr().out)
    (plain, log_plain), (mom, log_mom), (per, log_per) = files["plain"], files["moments"], files["periods"]
    lead = (n_points,) if n_points else ()
    assert not [k for k in plain if k.startswith("period_")] and "periods" not in log_plain
    assert set(mom) - set(plain) == PERIOD_KEYS and set(per) - set(plain) == PERIOD_KEYS | PERIOD_HIST_KEYS
    assert per["period_end_rows"].tolist() == [36, 72] and per["period_solved_rows"].tolist() == [36, 36]
    assert per["period_count"].shape == lead + (2,) and np.all(per["period_count"] == 128)
    assert per["period_thresholds_cm"].tolist() == [100, 400] and per["period_threshold_nodes"].shape == (2,)
    z = digest(200)[1].z
    assert np.array_equal(z[per["period_threshold_nodes"]], [z[z >= 100][0], z[z >= 400][0]])
    for n in NAMES:
        assert per[f"period_{n}_mean_cm"].shape == lead + (2,) and per[f"period_{n}_std_cm"].shape == lead + (2,)
        assert per[f"period_{n}_quantile_cm"].shape == lead + (2, 3)
    assert per["period_below_rows_mean"].shape == lead + (2, 2) and per["period_below_fraction_mean"].shape == lead + (2, 2)
    assert per["period_hist_flux"].shape == lead + (2, 2, 64) and per["period_hist_flux"].dtype == np.int32
    assert per["period_hist_wtd"].shape == lead + (2, 2, 200) and np.all(per["period_hist_wtd"].sum(axis=-1) == 128)
    assert int(per["period_hist_bins"]) == 64 and per["period_hist_flux_max_cm"].tolist() == [4, 1]
    assert int(per["period_hist_outside"]) == 0 and int(per["period_overflow"]) == 0
    assert np.all(per["period_hist_flux"].sum(axis=-1) == 128) and per["period_quantile_levels"].tolist() == [0.05, 0.5, 0.95]
    # the mean of the members' totals is the total of the rows' means (which the file already held), to the 2^-20 cm of
    # the floor; the sigma is not the root of the summed squares: the rows of a member are correlated
    for p, rows in enumerate((slice(1, 37), slice(37, 73))):
        for n in NAMES[:2]:
            total = per[f"{n}_mean"][..., rows].sum(axis=-1)
            assert np.all(total > 0 if n == "transpiration" else total >= 0) and np.allclose(per[f"period_{n}_mean_cm"][..., p], total, rtol=0, atol=2.0 ** -19)
    d = period_totals_distribution(per["period_hist_flux"], per["period_hist_wtd"], [0.05, 0.5, 0.95], (2, 0), float(z[0]), digest(200)[1].dz)
    for n in NAMES:
        assert _same(d[f"{n}_quantile_cm"], per[f"period_{n}_quantile_cm"]), n
    assert np.all(per["period_wtd_shallowest_mean_cm"] <= per["period_wtd_deepest_mean_cm"])
    for k in PERIOD_KEYS:                                    # the moments do not depend on the histograms
        assert _same(mom[k], per[k]), k
    for k in plain:                                          # every other dataset, byte for byte
        assert _same(plain[k], per[k]) and _same(plain[k], mom[k]), k
    who = "Sweep 2 points x128" if n_points else "Ensemble x128"
    line = f" [{who}] periods: 2 periods, 6 quantities\n"
    assert line in log_per and line in log_mom


@pytest.mark.parametrize("sweep", [False, True])
def test_two_ranks_sharing_the_card_write_what_one_rank_writes(tmp_path, sweep):
    params = cli_params(tmp_path)
    ens = {"Members": 250, "Seed": 5, "Days": 2, "Periods": BLOCK}
    if sweep:                                                # three points dealt to two ranks: 2 + 1
        ens.update(Members=32, Points=[{"Soil_Properties": {"n": n}} for n in (1.6, 2.0, 2.4)])
    params["Ensemble"] = ens
    one, log1 = run_cli_ranks(tmp_path, "one", params, 1)
    two, log2 = run_cli_ranks(tmp_path, "two", params, 2)
    assert PERIOD_KEYS | PERIOD_HIST_KEYS <= set(one) and set(one) == set(two)
    assert int(one["gpus"]) == 1 and int(two["gpus"]) == 2 and int(one["period_hist_outside"]) == 0
    members = 32 if sweep else 250
    assert np.all(one["period_count"] == members) and np.all(one["period_hist_flux"].sum(axis=-1) == members)
    for k in one:
        if k != "gpus":
            assert _same(one[k], two[k]), k
    line = [s for s in log1.splitlines() if "periods:" in s]
    assert len(line) == 1 and line == [s for s in log2.splitlines() if "periods:" in s]


def test_with_a_sharded_enkf_two_ranks_write_what_one_rank_writes(tmp_path):
    """Members persist through an analysis, so every rank reduces its own share of the one point and the shares are summed."""
    params = cli_params(tmp_path)
    params["Ensemble"] = {"Members": 512, "Seed": 5, "Days": 2, "EnKF": {"Stride": 24, "Sigma_cm": 8.0, "Sharded": True},
                          "Periods": dict(BLOCK, Rows=24)}
    one, log1 = run_cli_ranks(tmp_path, "one", params, 1)
    two, log2 = run_cli_ranks(tmp_path, "two", params, 2)
    assert PERIOD_KEYS | PERIOD_HIST_KEYS <= set(one) and set(one) == set(two) and "enkf_sharded" in one
    assert int(one["gpus"]) == 1 and int(two["gpus"]) == 2
    assert one["period_end_rows"].tolist() == [24, 48, 72, 96] and np.all(one["period_count"] == 512)
    for k in one:
        if k != "gpus":
            assert _same(one[k], two[k]), k
    assert " [Ensemble x512] periods: 4 periods, 6 quantities" in log1.splitlines()
    assert " [Ensemble x512] periods: 4 periods, 6 quantities" in log2.splitlines()
