"""Root-water uptake by depth on the GPU (include/hydrocol.h hc_set_root_uptake): the hook's theta against the stateless
plugin call and its u against the NumPy restatement (no tolerance) and against the oracle's and hc_rhs_ex's sink (the
tolerance test_rhs_matches_oracle holds `s` to); the accumulators, moments, share histograms and depth profile against the
restatement fed with the hook's u of a twin handle's rows (integers: no tolerance); no side effects on the run;
independence of launch length, member split, parameter points and handles; a checkpoint in the middle of a period;
skipped rows; the filters; the refusals.  Every case calls the new API, so none can pass without it."""
import copy
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the refusal test makes a sharded filter, whose buffer is torch's)

import rhs_states as bank
from helpers import digest, digest_point, golden, rel_err

pytestmark = pytest.mark.gpu

ROWS = 96                                # two days
ENDS = [5, 48, 49, 96]                   # as the period totals' tests: a night period, a day, a one-row period, a day


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _cells(D):
    """The top six cells, every cell, the last cell (below the roots: all zero) and two layers that overlap."""
    M = D - 1
    return [(0, 6), (0, M), (M - 1, M), (2, 30), (20, 60)]


@lru_cache(maxsize=None)
def _psi(well, N):
    """[N][D]: the initial profile raised by a per-member offset, uniform over 10 .. 50 cm (the period totals' members)."""
    ic = np.asarray(golden(f"g1_tables_{well}.npz")["initial_cond"])
    psi = ic[None, :] + np.random.default_rng(12).uniform(10.0, 50.0, size=N)[:, None]
    psi.setflags(write=False)
    return psi


@lru_cache(maxsize=None)
def _forcing(well, skipped=()):
    forcing = digest(well)[2]
    if skipped:
        forcing = copy.copy(forcing)
        forcing.wtd_obs = np.array(forcing.wtd_obs)
        forcing.wtd_obs[list(skipped)] = -1
        forcing.refresh = np.array(forcing.refresh)
        forcing.refresh[list(skipped)] = 0                           # a skipped row draws nothing (as the digest has it)
    return forcing


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


def _u_of_rows(st, psi_rows, row_begin=1):
    """[R][N][D - 1]: the hook's u of the staged rows, each on its own forcing row (the handle's state is put back)."""
    keep = st.get_state()
    u = np.zeros(psi_rows.shape[:2] + (st.D - 1,))
    for r in range(psi_rows.shape[0]):
        st.set_state(psi_rows[r])
        u[r] = st.root_uptake_eval(row_begin + r)[1]
    st.set_state(keep)
    return u


@lru_cache(maxsize=None)
def _twin(well, N, skipped=()):
    """Two days of a handle without the feature: (u [96][N][D - 1] of its rows' end states, state, moments, counters,
    forcing, the profile table at stride 24, the period totals' table)."""
    forcing = _forcing(well, skipped)
    st = _handle(well, N, forcing)
    try:
        st.set_profile_stats(24)
        st.set_period_totals(ENDS, [60], 32, [2, 2])
        st.profile_snapshot(0)
        out = st.step_rows(1, ROWS, want_psi=True)
        res = (st.get_state(), st.moments(), st.counters(), forcing, st.profile_table(), st.period_totals_table(),
               st.period_totals_hist_raw())
        return (_u_of_rows(st, out["psi"]),) + res
    finally:
        st.close()


def _tables(st):
    return st.root_uptake_table(), (st.root_uptake_hist() if st.uptake_bins else None)


# ---- 1. the hook ---------------------------------------------------------------------------------------------------------
def _plugin_theta(st, cols, psi):
    """theta [N][D - 1] of the stateless plugin call on the midpoints of psi [N][D], with the midpoint tables."""
    from hydromodel_amd import _lib as L
    ym = np.ascontiguousarray((0.5 * (psi[:, :-1] + psi[:, 1:])).T)          # [cells][columns]
    M, N = ym.shape
    out, qinf = np.empty((4, M, N)), np.empty(N)
    zeros = np.zeros(M)
    L.check(st.lib.hc_plugin_eval(0, C.byref(st.params), M, N, L.dptr(ym), L.dptr(L.as_f64(cols.por_mid)),
                                  L.dptr(L.as_f64(cols.meank_mid)), L.dptr(L.as_f64(cols.noisec_mid)), L.dptr(zeros),
                                  L.dptr(out), L.dptr(qinf)))
    return np.ascontiguousarray(out[0].T)


@pytest.mark.parametrize("D, crafted, flags", [(200, False, "no_lf"), (300, False, "no_lf"), (300, True, "default"),
                                               (200, False, "no_et")])
def test_the_hook_equals_the_restatement_the_plugin_and_the_oracles_sink(D, crafted, flags):
    from hydromodel_amd.stepper import EnsembleStepper, root_uptake_mid_tables, root_uptake_of
    from oracle.oracle import Oracle
    cols, forcing, rows = bank.case_column(D, crafted=crafted)
    names, Y, Z = bank.case_bank(cols)
    fl = bank.FLAG_SETS[flags]
    st = EnsembleStepper(cols, forcing, len(Y), flags=fl)
    try:
        st.set_state(Y)
        st.set_noise_host(Z)
        tabs = root_uptake_mid_tables(cols)
        assert _same(st.root_uptake_tables(), tabs)
        o = Oracle(cols, forcing.surface_evap, flags=fl)
        want_theta = _plugin_theta(st, cols, Y)
        active = 0
        for name, row, spin in rows:
            if spin:
                continue
            th, u = st.root_uptake_eval(row)
            assert _same(th, want_theta), name                           # the cell model's theta, bit for bit
            want = root_uptake_of(th, tabs, forcing.atm[row], forcing.daylight[row], cols.n_root_first, cols.n_root_int,
                                  cols.dz, flag_et=flags != "no_et")
            assert _same(u, want), name                                  # the documented order, bit for bit
            assert np.all(u >= 0.0) and not u[:, cols.n_root_int + 1:].any()
            if not forcing.daylight[row] or flags == "no_et":
                assert not u.any(), name
            active += int(u.any())
            if flags != "no_lf":
                continue                                                 # (with lateral flow on, s holds its sink too)
            aux = st.rhs(row, want_aux=True)[1]
            assert rel_err(u, -aux["s"], 1e-3) < 1e-11, name
            for k in range(len(Y)):
                ra = o.rhs(bank.oracle_row(forcing, row, False), Y[k], Z[k], want_aux=True)[1]
                assert rel_err(u[k], -ra["s"], 1e-3) < 1e-11, (name, names[k])
        assert active == (0 if flags == "no_et" else 3)                  # day_dry, day_demand and wet take up water
        assert st.uptake_cells.shape == (0, 2)                           # the hook needs no hc_set_root_uptake
    finally:
        st.close()


# ---- 2. the tables, period by period; no side effects -------------------------------------------------------------------
@pytest.mark.parametrize("well, N, B", [(200, 67, 32), (200, 67, 1024), (300, 3, 32)])
def test_every_period_equals_the_restatement_of_the_twins_rows(well, N, B):
    from hydromodel_amd.stepper import root_uptake_tables_of, split_root_uptake_table
    u, psi_twin, mom_twin, cnt_twin, forcing, prof_twin, per_twin, perh_twin = _twin(well, N)
    cols = digest(well)[1]
    D, cells = cols.dim_d, _cells(cols.dim_d)
    st = _handle(well, N)
    try:
        st.set_profile_stats(24)
        st.set_period_totals(ENDS, [60], 32, [2, 2])
        st.set_root_uptake(cells, B)
        got_cells, got_b = st.root_uptake_layout()
        assert got_cells.tolist() == [list(c) for c in cells] and got_b == B
        assert st.root_uptake_words() == 4 * (6 * 5 + 1 + 2 * (D - 1)) + 1
        st.profile_snapshot(0)
        done = 0
        for upto in (3, 5, 30, 48, 49, 70, 96):
            st.step_rows(done + 1, upto - done)
            done = upto
            want = root_uptake_tables_of(u[:upto], forcing.wtd_obs, ENDS, cells, cols.n_root_int, cols.dz, bins=B,
                                         daylight=forcing.daylight)
            table, hist = _tables(st)
            assert _same(table, want["table"]), upto
            assert _same(hist[0], want["hist"]), upto
            assert _same(st.root_uptake_acc(), want["acc"]), upto
            assert st.root_uptake_overflow() == want["overflow"] == 0 and st.root_uptake_outside() == want["outside"], upto
        parts = split_root_uptake_table(table, 1, len(ENDS), len(cells), D)
        assert np.all(parts["ucnt"] == N)
        # rows 1 .. 5 and row 49 are night rows: those periods' members have no total and no share; the day periods'
        # members all have one
        assert want["outside"] >= 2 * N and not parts["umom"][0, [0, 2]].any() and not parts["uprof"][0, [0, 2]].any()
        full = [p for p in (1, 3) if np.all(want["acc_at_end"][p][0] >> 12 > 0)]
        assert full                                                      # a period in which every member took up water
        for p in full:
            assert np.all(hist[0, p].sum(axis=-1) == N) and hist[0, p, 1, B - 1] == N       # the layer of every cell: share 1
            # the last cell: a sliver of the total; at D = 300 it lies below the roots (n_root_int = 199) and takes nothing
            assert hist[0, p, 2, 0] == N and want["acc_at_end"][p][3].any() == (D - 2 <= cols.n_root_int)
            assert parts["uprof"][0, p, 1:cols.n_root_int + 1].any()
            assert not parts["uprof"][0, p, cols.n_root_int + 1:].any()
        # the run itself is the twin's, to the bit: states, moments, counters, the profile and the period tables
        assert _same(st.get_state(), psi_twin) and np.array_equal(st.moments(), mom_twin) and st.counters() == cnt_twin
        assert _same(st.profile_table(), prof_twin) and _same(st.period_totals_table(), per_twin)
        assert _same(st.period_totals_hist_raw(), perh_twin)
    finally:
        st.close()


def test_the_end_states_uptake_integrates_to_the_reference_transpiration_of_that_state():
    """dz sum_{i >= 1} u_i is the RHS's `transpiration` AT the end state; diag[., 0] is that of the solve's last
    evaluation: the measured difference is printed, not asserted."""
    cols = digest(200)[1]
    st = _handle(200, 67)
    try:
        out = st.step_rows(1, 30, want_diag=True)
        u = st.root_uptake_eval(30)[1]
        tr = st.rhs(30, want_diag=True)[1]["diag"][:, 0]
        mine = cols.dz * u[:, 1:].sum(axis=1)
        assert tr.min() > 0 and rel_err(mine, tr, 1e-6) < 1e-10
        d = np.abs(mine - out["diag"][29, :, 0]) / out["diag"][29, :, 0]
        print(f"row 30, 67 members: |dz sum u - diag| / diag: median {np.median(d):.3e}, max {d.max():.3e}")
    finally:
        st.close()


# ---- 3. independence of the run's shape ------------------------------------------------------------------------------------
def _run(N, well=200, B=128, profiles=0, forcing=None, **kw):
    st = _handle(well, N, forcing, **kw)
    try:
        if profiles:
            st.set_profile_stats(profiles)
        st.set_period_totals(ENDS)
        st.set_root_uptake(_cells(200), B)
        st.step_rows(1, ROWS)
        assert st.root_uptake_overflow() == 0
        return _tables(st) + (st.root_uptake_outside(),)
    finally:
        st.close()


@lru_cache(maxsize=None)
def _whole_67():
    return _run(67)


def _all_same(got, want):
    return all(_same(g, w) if isinstance(w, np.ndarray) else g == w for g, w in zip(got, want))


def test_the_tables_do_not_depend_on_the_launch_length_or_on_the_profiles():
    assert _all_same(_run(67, rpl=7), _whole_67())
    assert _all_same(_run(67, profiles=1), _whole_67()) and _all_same(_run(67, profiles=48, rpl=13), _whole_67())


def test_one_handle_equals_two_handles_summed():
    psi = _psi(200, 67)
    a = _run(30, rpl=5, offset=0, psi=psi[:30])
    b = _run(37, rpl=11, offset=30, psi=psi[30:])
    assert all(_same(x + y, w) if isinstance(w, np.ndarray) else x + y == w for x, y, w in zip(a, b, _whole_67()))


def test_two_parameter_points_one_handle_equals_two_handles():
    from hydromodel_amd.stepper import split_root_uptake_table
    pts = [digest(200)[1], digest_point("a003")[1]]
    psi = _psi(200, 67)
    table, hist, outside = _run(134, B=64, points=pts, bases=[0, 5000], psi=np.concatenate([psi, psi]))
    parts = split_root_uptake_table(table, 2, len(ENDS), 5, 200)
    assert np.all(parts["ucnt"] == 67) and not _same(parts["umom"][0], parts["umom"][1])       # the points differ
    total = 0
    for k, (pt, offset) in enumerate(zip(pts, (0, 5000))):
        t1, h1, o1 = _run(67, B=64, points=pt, offset=offset, psi=psi)
        one = split_root_uptake_table(t1, 1, len(ENDS), 5, 200)
        for name in ("umom", "ucnt", "uprof"):
            assert _same(one[name][0], parts[name][k]), name
        assert _same(h1[0], hist[k])
        total += o1
    assert total == outside


def test_a_skipped_row_adds_nothing_and_a_period_of_skipped_rows_counts_nobody():
    from hydromodel_amd.stepper import root_uptake_tables_of, split_root_uptake_table
    u, *_, forcing, _, _, _ = _twin(200, 67, skipped=(20, 49))
    assert forcing.wtd_obs[20] == -1 and forcing.wtd_obs[49] == -1 and forcing.daylight[20]
    cols = digest(200)[1]
    table, hist, outside = _run(67, B=32, forcing=forcing)
    want = root_uptake_tables_of(u, forcing.wtd_obs, ENDS, _cells(200), cols.n_root_int, cols.dz, bins=32,
                                 daylight=forcing.daylight)
    assert _same(table, want["table"]) and _same(hist[0], want["hist"]) and outside == want["outside"] == 67
    parts = split_root_uptake_table(table, 1, len(ENDS), 5, 200)
    assert parts["ucnt"][0].tolist() == [67, 67, 0, 67]                  # the one-row period counts nobody
    u_with = u.copy()
    u_with[19] = u[18]                                                   # had row 20 counted, the tables would differ
    other = root_uptake_tables_of(u_with, digest(200)[2].wtd_obs, ENDS, _cells(200), cols.n_root_int, cols.dz, bins=32,
                                  daylight=forcing.daylight)
    assert not _same(other["table"], want["table"])


def test_a_checkpoint_in_the_middle_of_a_period_continues_bit_for_bit():
    first = _handle(200, 67)
    try:
        first.set_period_totals(ENDS)
        first.set_root_uptake(_cells(200), 128)
        first.step_rows(1, 30)                                          # period 1 is (5, 48]: the accumulators are half full
        acc, pacc = first.root_uptake_acc(), first.period_totals_acc()
        assert acc[0].all() and acc[1].all() and np.all(acc[1:] <= acc[0])
        saved = (first.get_state(), first.root_uptake_table(), first.root_uptake_hist(), first.root_uptake_outside(),
                 first.period_totals_table())
    finally:
        first.close()
    st = _handle(200, 67, psi=saved[0])
    try:
        st.set_period_totals(ENDS)
        st.set_root_uptake(_cells(200), 128)
        st.set_period_totals_table(saved[4])
        st.set_period_totals_acc(pacc)
        st.set_root_uptake_table(saved[1])
        st.set_root_uptake_hist(saved[2], saved[3])
        st.set_root_uptake_acc(acc)
        assert _same(st.root_uptake_acc(), acc) and st.root_uptake_outside() == saved[3]
        st.step_rows(31, ROWS - 30)
        assert _all_same(_tables(st) + (st.root_uptake_outside(),), _whole_67())
    finally:
        st.close()


# ---- 4. the filters --------------------------------------------------------------------------------------------------------
def test_the_particle_filters_resampling_carries_the_accumulators_to_the_slots():
    from hydromodel_amd.stepper import root_uptake_tables_of
    ends, cols, forcing = [72, 96], digest(200)[1], digest(200)[2]

    def run(feature):
        st = _handle(200, 67)
        try:
            st.set_filter(48, 8.0, seed=11)
            if feature:
                st.set_period_totals(ends)
                st.set_root_uptake(_cells(200), 32)
            a = st.step_rows(1, 48, want_psi=True)
            anc = st.filter_ancestors()
            b = st.step_rows(49, 48, want_psi=True)
            psi_rows = np.concatenate([a["psi"], b["psi"]])
            if feature:
                return psi_rows, anc, st.get_state(), _tables(st), (st.root_uptake_overflow(), st.root_uptake_outside())
            return _u_of_rows(st, psi_rows), psi_rows, anc, st.get_state()
        finally:
            st.close()

    u, psi_rows, anc, psi = run(False)
    assert len(set(anc.tolist())) < 67 and not np.array_equal(anc, np.arange(67))     # members were dropped and copied
    got_rows, got_anc, got_psi, (table, hist), counts = run(True)
    assert _same(got_rows, psi_rows) and _same(got_anc, anc) and _same(got_psi, psi)
    args = (u, forcing.wtd_obs, ends, _cells(200), cols.n_root_int, cols.dz)
    want = root_uptake_tables_of(*args, bins=32, ancestors={48: anc}, daylight=forcing.daylight)
    assert _same(table, want["table"]) and _same(hist[0], want["hist"]) and counts == (0, want["outside"])
    plain = root_uptake_tables_of(*args, bins=32, daylight=forcing.daylight)
    assert not _same(plain["table"], want["table"])                  # the ancestry matters to the tables


def test_enkf_members_persist_and_the_tables_are_the_forecasts():
    from hydromodel_amd.stepper import root_uptake_tables_of
    ends, cols, forcing = [48, 72, 96], digest(200)[1], digest(200)[2]    # the first period ends on the analysis row
    st = _handle(200, 67)
    try:
        st.set_enkf(48, 8.0, seed=11)
        st.set_period_totals(ends)
        st.set_root_uptake(_cells(200), 32)
        out = st.step_rows(1, ROWS, want_psi=True)                       # (the rows' forecasts)
        table, hist = _tables(st)
        acc, outside = st.root_uptake_acc(), st.root_uptake_outside()
        want = root_uptake_tables_of(_u_of_rows(st, out["psi"]), forcing.wtd_obs, ends, _cells(200), cols.n_root_int, cols.dz,
                                     bins=32, daylight=forcing.daylight)
        assert _same(table, want["table"]) and _same(hist[0], want["hist"]) and _same(acc, want["acc"])
        assert outside == want["outside"] and st.root_uptake_overflow() == 0
    finally:
        st.close()


# ---- 5. the refusals -------------------------------------------------------------------------------------------------------
def test_refusals():
    from hydromodel_amd._lib import HcError
    st = _handle(300, 4)
    try:
        def off():
            return st.root_uptake_layout()[0].shape == (0, 2) and st.uptake_cells.shape == (0, 2) and st.uptake_bins == 0

        with pytest.raises(HcError, match="the period totals are off"):
            st.set_root_uptake([(0, 6)])
        assert off()
        with pytest.raises(HcError, match="root uptake is off"):
            st.root_uptake_table()
        st.set_period_totals([48])
        with pytest.raises(HcError, match=r"9 layers \(1 to 8"):
            st.set_root_uptake([(0, 6)] * 9)
        for bad in ((6, 6), (-1, 4), (0, 300), (7, 3)):
            with pytest.raises(HcError, match="not a range of midpoint cells"):
                st.set_root_uptake([(0, 6), bad])
            assert off()
        for bins in (48, 16, 2048, -32):
            with pytest.raises(HcError, match="a power of two in 32 .. 1024"):
                st.set_root_uptake([(0, 6)], bins)
        assert off()
        st.set_root_uptake([(0, 6), (298, 299)])                         # moments alone; a layer below the roots is allowed
        assert st.root_uptake_words() == 3 * 5 + 1 + 2 * 299 + 1
        with pytest.raises(HcError, match="no histogram"):
            st.root_uptake_hist_raw()
        with pytest.raises(HcError, match="the table has 615 words, not 5"):
            st.set_root_uptake_table(np.zeros(5, dtype=np.int64))
        acc = st.root_uptake_acc()
        assert acc.shape == (3, 4) and not acc.any()
        # the accumulators and the tables travel (checkpoints)
        st.set_root_uptake_acc(np.arange(12))
        assert st.root_uptake_acc().reshape(-1).tolist() == list(range(12))
        t = np.arange(615, dtype=np.int64)
        st.set_root_uptake_table(t)
        assert _same(st.root_uptake_table(), t) and st.root_uptake_overflow() == 614
        st.reset_root_uptake()
        assert not st.root_uptake_table().any() and not st.root_uptake_acc().any()
        # the same ends keep it (zeroed), other ends and no ends turn it off
        st.set_root_uptake_acc(np.arange(12))
        st.set_period_totals([48])
        assert st.uptake_cells.tolist() == [[0, 6], [298, 299]] and not st.root_uptake_acc().any()
        st.set_period_totals([48, 96])
        assert off()
        st.set_root_uptake([(0, 6)], 32)
        st.set_period_totals([])
        assert off()
        # a sharded particle filter routes columns, not accumulators: refused either way round
        st.set_period_totals([48])
        st.set_root_uptake([(0, 6)], 32)
        st.set_filter(48, 8.0, seed=1)
        st.set_period_totals([])
        st.set_filter_shard([0, 4], 0)
        with pytest.raises(HcError, match="sharded particle filter"):
            st.set_period_totals([48])
        with pytest.raises(HcError, match="the period totals are off"):
            st.set_root_uptake([(0, 6)])
        assert off()
    finally:
        st.close()


# ---- 6. the simulations: dump and restore in the middle of a period ---------------------------------------------------------
LAYERS_CM = [[0, 100], [100, 300], [300, 1500]]


def test_resume_in_the_middle_of_a_period_gives_the_uninterrupted_tables(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(200)
    kw = dict(seed=7, psi0=_psi(200, 67), period_ends=ENDS, uptake_layers_cm=LAYERS_CM, uptake_bins=64)
    full = EnsembleSimulation(cols, forcing, 67, **kw)
    full.advance(ROWS)
    want, want_hist, want_out = full.uptake_table(), full.uptake_hist(), full.stepper.root_uptake_outside()
    assert full.uptake_cells.tolist() == [[0, 20], [20, 60], [60, 199]] and full.stepper.root_uptake_overflow() == 0
    full.close()
    first = EnsembleSimulation(cols, forcing, 67, **kw)
    first.advance(30)                                                # period 1 is (5, 48]: its accumulators are half full
    acc = first.stepper.root_uptake_acc()
    assert acc.all()
    path = first.dump(tmp_path / "ckpt.h5")
    first.close()
    resumed = EnsembleSimulation.restore(path, cols, forcing)
    assert _same(resumed.stepper.root_uptake_acc(), acc) and resumed.uptake_bins == 64
    resumed.advance(ROWS - 30)
    got, got_hist, got_out = resumed.uptake_table(), resumed.uptake_hist(), resumed.stepper.root_uptake_outside()
    stats, dist, prof = resumed.uptake_stats(), resumed.uptake_distribution([0.05, 0.5, 0.95]), resumed.uptake_profile()
    resumed.close()
    assert _same(got, want) and _same(got_hist, want_hist) and got_out == want_out
    assert want_hist.shape == (4, 3, 64) and stats["count"].tolist() == [67] * 4
    assert np.all(stats["total_mean_cm"][[1, 3]] > 0) and np.all(stats["total_mean_cm"][[0, 2]] == 0)    # night periods
    # the layers partition the column: their means add up to the total's, to the rounding of three quantised sums
    assert np.allclose(stats["layer_mean_cm"].sum(axis=-1), stats["total_mean_cm"], rtol=0, atol=4 * 2.0 ** -20)
    assert np.allclose(stats["share_of_mean"][[1, 3]].sum(axis=-1), 1.0, atol=1e-4)
    assert dist["share_quantile"].shape == (4, 3, 3) and np.all(dist["share_quantile"][1, 0] <= dist["share_quantile"][1, 2])
    assert prof["profile"].shape == (4, 199) and np.all(prof["profile"][[1, 3]].sum(axis=-1) > 0)
    # the period's profile integrates to the period's mean total (which is floored to 2^-20 cm per member)
    assert np.allclose(prof["profile"].sum(axis=-1) * cols.dz, stats["total_mean_cm"], rtol=0, atol=2.0 ** -19)
    q = prof["depth_quantile_cm"]
    assert q.shape == (4, 2) and np.all(np.isnan(q[[0, 2]])) and np.all(q[[1, 3], 0] <= q[[1, 3], 1])
    with pytest.raises(ValueError, match="uptake_layers_cm needs period_ends"):
        EnsembleSimulation(cols, forcing, 8, psi0=_psi(200, 8), uptake_layers_cm=LAYERS_CM)


# ---- 7. the CLI ------------------------------------------------------------------------------------------------------------
UPTAKE_KEYS = {"uptake_layers_cm", "uptake_cells", "uptake_depth_cm", "uptake_count", "uptake_total_mean_cm", "uptake_total_std_cm",
               "uptake_layer_mean_cm", "uptake_layer_std_cm", "uptake_share_of_mean", "uptake_profile", "uptake_depth_quantile_cm",
               "uptake_overflow"}
UPTAKE_HIST_KEYS = {"uptake_share_hist", "uptake_hist_outside", "uptake_quantile_levels", "uptake_share_quantile"}
BLOCK = {"Rows": 36, "Uptake": {"Layers_cm": LAYERS_CM, "Bins": 128, "Quantiles": [0.05, 0.5, 0.95]}}


@pytest.mark.parametrize("n_points", [0, 2])
def test_cli_block_writes_the_datasets_and_leaves_the_rest_alone(tmp_path, monkeypatch, capsys, n_points):
    import json
    from helpers import cli_params
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    params = cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    pts = {"Points": [{"Soil_Properties": {"n": n}} for n in (1.6, 2.4)][:n_points]} if n_points else {}
    blocks = (("plain", {"Periods": {"Rows": 36}}), ("moments", {"Periods": {"Rows": 36, "Uptake": {"Layers_cm": LAYERS_CM}}}),
              ("uptake", {"Periods": BLOCK}))
    files = {}
    for tag, extra in blocks:
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 128, "Seed": 3, "Days": 2, **pts, **extra}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        capsys.readouterr()
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = (loadResults(tmp_path / f"Run_{tag}_ensemble.h5"), capsys.readouterr().out)
    (plain, log_plain), (mom, log_mom), (upt, log_upt) = files["plain"], files["moments"], files["uptake"]
    lead = (n_points,) if n_points else ()
    assert not [k for k in plain if k.startswith("uptake_")] and "uptake:" not in log_plain
    assert set(mom) - set(plain) == UPTAKE_KEYS and set(upt) - set(plain) == UPTAKE_KEYS | UPTAKE_HIST_KEYS
    assert upt["uptake_layers_cm"].tolist() == LAYERS_CM and upt["uptake_cells"].tolist() == [[0, 20], [20, 60], [60, 199]]
    assert upt["uptake_depth_cm"].shape == (199,) and upt["uptake_depth_cm"][0] == 2.5
    assert upt["uptake_count"].shape == lead + (2,) and np.all(upt["uptake_count"] == 128) and int(upt["uptake_overflow"]) == 0
    for k in ("uptake_total_mean_cm", "uptake_total_std_cm"):
        assert upt[k].shape == lead + (2,)
    for k in ("uptake_layer_mean_cm", "uptake_layer_std_cm", "uptake_share_of_mean"):
        assert upt[k].shape == lead + (2, 3)
    assert upt["uptake_profile"].shape == lead + (2, 199) and upt["uptake_depth_quantile_cm"].shape == lead + (2, 2)
    assert upt["uptake_share_hist"].shape == lead + (2, 3, 128) and upt["uptake_share_hist"].dtype == np.int32
    assert np.all(upt["uptake_share_hist"].sum(axis=-1) == 128) and int(upt["uptake_hist_outside"]) == 0
    assert upt["uptake_quantile_levels"].tolist() == [0.05, 0.5, 0.95] and upt["uptake_share_quantile"].shape == lead + (2, 3, 3)
    # the members' uptake over a period is what the rows' transpiration says, up to the first cell's own call (which
    # `transpiration` leaves out) and the state the solve's last evaluation saw
    assert np.all(upt["uptake_total_mean_cm"] > 0)
    assert np.allclose(upt["uptake_layer_mean_cm"].sum(axis=-1), upt["uptake_total_mean_cm"], rtol=0, atol=4 * 2.0 ** -20)
    for k in UPTAKE_KEYS:                                    # the moments and the profile do not depend on the histograms
        assert _same(mom[k], upt[k]), k
    for k in plain:                                          # every other dataset, byte for byte
        assert _same(plain[k], upt[k]) and _same(plain[k], mom[k]), k
    who = "Sweep 2 points x128" if n_points else "Ensemble x128"
    line = [s for s in log_upt.splitlines() if "uptake:" in s]
    assert len(line) == 1 and line[0].startswith(f" [{who}] uptake: 3 layers over 2 periods, median depth ")
    assert line[0].endswith(" cm") and line == [s for s in log_mom.splitlines() if "uptake:" in s]


@pytest.mark.parametrize("kind", ["ensemble", "sweep", "enkf_sharded"])
def test_two_ranks_sharing_the_card_write_what_one_rank_writes(tmp_path, kind):
    from helpers import cli_params, run_cli_ranks
    params = cli_params(tmp_path)
    ens = {"Members": 250, "Seed": 5, "Days": 2, "Periods": BLOCK}
    if kind == "sweep":                                       # three points dealt to two ranks: 2 + 1
        ens.update(Members=32, Points=[{"Soil_Properties": {"n": n}} for n in (1.6, 2.0, 2.4)])
    if kind == "enkf_sharded":                                # every rank reduces its share of the one point
        ens.update(Members=512, EnKF={"Stride": 24, "Sigma_cm": 8.0, "Sharded": True}, Periods=dict(BLOCK, Rows=24))
    params["Ensemble"] = ens
    one, log1 = run_cli_ranks(tmp_path, "one", params, 1)
    two, log2 = run_cli_ranks(tmp_path, "two", params, 2)
    assert UPTAKE_KEYS | UPTAKE_HIST_KEYS <= set(one) and set(one) == set(two)
    assert int(one["gpus"]) == 1 and int(two["gpus"]) == 2
    assert np.all(one["uptake_count"] == ens["Members"])
    for k in one:
        if k != "gpus":
            assert _same(one[k], two[k]), k
    line = [s for s in log1.splitlines() if "uptake:" in s]
    assert len(line) == 1 and line == [s for s in log2.splitlines() if "uptake:" in s]
