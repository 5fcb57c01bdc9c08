"""The particle filter, its tempering, its sensor and window weights, the EnKF and the two sharded paths at 263 205 members a
point (tests/assimilation_scale.py M = 262 144 + 1 024 + 37), where hydrocol.hip runs code that 2 500 members never reach:

  the second round of the tile-offset scan, the strided max over the tiles' lmax, the strided integer sums of the tiles'
  {Q, S} (258 scan tiles > 256); the run ranks of the sharded filter over n_global; the second stride of enkf_finish_kernel
  (1 029 EnKF tiles > 1 024) and a shard that writes its partials from tile 1 024; C_m N_p above 2^64 in filter_slot; slot
  ranges thousands of slots long in filter_fill_kernel.

Well 1 (D = 101), Philox noise, the +-60 cm spread start, the assimilation at row 48.  The checks are those of the modules
whose helpers run here, with their tolerances; every integer comparison is over all members.  On top, the GPU's ancestry
itself is held against systematic resampling's defining property (assimilation_scale.assert_systematic)."""
from fractions import Fraction

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the sharded cases' buffers are torch's)

import assimilation_scale as scale
from assimilation_scale import M
from helpers import digest, golden

pytestmark = pytest.mark.gpu
Q_ONE = 1 << 31
SAMPLE = scale.sampled_members()


def test_the_member_count_is_past_one_round_of_either_reduction():
    assert scale.scan_tiles(M) == 258 > scale.SCAN_THREADS and scale.enkf_tiles(M) == 1029 > scale.ENKF_THREADS
    assert M % 64 != 0 and M % scale.SCAN_TILE == 37 == M % scale.ENKF_TILE


# ---- 1. the bin path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2])
def test_bin_path_ancestry_above_64_bits(P):
    """test_gpu_filter.test_ancestors_weights_and_gather_at_an_assimilation_row and test_increment_and_ess_against_numpy at M
    members a point with sigma = 4 dz: Q N_p >= 2 * 2^64, so at least half the members' C_m N_p need more than 64 bits."""
    from hydromodel_amd.stepper import filter_ancestors_of
    from test_gpu_filter import _q_numpy, _stepper
    N = P * M
    st, cols, forcing = _stepper(1, N, P, "philox")
    D, dz, sigma = cols.dim_d, cols.dz, 4.0 * cols.dz
    obs = int(forcing.wtd_obs[48])
    assert obs >= 0 and forcing.refresh[48] and scale.scan_tiles(M) > scale.SCAN_THREADS
    try:
        st.set_filter(48, sigma, 11)
        st.step_rows(1, 47)
        base_pre = st.filter_base()
        out = st.step_rows(48, 1, want_wtd=True, want_psi=True)
        anc, q, r = st.filter_ancestors(), st.filter_weights(), st.filter_draw()
        psi_post, base_post, table = st.get_state(), st.filter_base(), st.filter_table()
    finally:
        st.close()
    w, forecast = out["wtd"][0], out["psi"][0]
    assert q.shape == (P, D) and r.shape == (P,) and anc.shape == (N,)
    for p in range(P):
        sl = slice(p * M, (p + 1) * M)
        q_np, n, ell, s = _q_numpy(w[sl], obs, D, dz, sigma)
        assert np.all(np.abs(q[p] - q_np) <= 1) and np.all(q[p][n == 0] == 0)
        near = np.flatnonzero((n > 0) & (ell == s))
        assert near.size and np.all(q[p][near] == Q_ONE)
        assert np.unique(q[p][q[p] > 0]).size >= 2                 # weights that differ: a real choice
        qm = q[p][w[sl]]
        Q = int(qm.astype(object).sum())
        print(f"\n point {p}: Q N_p = {Q * M / 2.0 ** 64:.2f} x 2^64, {np.unique(w[sl]).size} occupied bins")
        assert Q * M >= 2 << 64                                    # a condition on the input: filter_slot's 128-bit path
        assert 0 <= int(r[p]) < Q
        local = anc[sl] - p * M
        assert np.array_equal(local, filter_ancestors_of(qm, int(r[p])))
        scale.assert_systematic(local, qm)
        assert table[p, 1, 0] == M and table[p, 1, 3] == np.unique(local).size
        assert np.isnan(table[p, 2:, 1:]).all() and np.all(table[p, 2:, 0] == 0)
        # the increment and the ESS (test_increment_and_ess_against_numpy)
        W = 0.0
        for b in np.flatnonzero(n):
            W += float(n[b]) * np.exp(ell[b] - s)
        inc = s + np.log(W / n.sum()) - np.log(sigma) - 0.5 * np.log(2.0 * np.pi)
        assert abs(table[p, 1, 2] - inc) <= 1e-13 * max(1.0, abs(inc))
        A = sum(int(n[b]) * int(q[p][b]) for b in range(D))
        B = sum(int(n[b]) * int(q[p][b]) ** 2 for b in range(D))
        assert A == Q and abs(table[p, 1, 1] - float(Fraction(A * A, B))) <= 4.5e-16 * float(Fraction(A * A, B))
    assert not np.array_equal(anc, np.arange(N))
    assert np.array_equal(psi_post, forecast[anc])               # the analysis: each slot's ancestor, bit for bit
    assert np.array_equal(base_post, base_pre[anc])


# ---- 2. weight on a few members ------------------------------------------------------------------------------------------
def test_weight_on_twenty_members_fills_ranges_thousands_of_slots_long():
    """test_gpu_filter.test_weight_on_a_few_members_fills_long_slot_ranges at M members a point: 20 members start 40 cm
    apart from the others (above them in point 0, below in point 1), sigma = dz / 20."""
    from hydromodel_amd.stepper import EnsembleStepper, filter_ancestors_of
    _, cols, forcing = digest(1)
    P = 2
    psi0 = golden("g1_tables_1.npz")["initial_cond"]
    few = np.zeros(M, dtype=bool)
    few[7::13161] = True                                           # one in tile 0, one in the last but one, 18 between
    assert few.sum() == 20 and few[250066]
    off = np.concatenate([np.where(few, 20.0, -20.0), np.where(few, -20.0, 20.0)])
    st = EnsembleStepper([cols] * P, forcing, P * M)
    try:
        st.set_state(psi0[None, :] + off[:, None])
        st.set_noise_philox(3, 0)
        st.set_filter(48, cols.dz / 20.0, 5)
        st.step_rows(1, 47)
        base_pre = st.filter_base()
        out = st.step_rows(48, 1, want_wtd=True, want_psi=True)
        anc, q, r = st.filter_ancestors(), st.filter_weights(), st.filter_draw()
        psi_post, base_post, table = st.get_state(), st.filter_base(), st.filter_table()
    finally:
        st.close()
    w = out["wtd"][0]
    longest = 0
    for p in range(P):
        sl = slice(p * M, (p + 1) * M)
        qm, local = q[p][w[sl]], anc[sl] - p * M
        assert np.array_equal(local, filter_ancestors_of(qm, int(r[p])))
        n_m = scale.assert_systematic(local, qm)
        assert table[p, 1, 3] == np.count_nonzero(n_m)
        longest = max(longest, int(n_m.max()))
    print(f"\n longest slot range: {longest}")
    assert longest > 4096
    assert np.array_equal(psi_post, out["psi"][0][anc]) and np.array_equal(base_post, base_pre[anc])


# ---- 3. the per-member weights: a sensor row and a windowed row ----------------------------------------------------------
def _sums_in_the_documented_order(qm, ell, counted, anc, table, columns, log_terms, extra_terms):
    """test_gpu_filter_sm.test_increment_ess_and_sensor_diagnostics_against_numpy for one point of M members: the increment
    from W = filter_tile_sum(exp(l - s)), the exact ESS, and the means and stds of ``columns`` = [(table row, value column,
    x [M], std bound relative)] to the bit of filter_tile_sum and within the bound of the exact ones.  ``log_terms``: the
    errors whose logarithm the increment subtracts, one 0.5 log(2 pi) each.  The bound is that test's (and the window
    module's twin's), (N_p + 16 + extra_terms) 2^-53: N_p positive terms, the ulps of exp and log, m_w more log terms."""
    from hydromodel_amd.stepper import filter_tile_sum
    # (At M the bound is 2.9e-11: against the exact values it only tells a sum from a wrong one.  What checks the order of
    #  the strided sums is the equality with filter_tile_sum, to the bit, of the means; the increment came out equal too.)
    assert counted.all()
    s = ell.max()
    e = np.exp(ell - s)
    W = filter_tile_sum(e)
    inc = s + np.log(W / M)
    for term in log_terms:
        inc -= np.log(term)
    inc -= 0.5 * float(len(log_terms)) * np.log(2.0 * np.pi)
    bound = (M + 16 + extra_terms) * 2.0 ** -53
    print(f"\n increment {table[2]!r} against {inc!r}: {abs(table[2] - inc):.3e} (bound {bound * max(1.0, abs(inc)):.3e})")
    assert table[0] == M and abs(table[2] - inc) <= bound * max(1.0, abs(inc))
    q = qm.astype(object)
    ess = Fraction(int(q.sum()) ** 2, int((q * q).sum()))
    assert abs(table[1] - float(ess)) <= 4.5e-16 * float(ess)                      # within 2 ulp
    assert table[3] == np.unique(anc).size
    for row, col, x, relative in columns:
        mean = filter_tile_sum(x) / M
        std = np.sqrt(filter_tile_sum((x - mean) * (x - mean)) / (M - 1))
        exact_mean, exact_std = scale.mean_std(x)
        assert row[col] == mean and abs(mean - exact_mean) <= bound * max(1.0, abs(exact_mean))
        assert abs(row[col + 1] - std) <= bound * (max(1.0, std) if relative else 1.0)
        assert abs(row[col + 1] - exact_std) <= bound * max(1.0, exact_std)


def test_sensor_row_member_weights_and_ancestry():
    """test_gpu_filter_sm._row_48 / _check_row_48 at (1, 1, M): l_m bit for bit, q_m within 1 of NumPy's, the ancestry bit
    for bit; the increment, ESS, sensor means and stds of test_increment_ess_and_sensor_diagnostics_against_numpy."""
    import test_gpu_filter_sm as sm
    g = sm._row_48(1, 1, M, "philox")
    sm._check_row_48(g, 1, M)
    assert scale.scan_tiles(g["qm"].size) > scale.SCAN_THREADS
    scale.assert_systematic(g["anc"], g["qm"])
    theta, post = g["theta"], g["theta"][g["anc"]]
    columns = [(g["smt"][0, 1, i], col, np.ascontiguousarray(x[:, i]), False) for i in range(2)
               for col, x in ((2, theta), (4, post))]
    _sums_in_the_documented_order(g["qm"], g["ell"], (g["w"] < g["cols"].dim_d) & np.isfinite(g["ell"]), g["anc"],
                                  g["table"][0, 1], columns, [g["sigma"], *sm.SIGMAS], 0)


def test_windowed_row_member_weights_and_ancestry():
    """test_gpu_filter_window._row_48 / _check_row_48 at (1, 1, M) with two sensors: the same comparisons with the lagged
    rows' terms; the window's means and stds of test_increment_ess_and_window_diagnostics_against_numpy."""
    import test_gpu_filter_window as win
    g = win._row_48(1, 1, M, "philox", 2)
    win._check_row_48(g, 1, M, 2)
    assert scale.scan_tiles(g["qm"].size) > scale.SCAN_THREADS
    scale.assert_systematic(g["anc"], g["qm"])
    b, dz = g["cap"][0], g["cols"].dz
    counted = (np.maximum(g["w"], b.max(axis=0)) < g["cols"].dim_d) & np.isfinite(g["ell"])
    columns = [(g["wint"][0, 1, j], 2, dz * b[j].astype(np.float64), True) for j in range(3)]
    _sums_in_the_documented_order(g["qm"], g["ell"], counted, g["anc"], g["table"][0, 1], columns,
                                  [g["sigma"], *win.SIGMAS, g["sigma"], g["sigma"], g["sigma"]], 3)


# ---- 4. tempering ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bins", "sensor"])
def test_tempering_bisection_over_the_strided_sums(kind):
    """test_gpu_filter_temper._check at (1, M) with the module's floor: every trial's decision, the bisection's sequence,
    the final sums, the weights, the draw and the ancestry; the eleven trials (k, Q_k, S_k) and the k that is kept equal
    the restatement's (assimilation_scale.temper_of) as Python integers.  ``margin=False``: _check says why its
    condition on the restatement's trials is not asked of an input at this member count."""
    import test_gpu_filter_temper as temper
    runs = {}

    def run(*args, **kw):                                           # this test's two runs at M members, kept for its length
        key = (args, tuple(sorted(kw.items())))
        if key not in runs:
            runs[key] = temper._run.__wrapped__(*args, **kw)
        return runs[key]

    seen = temper._check(kind, 1, M, well=1, temper_of=scale.temper_of, margin=False, run=run)
    got, twin = run(kind, 1, M, temper.FLOOR, "philox", well=1), run(kind, 1, M, 0.0, "philox", well=1)
    assert len(runs) == 2
    tt, h, h1 = got["ttable"][0, 1], got["hooks"][0], twin["hooks"][0]
    assert scale.scan_tiles(M) > scale.SCAN_THREADS and 0.0 < tt[0] < 1.0           # the row was tempered: beta < 1
    ones = np.ones(M, dtype=np.int64)
    qm = h["q_bins"][0][h["w"]] if kind == "bins" else h["qm"]
    scale.assert_systematic(h["anc"], qm)
    (trials, trials_np), = seen
    assert trials == trials_np and len(trials) == 11
    assert all(type(v) is int for t in trials + trials_np for v in t)
    q1 = h1["q_bins"][0][h1["w"]] if kind == "bins" else h1["qm"]
    assert trials[0] == (1024,) + scale.weighted_sums(ones, q1)                     # beta = 1: the twin's hooked weights
    assert (int(round(tt[0] * 1024)),) + scale.weighted_sums(ones, qm) in trials    # the k that was kept


# ---- 5. the EnKF -----------------------------------------------------------------------------------------------------------
def test_enkf_analysis_over_the_strided_column_sums():
    """test_gpu_enkf.test_analysis_against_numpy at (1, 1, M, loc 60) with its tolerances; the reference's sums over the
    members in np.longdouble (assimilation_scale.analysis_well).  The draw is restated with Python integers for a sample of
    256 members: the tile and round edges 0, 255, 256, 1 023, 1 024, 262 143, 262 144, 262 145, M - 38, M - 37, M - 1 and a
    seeded random rest; every other comparison is over all members."""
    from test_gpu_enkf import _check_analysis
    assert scale.enkf_tiles(M) > scale.ENKF_THREADS
    _check_analysis(1, 1, M, 60.0, "philox", find_wtd=scale.find_wtd, y_of=scale.y_of, analysis=scale.analysis_well,
                    eps_members=SAMPLE, mean_std=scale.mean_std)


def test_enkf_square_root_analysis_with_relaxation_over_the_strided_column_sums():
    """test_gpu_enkf_sqrt.test_analysis_against_numpy at (1, 1, M, loc 60, three sensors, sqrt, alpha = 0.5) with its
    tolerances: the squared-anomaly partials go through enkf_finish_kernel too.  The references' sums in np.longdouble."""
    from test_gpu_enkf_sqrt import _check_analysis
    assert scale.enkf_tiles(M) > scale.ENKF_THREADS
    _check_analysis(1, 1, M, 60.0, 3, "philox", "sqrt", 0.5, find_wtd=scale.find_wtd, y_of=scale.y_of,
                    sqrt_analysis=scale.sqrt_analysis, analysis=scale.analysis, rtps=scale.rtps, mean_std=scale.mean_std,
                    std_columns=scale.std_columns)


# ---- 6. two handles ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["stochastic-well", "sqrt-relaxed"])
def test_sharded_enkf_second_handle_starts_at_tile_1024(case):
    """Members [0, 262 144) and [262 144, M) on two handles against the one that holds them all, bit for bit, over the
    analysis at row 48 (test_gpu_enkf_shard's machinery): the second handle writes tiles 1 024 ... 1 028."""
    import test_gpu_enkf_shard as shard
    bounds = [(0, 262144), (262144, M)]
    whole = shard._handle(0, M, case, n_global=M, well=1)
    try:
        whole.step_rows(1, 48)
        ref = shard._results(whole, case)
    finally:
        whole.close()
    assert ref["table"][0, 1, 0] == M and np.abs(ref["gain"]).max() > 0.0

    def look(handles):
        assert handles[1].get_enkf_shard() == (M, 262144)
        assert handles[1].get_enkf_shard()[1] // scale.ENKF_TILE == 1024 == scale.ENKF_THREADS    # its first tile
        assert scale.enkf_tiles(M) - 1024 == 5

    got, calls = shard._run_together(bounds, case, rows=48, n_global=M, well=1, look=look)
    assert calls == (8 if shard.CASES[case][1] > 0 else 4)
    assert shard._bits(np.concatenate([g["psi"] for g in got]), ref["psi"])
    assert shard._bits(sum(g["moments"] for g in got), ref["moments"])
    for g in got:
        for key in ("table", "gain", "full_gain"):
            assert shard._bits(g[key], ref[key]), key


def test_sharded_filter_ranks_the_runs_past_one_round():
    """Members [0, 100 001) and [100 001, M) on two handles against the one that holds them all, bit for bit, over the
    assimilation at row 48 (test_gpu_filter_shard's machinery): the run ranks are a scan over 258 tiles of slots."""
    import test_gpu_filter_shard as shard
    bounds = [0, 100001, M]
    st = shard._handle(0, M, None, None, "philox", "spread", M, 1)
    try:
        shard._step(st, 0, M, 48, "philox", M)
        ref = shard._results(st, "philox")
    finally:
        st.close()
    assert ref["table"][0, 1, 0] == M and not np.array_equal(ref["anc"], np.arange(M))
    assert scale.scan_tiles(bounds[-1]) > scale.SCAN_THREADS
    got, card, failures = shard._run_together(bounds, rows=48, well=1)
    assert failures == [None, None], failures
    assert card.gathers == [1, 1] and card.routes == [1, 1]
    assert any(sum(words) for k in range(card.n) for words in card.sent[k])    # columns did change hands
    shard._assert_like_one(got, ref, bounds, "spread at M")
