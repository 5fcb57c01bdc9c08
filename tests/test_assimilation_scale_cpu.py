"""The host side of the assimilation tests at 263 205 members a point (no GPU): the vectorised restatements of
tests/assimilation_scale.py against the looping ones they stand in for, on random inputs at 5 000 members with zero weights
and a single survivor; the long-sum references of the EnKF against the float64 restatements; the sample of members; and
systematic resampling's defining property for stepper.filter_ancestors_of at 263 205 members with C_m N_p above 2^64."""
import numpy as np
import pytest

import assimilation_scale as scale
from hydromodel_amd.stepper import FILTER_Q_ONE, filter_ancestors_of, filter_temper_of

N5 = 5000


def test_the_member_count_crosses_every_threshold_by_the_least():
    assert scale.M == 263205 == 262144 + 1024 + 37 and scale.M % 64 != 0
    assert scale.scan_tiles(scale.M) == 258 and scale.scan_tiles(262144) == scale.SCAN_THREADS      # two tiles in a second round
    assert scale.enkf_tiles(scale.M) == 1029 and scale.enkf_tiles(262144) == scale.ENKF_THREADS     # five in a second stride
    assert scale.M - (scale.scan_tiles(scale.M) - 1) * scale.SCAN_TILE == 37
    assert scale.M - (scale.enkf_tiles(scale.M) - 1) * scale.ENKF_TILE == 37


def test_the_sample_holds_the_edges_and_a_seeded_rest():
    s = scale.sampled_members()
    assert s.size == 256 and np.unique(s).size == 256 and s.min() == 0 and s.max() == scale.M - 1
    assert set(scale.EDGES) <= set(s.tolist()) and np.array_equal(s, scale.sampled_members())
    for m in (0, 255, 256, 1023, 1024, 262143, 262144, 262145, scale.M - 38, scale.M - 37, scale.M - 1):
        assert m in scale.EDGES
    assert scale.sampled_members(100).tolist() == list(range(100))              # fewer members than the sample: all of them


# ---- the water table ---------------------------------------------------------------------------------------------------
def _states(seed, n=N5, D=101, psat=-3.25):
    rng = np.random.default_rng(seed)
    wt = rng.integers(0, D + 1, size=n)                                          # (0: every node saturated; D: none)
    psi = np.where(np.arange(D)[None, :] < wt[:, None], psat - rng.uniform(0.0, 90.0, size=(n, D)),
                   psat + rng.uniform(0.0, 40.0, size=(n, D)))
    psi[rng.integers(0, n, 200), rng.integers(0, D, 200)] = psat                # nodes exactly at psi_sat
    psi[rng.integers(0, n, 200), rng.integers(0, D, 200)] = psat - 1.0          # unsaturated nodes inside the saturated tail
    return psi, psat


@pytest.mark.parametrize("seed", [1, 2])
def test_the_vectorised_water_table_is_the_looping_one(seed):
    from test_gpu_enkf import _find_wtd, _y_of
    psi, psat = _states(seed)
    b = _find_wtd(psi, psat)
    assert (b == 0).any() and (b == psi.shape[1] - 1).any() and np.unique(b).size > 50
    assert np.array_equal(scale.find_wtd(psi, psat), b) and scale.find_wtd(psi, psat).dtype == b.dtype
    y = _y_of(psi, b, psat, 5.0)
    assert np.unique(y).size > np.unique(b).size                                 # the crossing branch was taken
    assert scale.y_of(psi, b, psat, 5.0).tobytes() == y.tobytes()
    shifted = np.minimum(b + 1, psi.shape[1] - 1)                                # indices that are not the water table's
    assert scale.y_of(psi, shifted, psat, 5.0).tobytes() == _y_of(psi, shifted, psat, 5.0).tobytes()


# ---- tempering ---------------------------------------------------------------------------------------------------------
def _loglik(kind, seed):
    rng = np.random.default_rng(seed)
    l = -0.5 * rng.uniform(0.0, 9.0, size=N5) ** 2
    counted = rng.uniform(size=N5) < 0.97
    if kind == "zero weights":                                                   # exp(l - s) below 2^-31: q = 0 at beta = 1
        l[rng.uniform(size=N5) < 0.4] = -400.0
    if kind == "single survivor":
        l[:] = -1e4 - rng.uniform(0.0, 1.0, size=N5)
        l[1234], counted[1234] = 0.0, True
    return l, counted


@pytest.mark.parametrize("floor", [0.5, 0.05, 0.999])
@pytest.mark.parametrize("kind", ["spread", "zero weights", "single survivor"])
def test_the_vectorised_tempering_is_the_looping_one(kind, floor):
    l, counted = _loglik(kind, seed=3)
    k, trials, q = filter_temper_of(l, counted, floor)
    k_v, trials_v, q_v = scale.temper_of(l, counted, floor)
    assert k_v == k and trials_v == trials and np.array_equal(q_v, q) and q_v.dtype == q.dtype
    assert all(type(v) is int for t in trials_v for v in t)
    met = kind != "single survivor" and floor == 0.05                            # the cases whose floor beta = 1 meets
    assert len(trials) == (1 if met else 11) and trials[0][0] == 1024 and (q[~counted] == 0).all()
    assert (k == 1024) == met
    if kind != "spread":
        from hydromodel_amd.stepper import filter_temper_weights
        at_one = filter_temper_weights(l, counted, 1024)
        assert (at_one[counted] == 0).any() and ((at_one > 0).sum() == 1) == (kind == "single survivor")


def test_the_vectorised_tempering_with_bin_counts_and_a_floor_that_is_met():
    rng = np.random.default_rng(5)
    D = 101
    n_b = rng.integers(0, 3000, size=D) * (rng.uniform(size=D) < 0.7)
    l = -0.5 * (0.5 * (np.arange(D) - 40.0)) ** 2
    for floor in (0.5, 0.0002):
        want, got = filter_temper_of(l, n_b > 0, floor, n_b=n_b), scale.temper_of(l, n_b > 0, floor, n_b=n_b)
        assert got[0] == want[0] and got[1] == want[1] and np.array_equal(got[2], want[2])
    assert len(got[1]) == 1 and got[0] == 1024                                    # the small floor is met at beta = 1
    nothing = scale.temper_of(l, np.zeros(D, dtype=bool), 0.5, n_b=np.zeros(D, dtype=np.int64))
    assert nothing[0] is None and nothing[1] == [] and not nothing[2].any()


def test_the_sums_of_a_trial_hold_at_the_largest_weights():
    q = np.full(scale.M, FILTER_Q_ONE, dtype=np.int64)
    Q, S = scale.weighted_sums(np.ones(scale.M, dtype=np.int64), q)
    assert (Q, S) == (scale.M * FILTER_Q_ONE, scale.M * FILTER_Q_ONE ** 2) and S > 1 << 64


# ---- the EnKF's references ---------------------------------------------------------------------------------------------
# The float64 forms sum 5 000 terms with BLAS or pairwise: within 5 000 x 2^-53 = 5.6e-13 of the terms' absolute sum in the
# worst case, and the covariances here are not small against it.  1e-11 leaves a factor of twenty.
def _close(a, b, tol=1e-11):
    return np.abs(np.asarray(a) - np.asarray(b)).max() <= tol * max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("loc", [0.0, 60.0])
@pytest.mark.parametrize("mpp", [N5, N5 // 2])
def test_the_long_sum_references_agree_with_the_float64_restatements(loc, mpp):
    from test_enkf_sm_cpu import analysis_restated
    from test_enkf_sqrt_cpu import _case, rtps_restated, sqrt_analysis_restated
    from test_gpu_enkf import _analysis_numpy
    psi, Y, o, R, zeta = _case(N5, 101, 4, seed=9)
    E = np.random.default_rng(4).standard_normal(Y.shape)
    a, b = scale.analysis(psi, Y, E, o, R, zeta, 5.0, loc, mpp), analysis_restated(psi, Y, E, o, R, zeta, 5.0, loc, mpp)
    for key in ("K", "post", "ybar"):
        assert a[key].shape == b[key].shape and _close(a[key], b[key]), key
    a, b = scale.sqrt_analysis(psi, Y, o, R, zeta, 5.0, loc, mpp), sqrt_analysis_restated(psi, Y, o, R, zeta, 5.0, loc, mpp)
    for key in ("K", "Kr", "dbar", "post", "ybar"):
        assert a[key].shape == b[key].shape and _close(a[key], b[key]), key
    for alpha in (0.0, 0.5):
        got, want = scale.rtps(psi, a["post"], alpha, mpp), rtps_restated(psi, a["post"], alpha, mpp)
        for x, y in zip(got, want):
            assert x.shape == y.shape and _close(x, y)
        assert (got[2][:, -7:] == 1.0).all() and np.array_equal(got[3][:, -7:], a["post"][:, -7:])    # sigma_a = 0: untouched
    K, post = scale.analysis_well(psi, Y[:, 0], E[:, 0], 31, 5.0, 5.0, loc, mpp)
    K_np, post_np = _analysis_numpy(psi, Y[:, 0], E[:, 0], 31, 5.0, 5.0, loc, mpp)
    assert K.shape == K_np.shape and _close(K, K_np) and _close(post, post_np)
    mean, std = scale.mean_std(Y[:, 0])
    assert abs(mean - Y[:, 0].mean()) <= 1e-13 * abs(mean) and abs(std - Y[:, 0].std(ddof=1)) <= 1e-12 * std


def test_one_member_a_point_moves_nothing_in_the_references():
    from test_enkf_sqrt_cpu import _case
    psi, Y, o, R, zeta = _case(3, 101, 4, seed=9)
    res = scale.sqrt_analysis(psi, Y, o, R, zeta, 5.0, 0.0, 1)
    assert np.array_equal(res["post"], psi) and not res["Kr"].any() and not res["dbar"].any()
    sb, sa, f, out = scale.rtps(psi, psi, 0.5, 1)
    assert not sb.any() and not sa.any() and (f == 1.0).all() and np.array_equal(out, psi)


# ---- systematic resampling ---------------------------------------------------------------------------------------------
def test_the_defining_property_holds_for_the_restated_ancestry_above_64_bits():
    rng = np.random.default_rng(8)
    q = rng.integers(0, FILTER_Q_ONE + 1, size=scale.M)
    q[rng.uniform(size=scale.M) < 0.3] = 0                                       # members without a weight
    q[100000:100040] = FILTER_Q_ONE
    Q = int(q.astype(object).sum())
    assert Q * scale.M >= 2 << 64                                                # half the C_m N_p need more than 64 bits
    for r in (0, Q // 3, Q - 1):
        anc = filter_ancestors_of(q, r)
        n_m = scale.assert_systematic(anc, q)
        assert (n_m[q == 0] == 0).all() and n_m.max() >= 2


def test_the_defining_property_refuses_what_is_not_a_systematic_resampling():
    q = np.array([3, 0, 5, 1, 7], dtype=np.int64)
    anc = filter_ancestors_of(q, 4)
    scale.assert_systematic(anc, q)
    for wrong in (np.array([0, 0, 0, 2, 4]), anc[::-1].copy(), np.where(anc == 4, 3, anc)):
        with pytest.raises(AssertionError):
            scale.assert_systematic(wrong, q)
    one = np.zeros(scale.M, dtype=np.int64)                                      # a single survivor fills every slot
    one[777] = 12345
    anc = filter_ancestors_of(one, 12344)
    assert (anc == 777).all() and scale.assert_systematic(anc, one)[777] == scale.M
