"""Tempered weights of the particle filter (include/hydrocol.h hc_set_filter_tempering), the parts that need no GPU: the
NumPy restatement of the procedure against integers worked out by hand, the target's clamps, the exact comparison against
its 128-bit formulation, the bisection's trial sequence, the CLI's "Filter": {"ESS_floor": ...} key with its refusals, the
summary's keys, and the exported symbols."""
import json
import math
import re

import numpy as np
import pytest

from hydromodel_amd.cli import FILTER_KEYS, filter_ess_floor, filter_settings, run_cli
from hydromodel_amd.stepper import (FILTER_Q_ONE, TEMPER_STEPS, TEMPER_TRIALS, filter_summary, filter_temper_of,
                                    filter_temper_ok, filter_temper_target, filter_temper_weights)

ONE = 1 << 31


def _three(a, k):
    """(Q_k, S_k, q of the two far members) of l = (0, -a, -a) with Python's own exp: 2^31 + 2 q and 2^62 + 2 q^2"""
    q = math.floor(ONE * math.exp((k / 1024) * (0.0 - a - 0.0)))
    return ONE + 2 * q, ONE * ONE + 2 * q * q, q


def _bisect_by_hand(a, T):
    """the issue's procedure on three members, written out with Python integers"""
    trials = []

    def ok(k):
        Q, S, _ = _three(a, k)
        trials.append((k, Q, S))
        return Q * Q >= T * S

    if ok(1024):
        return 1024, trials
    lo, hi = 0, 1024
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if ok(mid):
            lo = mid
        else:
            hi = mid
    return lo, trials


# ---- 1. the restatement against integers worked out by hand -------------------------------------------------------------
@pytest.mark.parametrize("a", [3.0, 5.0, 12.5, 40.0])
def test_three_members_against_hand_computed_integers(a):
    """f = 0.5, n = 3: T = 2.  ESS(1) = (1 + 2 e)^2 / (1 + 2 e^2) with e = exp(-a) <= exp(-3) is below 2, so the weights
    are tempered; the procedure's k and every trial's sums are those of the integers written out above."""
    l = np.array([0.0, -a, -a])
    k, trials, q = filter_temper_of(l, [True] * 3, 0.5)
    want_k, want_trials = _bisect_by_hand(a, 2)
    assert filter_temper_target(0.5, 3) == 2
    assert 0 < k < 1024 and k == want_k and trials == want_trials and len(trials) == TEMPER_TRIALS
    Q, S, far = _three(a, k)
    assert q.dtype == np.int64 and q.tolist() == [ONE, far, far]
    assert Q * Q >= 2 * S                                           # the floor holds at k ...
    Q1, S1, _ = _three(a, 1024)
    assert Q1 * Q1 < 2 * S1                                         # ... and did not at beta = 1
    Qn, Sn, _ = _three(a, k + 1)
    assert Qn * Qn < 2 * Sn                                         # (here ESS falls with beta: k + 1 misses it)


def test_a_floor_that_is_met_takes_one_trial_and_leaves_the_weights():
    l = np.array([0.0, -0.1, -0.1])
    k, trials, q = filter_temper_of(l, [True] * 3, 0.5)
    Q, S, far = _three(0.1, 1024)
    assert k == 1024 and trials == [(1024, Q, S)] and Q * Q >= 2 * S
    assert q.tolist() == [ONE, far, far] == filter_temper_weights(l, [True] * 3, 1024).tolist()


def test_a_target_of_every_member_ends_at_beta_zero():
    """f = 0.999, n = 3: T = 3 = n, which only equal weights reach -- no k >= 1 has them, k = 0 has (ok(0) by construction)"""
    l = np.array([0.0, -5.0, -5.0])
    assert filter_temper_target(0.999, 3) == 3
    k, trials, q = filter_temper_of(l, [True] * 3, 0.999)
    assert k == 0 and q.tolist() == [ONE] * 3 and len(trials) == TEMPER_TRIALS
    assert [t[0] for t in trials] == [1024, 512, 256, 128, 64, 32, 16, 8, 4, 2, 1]
    assert all(Q * Q < 3 * S for _, Q, S in trials)
    assert filter_temper_ok(3 * ONE, 3 * ONE * ONE, 3)              # Q_0^2 = n^2 2^62 >= T n 2^62


def test_uncounted_members_get_zero_and_do_not_count():
    l = np.array([-1.0, np.nan, -1.0 - 6.0, -np.inf, -1.0 - 6.0])
    counted = np.array([True, False, True, False, True])
    k, trials, q = filter_temper_of(l, counted, 0.5)
    k3, trials3, q3 = filter_temper_of(np.array([0.0, -6.0, -6.0]), [True] * 3, 0.5)
    assert (k, trials) == (k3, trials3) and q[counted].tolist() == q3.tolist() and q[~counted].tolist() == [0, 0]
    none = filter_temper_of(l, [False] * 5, 0.5)
    assert none[:2] == (None, []) and none[2].tolist() == [0] * 5


def test_bins_are_weighed_by_their_counts():
    """the bin path: three bins holding (1, 2, 0) members are the three members above"""
    l_b = np.array([0.0, -6.0, -2.0])
    n_b = np.array([1, 2, 0])
    k, trials, q = filter_temper_of(l_b, n_b > 0, 0.5, n_b=n_b)
    k3, trials3, q3 = filter_temper_of(np.array([0.0, -6.0, -6.0]), [True] * 3, 0.5)
    assert (k, trials) == (k3, trials3) and q.tolist() == [q3[0], q3[1], 0]


# ---- 2. the target ------------------------------------------------------------------------------------------------------
def test_target_at_the_clamps():
    assert 0.3 * 10.0 == 3.0 and filter_temper_target(0.3, 10) == 3              # f n on an integer
    up = float(np.nextafter(0.3, 1.0))
    assert up * 10.0 > 3.0 and filter_temper_target(up, 10) == 4                  # ... just above it
    down = float(np.nextafter(0.3, 0.0))
    assert down * 10.0 < 3.0 and filter_temper_target(down, 10) == 3              # ... just below it
    for f in (1e-300, 0.1, 0.5, float(np.nextafter(1.0, 0.0))):
        assert filter_temper_target(f, 1) == 1                                    # n = 1
    assert filter_temper_target(1e-9, 1000) == 1                                  # max(1, .)
    assert filter_temper_target(float(np.nextafter(1.0, 0.0)), 1000) == 1000      # min(n, .)
    assert filter_temper_target(0.9991, 1000) == 1000 and filter_temper_target(0.999, 1000) == 999
    n = (1 << 31) - 1
    assert filter_temper_target(0.5, n) == 1 << 30 and filter_temper_target(float(np.nextafter(1.0, 0.0)), n) == n


# ---- 3. beta = 1 is the untempered weight -------------------------------------------------------------------------------
def test_weights_at_k_1024_are_the_untempered_bits():
    rng = np.random.default_rng(2)
    l = -0.5 * rng.uniform(0.0, 7.0, size=4000) ** 2
    counted = rng.uniform(size=l.size) > 0.1
    s = l[counted].max()
    e = np.where(counted, np.exp(np.where(counted, l - s, 0.0)), 0.0)             # include/hydrocol.h: q_m of a sensor row
    want = np.floor(2.0 ** 31 * e).astype(np.int64)
    got = filter_temper_weights(l, counted, TEMPER_STEPS)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert got.max() == FILTER_Q_ONE and (got[~counted] == 0).all() and (got[counted] == 0).any()
    half = filter_temper_weights(l, counted, 512)
    assert (half >= got).all() and (half[counted] > 0).all()
    assert (filter_temper_weights(l, counted, 0)[counted] == FILTER_Q_ONE).all()


# ---- 4. the comparison --------------------------------------------------------------------------------------------------
def _ok_128(Q, s_hi, s_lo, T):
    """ok(k) as the device forms it: both products in 128-bit unsigned words, S from its two 64-bit words"""
    mask = (1 << 128) - 1
    S = ((s_hi << 64) | s_lo) & mask
    left, right = (Q * Q) & mask, (T * S) & mask
    return left >= right


def test_ok_in_python_integers_is_the_128_bit_formulation():
    n = (1 << 31) - 1
    Q, S, T = n * ONE, n * ONE * ONE, n                          # the largest sums: every member at 2^31
    assert Q < 1 << 62 and S < 1 << 93 and Q * Q < 1 << 124 and T * S < 1 << 124
    assert filter_temper_ok(Q, S, T) and _ok_128(Q, S >> 64, S & ((1 << 64) - 1), T)
    rng = np.random.default_rng(9)
    for _ in range(300):
        m = int(rng.integers(1, 2000))
        q = [int(v) for v in rng.integers(0, ONE + 1, size=m)]
        Q, S = sum(q), sum(v * v for v in q)
        for T in (1, m // 2 + 1, m, Q * Q // max(S, 1), Q * Q // max(S, 1) + 1):
            assert filter_temper_ok(Q, S, T) == _ok_128(Q, S >> 64, S & ((1 << 64) - 1), T) == (Q * Q >= T * S)
    # the boundary: equality holds, one less does not
    assert filter_temper_ok(6, 12, 3) and not filter_temper_ok(6, 13, 3) and filter_temper_ok(0, 0, 5)


# ---- 5. the trial sequence ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_trials_are_the_bisections(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(5, 400))
    l = -0.5 * (rng.uniform(0.0, 30.0, size=n) / rng.uniform(0.5, 6.0)) ** 2
    f = float(rng.uniform(0.05, 0.95))
    k, trials, q = filter_temper_of(l, [True] * n, f)
    T = filter_temper_target(f, n)
    ks = [t[0] for t in trials]
    assert ks[0] == 1024 and len(trials) in (1, TEMPER_TRIALS)
    if len(trials) == 1:
        assert k == 1024 and filter_temper_ok(trials[0][1], trials[0][2], T)
        return
    assert ks[1] == 512 and not filter_temper_ok(trials[0][1], trials[0][2], T)
    lo, hi = 0, 1024
    for width, (kk, Q, S) in zip((1024 >> j for j in range(10)), trials[1:]):
        assert hi - lo == width and kk == (lo + hi) >> 1
        if filter_temper_ok(Q, S, T):
            lo = kk
        else:
            hi = kk
    assert hi - lo == 1 and k == lo
    assert q.tolist() == filter_temper_weights(l, [True] * n, k).tolist()
    qq = [int(v) for v in q]
    assert filter_temper_ok(sum(qq), sum(v * v for v in qq), T)


# ---- 6. the CLI's key ---------------------------------------------------------------------------------------------------
def _ens(**block):
    return {"Members": 8, "Filter": {"Sigma_cm": 10.0, **block}}


def test_the_key_parses_and_leaves_the_filters_tuple():
    assert "ESS_floor" in FILTER_KEYS and FILTER_KEYS[:5] == ("Stride", "Sigma_cm", "Seed", "Sharded", "Soil_Moisture")
    assert filter_ess_floor(_ens(ESS_floor=0.1)) == 0.1 and filter_settings(_ens(ESS_floor=0.1), 1) == (48, 10.0, None)
    assert filter_ess_floor(_ens(ESS_floor=0.5, Stride=24, Seed=3)) == 0.5
    assert filter_ess_floor(_ens()) is None and filter_ess_floor({"Members": 8}) is None
    assert filter_ess_floor({**_ens(ESS_floor=0.25, Sharded=True)}) == 0.25
    pts = [{"Soil_Properties": {"n": 1.6}}, {"Soil_Properties": {"n": 2.4}}]
    assert filter_ess_floor({**_ens(ESS_floor=0.25), "Points": pts}) == 0.25


@pytest.mark.parametrize("ens, message", [
    (_ens(ESS_floor=0), "Filter.ESS_floor = 0 must be a finite number with 0 < ESS_floor < 1"),
    (_ens(ESS_floor=1), "Filter.ESS_floor = 1 must be"),
    (_ens(ESS_floor=1.5), "Filter.ESS_floor = 1.5 must be"),
    (_ens(ESS_floor=-0.1), "Filter.ESS_floor = -0.1 must be"),
    (_ens(ESS_floor=float("nan")), "Filter.ESS_floor = nan must be"),
    (_ens(ESS_floor=float("inf")), "Filter.ESS_floor = inf must be"),
    (_ens(ESS_floor="0.1"), "Filter.ESS_floor = '0.1' must be"),
    (_ens(ESS_floor=None), "Filter.ESS_floor = None must be"),
    (_ens(ESS_floor=True), "Filter.ESS_floor = True must be a finite number with 0 < ESS_floor < 1"),
    (_ens(ESS_floor=False), "Filter.ESS_floor = False must be"),
    (_ens(ESS_floor=0.1, Stride=0), "Filter.ESS_floor needs an active filter (Filter.Stride > 0)"),
    ({"Members": 8, "ESS_floor": 0.1}, "ESS_floor belongs inside the \"Filter\" block"),
    ({"Members": 8, "ESS_floor": 0.1, "Filter": {"Sigma_cm": 10.0}}, "ESS_floor belongs inside the \"Filter\" block"),
    (_ens(ESS_Floor=0.1), "Filter has unknown keys ['ESS_Floor']"),
])
def test_the_key_rejects(ens, message):
    for parse in (filter_ess_floor, filter_settings):
        with pytest.raises(ValueError, match=re.escape(message)):
            parse(ens)


def test_cli_refuses_a_bad_floor_before_any_gpu_work(tmp_path, capsys):
    """The parameter file names no data file that exists and no GPU is asked for: the refusal comes first."""
    from hydromodel_amd.synthetic import default_parameters
    params = default_parameters()
    params["Data_Filename"] = str(tmp_path / "missing.csv")
    params["Ensemble"] = {"Members": 64, "Days": 1, "Filter": {"Sigma_cm": 10.0, "ESS_floor": 1.0}}
    (tmp_path / "p.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as status:
        run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "p.json")])
    assert status.value.code == 1
    assert "Filter.ESS_floor = 1.0 must be a finite number with 0 < ESS_floor < 1" in capsys.readouterr().out


# ---- 7. the summary -----------------------------------------------------------------------------------------------------
def _tables(P=None):
    lead = () if P is None else (P,)
    ft = np.zeros(lead + (5, 4))
    ft[..., 1:] = np.nan
    ft[..., 1, :] = [8, 1.5, -3.0, 5]
    ft[..., 3, :] = [8, 7.0, -2.5, 6]
    tt = np.full(lead + (5, 4), np.nan)
    tt[..., 1, :] = [0.25, 4.2, 4, 11]
    tt[..., 3, :] = [1.0, 7.0, 4, 1]
    return ft, tt


@pytest.mark.parametrize("P", [None, 3])
def test_summary_gains_its_keys_only_with_a_table(P):
    ft, tt = _tables(P)
    lead = () if P is None else (P,)
    plain = filter_summary(ft, 24, 10.0)
    assert set(plain) == {"rows", "count", "ess", "loglik_rows", "survivors", "loglik", "stride", "sigma_cm"}
    assert set(filter_summary(ft, 24, 10.0, temper_table=None)) == set(plain)
    s = filter_summary(ft, 24, 10.0, temper_table=tt)
    assert set(s) - set(plain) == {"beta", "ess_tempered", "ess_target", "tempered_rows"}
    for key in plain:
        assert np.array_equal(np.asarray(s[key]), np.asarray(plain[key]), equal_nan=True), key
    assert s["rows"].tolist() == [24, 72]
    for key, want in (("beta", [0.25, 1.0]), ("ess_tempered", [4.2, 7.0]), ("ess_target", [4.0, 4.0])):
        assert s[key].shape == lead + (2,) and s[key].reshape(-1, 2)[0].tolist() == want
    assert np.all(np.asarray(s["tempered_rows"]) == 1) and np.shape(s["tempered_rows"]) == lead
    assert s["ess"].reshape(-1, 2)[0].tolist() == [1.5, 7.0]         # the stated error's ESS stays the filter's


class _Fake:
    """EnsembleSimulation.filter_summary without a handle: the tables come as arguments."""
    from hydromodel_amd.ensemble import _Run
    filter_summary = _Run.filter_summary
    filter_stride, filter_sigma_cm, filter_soil_moisture = 24, 10.0, None

    def __init__(self, floor):
        self.filter_ess_floor = floor


def test_the_runs_summary_follows_its_setting():
    ft, tt = _tables()
    assert set(_Fake(0.0).filter_summary(ft)) == set(filter_summary(ft, 24, 10.0))
    got = _Fake(0.5).filter_summary(ft, temper_table=tt)
    assert got["beta"].tolist() == [0.25, 1.0] and got["tempered_rows"] == 1


# ---- 8. the symbols -----------------------------------------------------------------------------------------------------
def test_every_declared_symbol_is_exported():
    import __graft_entry__ as ge
    ge.build()
    from hydromodel_amd import _lib
    lib = _lib.load()
    header = (ge.REPO / "include" / "hydrocol.h").read_text()
    for name in ("hc_set_filter_tempering", "hc_get_filter_temper_stats", "hc_set_filter_temper_stats",
                 "hc_get_filter_temper_trials"):
        assert re.search(rf"^int {name}\(hc_handle \*h, ", header, flags=re.M), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
