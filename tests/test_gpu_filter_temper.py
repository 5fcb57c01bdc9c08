"""Tempered weights of the particle filter on the GPU (include/hydrocol.h hc_set_filter_tempering), on the bin path and on
sensor rows: from the hooks alone every trial's decision against Python's integer comparison, the bisection's sequence, the
final sums against the hooked weights, the weights against NumPy, the ancestry as an integer function of the hooked weights
and draw, the draw against the untempered twin's Philox value, the filter's own entries against the twin's bits; the NumPy
restatement's k against the device's; a floor the forecast already meets against the twin without the key; the same bits
at another launch length, with the points on two handles, across a checkpoint and with the members on two handles; host
noise; period totals that follow the tempered ancestry; the CLI's "Filter": {"ESS_floor": ...} key."""
import json
import re
import threading
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the sharded case's buffer is torch's)

from helpers import digest, golden
from helpers import cli_params as _cli_params
from test_gpu_enkf import _spread

pytestmark = pytest.mark.gpu
Q_ONE = 1 << 31
WELL, STRIDE, SEED, FSEED, SPREAD_SEED = 200, 48, 7, 11, 12
SIGMA_DZ = 0.5                  # the well's error as a fraction of dz: a bin next to the nearest one keeps exp(-2)
FLOOR = 0.5
NODES = [6, 45]                 # 30 cm and 225 cm, as in test_gpu_filter_sm.py
VALUES = [0.24, 0.36]
SIGMAS = np.array([0.05, 0.08])
MASK = (1 << 64) - 1


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _initial(N, well=WELL):
    psi = _spread(golden(f"g1_tables_{well}.npz")["initial_cond"], N, seed=SPREAD_SEED)
    psi.setflags(write=False)
    return psi


def _record(T, rows):
    v = np.full((T, len(VALUES)), np.nan)
    for r in rows:
        v[r] = VALUES
    return v


@lru_cache(maxsize=None)
def _run(kind, P, mpp, floor, noise="philox", rows=(48,), rpl=0, point=None, sigma_dz=SIGMA_DZ, well=WELL):
    """One handle stepped through the assimilations at ``rows``: the hooks after each of them and the tables at the end.
    ``kind``: "bins" (the well alone) or "sensor" (two sensors on every assimilation row).  ``point``: the handle holds
    that point of the P alone (its members of the whole ensemble, its own stream).  Computed once per setting, shared
    and left unchanged."""
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(well)
    n_pts = 1 if point is not None else P
    lo = 0 if point is None else point * mpp
    N = n_pts * mpp
    st = EnsembleStepper([cols] * n_pts if n_pts > 1 else cols, forcing, N)
    host = noise == "numpy"
    hooks = []
    try:
        st.set_state(np.ascontiguousarray(_initial(P * mpp, well)[lo:lo + N]))
        if host:
            st.set_noise_host(np.random.default_rng(SEED).standard_normal((P * mpp, cols.dim_d))[lo:lo + N])
        else:
            st.set_noise_philox(SEED, lo)
        if rpl:
            st.set_rows_per_launch(rpl)
        st.set_filter(STRIDE, sigma_dz * cols.dz, FSEED)
        if kind == "sensor":
            st.set_filter_soil_moisture(NODES, _record(st.T, rows), SIGMAS)
        if floor:
            st.set_filter_tempering(floor)
        at = 1

        def fresh(r0, n):
            if not host:
                return {}
            f = np.random.default_rng(1000 + r0).standard_normal((st.n_refresh(r0, n), P * mpp, st.D))
            return {"fresh_noise": np.ascontiguousarray(f[:, lo:lo + N])}

        for row in rows:
            assert int(forcing.wtd_obs[row]) >= 0
            st.step_rows(at, row - at, **fresh(at, row - at))
            base_pre = st.get_noise_base() if host else st.filter_base()
            out = st.step_rows(row, 1, want_wtd=True, want_psi=True, **fresh(row, 1))
            h = dict(row=row, obs=int(forcing.wtd_obs[row]), w=out["wtd"][0].astype(np.int64), forecast=out["psi"][0],
                     base_pre=base_pre, anc=st.filter_ancestors(), q_bins=st.filter_weights(), r=st.filter_draw(),
                     psi=st.get_state(), base=st.get_noise_base() if host else st.filter_base())
            if kind == "sensor":
                assert st.filter_sm_width() == 2
                h.update(qm=st.filter_member_weights(), ell=st.filter_loglik())
            if floor:
                h["trials"] = st.filter_temper_trials()
            hooks.append(h)
            at = row + 1
        res = dict(hooks=hooks, table=st.filter_table(), psi=st.get_state(), moments=np.asarray(st.moments()), cols=cols,
                   base=st.get_noise_base() if host else st.filter_base())
        if kind == "sensor":
            res["smt"] = st.filter_sm_table()
        if floor:
            res["ttable"] = st.filter_temper_table()
        return res
    finally:
        st.close()


def _trials_of(rows):
    """[(k, Q_k, S_k)] of a point's hook rows [11][4], the unused rows dropped"""
    out = []
    for k, Q, lo, hi in rows.tolist():
        if k >= 0:
            out.append((k, Q & MASK, ((hi & MASK) << 64) | (lo & MASK)))
    assert [r[0] for r in rows.tolist()[len(out):]] == [-1] * (len(rows) - len(out))
    return out


def _loglik_of(kind, h, sl, cols, sigma_dz=SIGMA_DZ):
    """(l, counted, multiplicity) of a point's weights: per bin on the bin path, per member on a sensor row"""
    D = cols.dim_d
    if kind == "bins":
        n_b = np.bincount(h["w"][sl], minlength=D)[:D]
        t = cols.dz * (np.arange(D) - h["obs"]).astype(np.float64) / (sigma_dz * cols.dz)
        return -0.5 * (t * t), n_b > 0, n_b
    ell = h["ell"][sl]
    return ell, (h["w"][sl] < D) & np.isfinite(ell), None


def _check(kind, P, mpp, noise="philox", floor=FLOOR, well=WELL, temper_of=None, margin=True, run=None):
    """``temper_of``: the restatement of the bisection (None: stepper.filter_temper_of; a large ensemble passes a form of it
    without a loop over the members).  ``margin`` = False: the restatement's trials are held against the device's as
    integers without the condition that they clear the weights' rounding (below).  ``run``: stands in for the module's
    cached _run.  Returns, per point, the device's trials and the restatement's."""
    from hydromodel_amd.stepper import (filter_ancestors_of, filter_temper_of, filter_temper_ok, filter_temper_target,
                                        filter_temper_weights)
    temper_of = temper_of or filter_temper_of
    kw = {} if well == WELL else {"well": well}
    run = run or _run
    got, twin = run(kind, P, mpp, floor, noise, **kw), run(kind, P, mpp, 0.0, noise, **kw)
    seen = []
    cols, h, h1 = got["cols"], got["hooks"][0], twin["hooks"][0]
    assert _same(h["w"], h1["w"]) and _same(h["forecast"], h1["forecast"])          # one forecast, two resamplings
    # entries 0-2 of the filter's table and the sensors' forecast columns: the stated error's, the twin's bits
    assert _same(got["table"][:, :, :3], twin["table"][:, :, :3])
    if kind == "sensor":
        assert _same(got["smt"][..., :4], twin["smt"][..., :4])
        assert not h["q_bins"].any()
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        l, counted, n_b = _loglik_of(kind, h, sl, cols)
        mult = np.ones(l.size, dtype=np.int64) if n_b is None else n_b
        n = int(mult[counted].sum())
        t, tt = got["table"][p, 1], got["ttable"][p, 1]
        T = filter_temper_target(floor, n)
        assert t[0] == n == mpp and tt[2] == T
        # every trial's decision is Python's integer comparison of its sums, and the sequence is the bisection's
        trials = _trials_of(h["trials"][p])
        assert tt[3] == len(trials) == 11 and trials[0][0] == 1024
        assert not filter_temper_ok(trials[0][1], trials[0][2], T)                  # ESS(1) < T: this row needed it
        lo, hi = 0, 1024
        for kk, Q, S in trials[1:]:
            assert hi - lo > 1 and kk == (lo + hi) >> 1
            lo, hi = (kk, hi) if filter_temper_ok(Q, S, T) else (lo, kk)
        k = lo
        assert hi - lo == 1 and tt[0] == k / 1024
        # the hooked weights: what the resampling used
        q = h["q_bins"][p] if kind == "bins" else h["qm"][sl]
        qm = q[h["w"][sl]] if kind == "bins" else q
        Qk = sum(int(a) * int(b) for a, b in zip(mult, q))
        Sk = sum(int(a) * int(b) * int(b) for a, b in zip(mult, q))
        assert Qk == sum(int(v) for v in qm)
        if k > 0:
            assert (k, Qk, Sk) in trials                                            # the sums of the trial that set lo
        else:
            assert (Qk, Sk) == (n * Q_ONE, n * Q_ONE * Q_ONE)
        assert Qk * Qk >= T * Sk
        ess = Fraction(Qk * Qk, Sk)
        assert abs(tt[1] - float(ess)) <= 4.5e-16 * float(ess)                      # within 2 ulp, as the filter's ESS
        q_np = filter_temper_weights(l, counted, k)
        print(f"\n {kind} P={P} N_p={mpp} {noise} point {p}: k = {k}, T = {T}, ESS(1) = "
              f"{float(Fraction(trials[0][1] ** 2, trials[0][2])):.3f}, ESS(beta) = {tt[1]:.3f}, "
              f"max |q - numpy| = {int(np.abs(q - q_np).max())}")
        assert np.all(np.abs(q - q_np) <= 1) and np.all(q[~counted] == 0)           # the device's exp against NumPy's
        assert q.max() == Q_ONE
        # the ancestry: an integer function of the hooked weights and the hooked draw
        r = int(h["r"][p])
        assert 0 <= r < Qk
        assert np.array_equal(h["anc"][sl], filter_ancestors_of(qm, r) + p * mpp)
        assert t[3] == np.unique(h["anc"][sl]).size
        # the tempered draw used the twin's Philox value x: r = floor(x Q / 2^64) on both sides
        q1 = h1["q_bins"][p][h1["w"][sl]] if kind == "bins" else h1["qm"][sl]
        Q1, r1 = sum(int(v) for v in q1), int(h1["r"][p])
        assert Q1 == trials[0][1]
        assert r * Q1 < (r1 + 1) * Qk and r1 * Qk < (r + 1) * Q1
        # the restatement's k is the device's.  A +-1 in a weight moves Q by at most n and S by at most 2 Q + n; with
        # u = n / Q <= n / 2^31 (the likeliest member has 2^31) and S >= Q^2 / n that is a relative change of Q^2 / (T S)
        # of at most (4 u + 2 u^2) / (1 - 2 u - u^2) < 4.001 u.  Every trial of the restatement must clear that margin: a
        # condition of the input, named here.
        k_np, trials_np, _ = temper_of(l, counted, floor, n_b=n_b)
        if margin:
            for kk, Q, S in trials_np:
                assert abs(Q * Q - T * S) * 1000 * Q_ONE > 4001 * n * T * S, \
                    f"spread seed {SPREAD_SEED}, {kind}, point {p}: the trial at k = {kk} is within the weights' rounding of T"
            assert k_np == k and [v[0] for v in trials_np] == [v[0] for v in trials]
        else:
            # The margin is 4.001 n / 2^31 of T and grows with n, while one step of k moves Q^2 / S by a fraction that
            # does not: at 263 205 members, well 1, this sigma and floor, the closest trial of eight spread seeds lay at
            # 0.008 ... 0.78 of it for either kind.  Without it the comparison is the plain one: every trial (k, Q_k, S_k)
            # of the restatement equals the device's as Python integers, and so does k.  Should it ever fail with sums
            # that differ by no more than n in Q and 2 Q + n in S, the device's exp and NumPy's rounded a weight apart
            # (+-1 a weight is all the weights' own check allows); a larger difference is a tile lost or counted twice.
            for a, b in zip(trials, trials_np):
                assert a == b, (a, b, "differences", a[1] - b[1], a[2] - b[2], "rounding allows", n, 2 * b[1] + n)
            assert trials_np == trials and k_np == k
        seen.append((trials, trials_np))
    assert _same(h["psi"], h["forecast"][h["anc"]]) and _same(h["base"], h["base_pre"][h["anc"]])
    assert not _same(h["anc"], h1["anc"])                                           # tempering changed who survives
    return seen


# ---- 1. the bin path and the sensor row, from the hooks ------------------------------------------------------------------
@pytest.mark.parametrize("P, mpp", [(1, 1000), (2, 2500)])
@pytest.mark.parametrize("kind", ["bins", "sensor"])
def test_trials_weights_draw_and_ancestry_from_the_hooks(kind, P, mpp):
    """2 500 members: three tiles of the prefix scan, not a multiple of 64."""
    _check(kind, P, mpp)


@pytest.mark.parametrize("kind", ["bins", "sensor"])
def test_host_noise(kind):
    _check(kind, 1, 1000, noise="numpy")
    a, b = _run(kind, 1, 1000, FLOOR, "numpy"), _run(kind, 1, 1000, FLOOR, "numpy", rpl=7)
    for key in ("psi", "base", "table", "ttable", "moments"):
        assert _same(a[key], b[key]), key


# ---- 2. a floor the forecast already meets -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bins", "sensor"])
def test_a_floor_that_is_met_is_the_run_without_the_key(kind):
    from hydromodel_amd.stepper import filter_temper_ok, filter_temper_target
    floor, P, mpp = 0.002, 2, 2500
    T = filter_temper_target(floor, mpp)
    assert T in (5, 6)
    got, twin = _run(kind, P, mpp, floor, rows=(48, 96)), _run(kind, P, mpp, 0.0, rows=(48, 96))
    for key in ("psi", "base", "table", "moments") + (("smt",) if kind == "sensor" else ()):
        assert _same(got[key], twin[key]), key
    for h, h1 in zip(got["hooks"], twin["hooks"]):
        for key in ("anc", "q_bins", "r", "psi", "base") + (("qm",) if kind == "sensor" else ()):
            assert _same(h[key], h1[key]), (h["row"], key)
        assert not _same(h["anc"], np.arange(P * mpp))
    for p in range(P):
        tt = got["ttable"][p]
        trials = _trials_of(got["hooks"][-1]["trials"][p])
        assert len(trials) == 1 and trials[0][0] == 1024 and filter_temper_ok(trials[0][1], trials[0][2], T)
        for slot in (1, 2):
            assert tt[slot].tolist() == [1.0, got["table"][p, slot, 1], float(T), 1.0]   # the filter's ESS, to the bit
        assert np.isnan(tt[0]).all() and np.isnan(tt[3:]).all()


# ---- 3. the same bits --------------------------------------------------------------------------------------------------
KEYS = ("psi", "base", "table", "ttable", "moments")


@pytest.mark.parametrize("kind", ["bins", "sensor"])
def test_launch_length_and_the_dealing_of_points_do_not_change_a_bit(kind):
    P, mpp, rows = 2, 2500, (48, 96)
    whole = _run(kind, P, mpp, FLOOR, rows=rows)
    assert np.all(whole["ttable"][:, 1, 0] < 1.0) and np.isfinite(whole["ttable"][:, 1:3]).all()    # row 48 was tempered
    short = _run(kind, P, mpp, FLOOR, rows=rows, rpl=7)
    for key in KEYS + (("smt",) if kind == "sensor" else ()):
        assert _same(whole[key], short[key]), key
    for a, b in zip(whole["hooks"], short["hooks"]):
        for key in ("anc", "q_bins", "r", "trials"):
            assert _same(a[key], b[key]), (a["row"], key)
    for p in range(P):
        part = _run(kind, P, mpp, FLOOR, rows=rows, point=p)
        assert _same(part["psi"], whole["psi"][p * mpp:(p + 1) * mpp]) and _same(part["base"], whole["base"][p * mpp:(p + 1) * mpp])
        assert _same(part["table"][0], whole["table"][p]) and _same(part["ttable"][0], whole["ttable"][p])
        for a, b in zip(part["hooks"], whole["hooks"]):
            assert _same(a["trials"][0], b["trials"][p]) and _same(a["r"][0], b["r"][p])
            assert _same(a["anc"] + p * mpp, b["anc"][p * mpp:(p + 1) * mpp])


def test_dump_and_restore_continue_a_tempered_run_bit_for_bit(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(WELL)
    kw = dict(seed=6, psi0=np.array(_initial(300)), filter_stride=STRIDE, filter_sigma_cm=SIGMA_DZ * cols.dz,
              filter_ess_floor=FLOOR)

    def state(sim):
        return [sim.stepper.get_state(), sim.filter_table(), sim.filter_temper_table(), sim.moments(),
                sim.stepper.filter_base()]

    whole = EnsembleSimulation(cols, forcing, 300, **kw)
    try:
        whole.advance(48)
        path = whole.dump(tmp_path / "ck.h5")
        whole.advance(48)
        want, summary = state(whole), whole.filter_summary()
    finally:
        whole.close()
    back = EnsembleSimulation.restore(path, cols, forcing)
    try:
        assert back.next_row == 49 and back.filter_ess_floor == FLOOR and back.stepper.filter_ess_floor == FLOOR
        assert _same(back.filter_temper_table()[1], want[2][1])
        back.advance(48)
        got = state(back)
    finally:
        back.close()
    for a, b in zip(want, got):
        assert _same(a, b)
    assert summary["rows"].tolist() == [48, 96] and summary["beta"][0] < 1.0 and summary["tempered_rows"] >= 1
    assert np.all(summary["ess_tempered"] >= summary["ess_target"]) and summary["ess"][0] < summary["ess_target"][0]


def test_two_handles_temper_like_the_one_that_holds_every_member():
    """Members [0, 512) and [512, 1000) of a well-only run: every handle runs the same kernels on the same gathered
    indices and finds the same k."""
    import test_gpu_filter_shard as shard
    _, cols, _ = digest(WELL)
    sigma, bounds, noise = SIGMA_DZ * cols.dz, shard.TWO, "philox"

    def results(st):
        return dict(psi=st.get_state(), base=st.filter_base(), table=st.filter_table(), ttable=st.filter_temper_table(),
                    weights=st.filter_weights(), draw=st.filter_draw(), anc=st.filter_ancestors(),
                    trials=st.filter_temper_trials(), moments=np.asarray(st.moments()))

    one = shard._handle(0, shard.N, None, sigma)
    try:
        one.set_filter_tempering(FLOOR)
        shard._step(one, 0, shard.N, shard.ROWS, noise)
        ref = results(one)
    finally:
        one.close()
    assert ref["ttable"][0, 1, 0] < 1.0 and ref["ttable"][0, 1, 3] == 11 and np.isfinite(ref["ttable"][0, 1:3]).all()
    S = len(bounds) - 1
    card = shard.CardExchange(S)                                    # every barrier on a timeout
    handles = [shard._handle(bounds[k], bounds[k + 1], (bounds, k, card.of(k)), sigma) for k in range(S)]
    failures = [None] * S

    def work(k):
        try:
            handles[k].set_filter_tempering(FLOOR)
            shard._step(handles[k], bounds[k], bounds[k + 1], shard.ROWS, noise)
        except BaseException as e:  # noqa: BLE001
            failures[k] = e
            card.barrier.abort()
    try:
        threads = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(S)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
        assert not any(t.is_alive() for t in threads), "a handle's step did not return"
        assert failures == [None] * S, failures
        got = [results(st) for st in handles]
    finally:
        for st in handles:
            st.close()
    for key in ("psi", "base", "anc"):
        assert _same(np.concatenate([g[key] for g in got]), ref[key]), key
    assert _same(sum(g["moments"] for g in got), ref["moments"])
    for g in got:
        for key in ("table", "ttable", "weights", "draw", "trials"):
            assert _same(g[key], ref[key]), key


# ---- 4. period totals ----------------------------------------------------------------------------------------------------
def test_period_totals_follow_the_tempered_ancestry():
    from hydromodel_amd.stepper import EnsembleStepper, period_totals_of
    _, cols, forcing = digest(WELL)
    N, ends, thr, fexp = 67, [72, 96], [], [12, 12]
    psi = np.array(_initial(N))

    def run(floor):
        st = EnsembleStepper(cols, forcing, N)
        try:
            st.set_state(psi)
            st.set_noise_philox(SEED, 0)
            st.set_filter(STRIDE, SIGMA_DZ * cols.dz, seed=FSEED)
            if floor:
                st.set_filter_tempering(floor)
            st.set_period_totals(ends, thr, 32, fexp)
            a = st.step_rows(1, 48, want_diag=True, want_wtd=True)
            anc = st.filter_ancestors()
            beta = st.filter_temper_table()[0, 1, 0] if floor else 1.0
            b = st.step_rows(49, 48, want_diag=True, want_wtd=True)
            hf, hw = st.period_totals_hists()
            return (np.concatenate([a["diag"], b["diag"]]), np.concatenate([a["wtd"], b["wtd"]]), anc, beta,
                    st.period_totals_table(), hf, hw, (st.period_totals_overflow(), st.period_totals_outside()))
        finally:
            st.close()

    diag, wtd, anc, beta, table, hf, hw, counts = run(FLOOR)
    anc1 = run(0.0)[2]
    assert beta < 1.0 and not np.array_equal(anc, anc1)                              # the tempered ancestry is another one
    want = period_totals_of(diag, wtd, forcing.wtd_obs, ends, thr, 32, fexp, ancestors={48: anc}, D=cols.dim_d)
    assert _same(table, want["table"]) and _same(hf[0], want["hist_flux"]) and _same(hw[0], want["hist_wtd"])
    assert counts == (0, 0) and want["overflow"] == 0 and want["outside"] == 0
    other = period_totals_of(diag, wtd, forcing.wtd_obs, ends, thr, 32, fexp, ancestors={48: anc1}, D=cols.dim_d)
    assert not _same(other["table"], want["table"])


# ---- 5. the CLI ----------------------------------------------------------------------------------------------------------
TEMPER_KEYS = {"filter_ess_floor", "filter_beta", "filter_ess_tempered", "filter_ess_target"}


def test_cli_key_adds_the_datasets_and_the_closing_line(tmp_path, monkeypatch, capsys):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    params = _cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    files, logs = {}, {}
    pts = [{"Soil_Properties": {"n": 1.6}}, {"Soil_Properties": {"n": 2.4}}]
    base = {"Stride": 24, "Sigma_cm": 2.0}
    for tag, extra in (("plain", {"Filter": base}),
                       ("ens", {"Filter": {**base, "ESS_floor": 0.5}}),
                       ("sweep", {"Points": pts, "Filter": {**base, "ESS_floor": 0.25}})):
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 64, "Seed": 3, "Days": 2, **extra}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = loadResults(tmp_path / f"Run_{tag}_ensemble.h5")
        logs[tag] = capsys.readouterr().out
    plain, ens, sweep = files["plain"], files["ens"], files["sweep"]
    assert "tempering" not in logs["plain"] and not TEMPER_KEYS & set(plain)
    assert set(ens) - set(plain) == TEMPER_KEYS and TEMPER_KEYS <= set(sweep)
    assert ens["filter_rows"].tolist() == [24, 48, 72, 96] and float(ens["filter_ess_floor"]) == 0.5
    for key in TEMPER_KEYS - {"filter_ess_floor"}:
        assert ens[key].shape == (4,) and sweep[key].shape == (2, 4), key
    for key in ("filter_rows", "filter_count"):
        assert _same(ens[key], plain[key]), key
    assert _same(ens["filter_ess"][0], plain["filter_ess"][0]) and _same(ens["filter_loglik_rows"][0], plain["filter_loglik_rows"][0])
    assert np.all(ens["filter_ess_target"] == 32) and np.all(sweep["filter_ess_target"] == 16)
    assert np.all(ens["filter_ess_tempered"] >= ens["filter_ess_target"])
    met = ens["filter_beta"] == 1.0
    assert _same(ens["filter_ess_tempered"][met], ens["filter_ess"][met])
    for tag, label, data in (("ens", "Ensemble x64", ens), ("sweep", "Sweep 2 points x64", sweep)):
        line = re.search(rf"\[{label}\] filter tempering: (\d+) of 4 rows tempered, smallest beta = ([0-9.e+-]+)", logs[tag])
        beta = np.asarray(data["filter_beta"]).reshape(-1, 4)
        assert line, logs[tag]
        assert int(line.group(1)) == int((beta < 1.0).any(axis=0).sum())
        assert abs(float(line.group(2)) - beta.min()) <= 1e-5
        assert logs[tag].index("filter log-likelihood") < logs[tag].index("filter tempering")


# ---- 6. refusals and what turns it off -----------------------------------------------------------------------------------
def test_refusals_and_what_removes_the_tempering():
    from hydromodel_amd._lib import HcError
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(WELL)
    st = EnsembleStepper(cols, forcing, 64)
    try:
        st.set_state(np.array(_initial(64)))
        st.set_noise_philox(SEED, 0)
        with pytest.raises(HcError, match="the particle filter is off"):
            st.set_filter_tempering(0.5)
        st.set_filter_tempering(0.0)                                # off stays off without a filter
        st.set_filter(STRIDE, 5.0, 1)
        with pytest.raises(HcError, match="not tempered"):
            st.filter_temper_table()
        for bad in (1.0, -0.5, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="must be 0 .off. or finite with 0 < f < 1"):
                st.set_filter_tempering(bad)
        lib_refuses = st.lib.hc_set_filter_tempering(st.h, 1.0)
        assert lib_refuses != 0 and b"must be 0 (off) or finite with 0 < f < 1" in st.lib.hc_last_error()
        st.set_filter_tempering(0.5)
        assert st.filter_ess_floor == 0.5 and np.isnan(st.filter_temper_table()).all()
        assert st.filter_temper_table().shape == (1, (st.T - 1) // STRIDE + 1, 4)
        with pytest.raises(HcError, match="no assimilation since hc_set_filter"):
            st.filter_temper_trials()
        st.set_filter(STRIDE, 5.0, 1)                               # hc_set_filter removes it, as it removes a record
        assert st.filter_ess_floor == 0.0
        with pytest.raises(HcError, match="not tempered"):
            st.filter_temper_table()
        st.set_filter_tempering(0.5)
        st.set_filter_tempering(0.0)
        with pytest.raises(HcError, match="not tempered"):
            st.filter_temper_trials()
    finally:
        st.close()
