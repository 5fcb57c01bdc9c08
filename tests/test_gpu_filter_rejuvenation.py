"""Rejuvenation of the particle filter's base noise vectors on the GPU (include/hydrocol.h hc_set_filter_rejuvenation):
the moved vectors, the moments and the table against the NumPy restatement fed with the twin's resampled vectors and the
hooked normals; the normals against a Philox written with Python integers; flat weights against the run without the key,
stepper and written file; the same bits at another launch length, in another point order, with the points on handles of
their own and across a checkpoint; the distinct fields of a ten-day run; the CLI's key; the refusals."""
import json
import re
from functools import lru_cache

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the sharded refusal's buffer is torch's)

from helpers import digest, golden
from helpers import cli_params as _cli_params
from test_gpu_enkf import _spread

pytestmark = pytest.mark.gpu
STRIDE, SEED, FSEED, SPREAD_SEED = 48, 7, 11, 12
SIGMA_DZ = 0.5                  # the well's error as a fraction of dz: sharp, as in test_gpu_filter_temper.py
DELTA = 0.95
NODES = [6, 45]                 # 30 cm and 225 cm, as in test_gpu_filter_sm.py
VALUES = [0.24, 0.36]
SIGMAS = np.array([0.05, 0.08])
OFFSETS = (12, 24, 36)
PERIODS = ([72, 96], [], 32, [12, 12])


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _initial(N, well):
    psi = _spread(golden(f"g1_tables_{well}.npz")["initial_cond"], N, seed=SPREAD_SEED)
    psi.setflags(write=False)
    return psi


def _variance_bar(delta, N):
    """six standard deviations of var' / s^2 - 1 (tests/test_filter_rejuvenation_cpu.py)"""
    from hydromodel_amd.stepper import rejuvenation_shrinkage
    a, h = rejuvenation_shrinkage(delta)
    return 6.0 * np.sqrt((2.0 * h ** 4 + 4.0 * a * a * h * h) / N)


@lru_cache(maxsize=None)
def _run(well, P, mpp, delta, noise="philox", rows=(48,), rpl=0, point=None, sigma_dz=SIGMA_DZ, extras=False):
    """One handle stepped through the assimilations at ``rows``: the hooks after each of them and the tables at the end.
    ``point``: the handle holds that point of the P alone.  ``extras``: sensors, a window, an ESS floor and period totals
    on.  Computed once per setting, shared and left unchanged."""
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
        if extras:
            v = np.full((st.T, len(VALUES)), np.nan)
            v[list(rows)] = VALUES
            st.set_filter_soil_moisture(NODES, v, SIGMAS)
            st.set_filter_tempering(0.5)
            st.set_filter_window(OFFSETS)
            st.set_period_totals(*PERIODS)
        if delta:
            st.set_filter_rejuvenation(delta)
        at = 1

        def fresh(r0, n):
            if not host:
                return {}
            f = np.random.default_rng(1000 + r0).standard_normal((st.n_refresh(r0, n), P * mpp, st.D))
            return {"fresh_noise": np.ascontiguousarray(f[:, lo:lo + N])}

        def base():
            return st.get_noise_base() if host else st.filter_base()

        for row in rows:
            assert int(forcing.wtd_obs[row]) >= 0
            st.step_rows(at, row + 1 - at, **fresh(at, row + 1 - at))
            h = dict(row=row, anc=st.filter_ancestors(), psi=st.get_state(), base=base(),
                     eps=st.filter_rejuvenation_normals(row))
            if delta:
                h["mom"] = st.filter_rejuvenation_moments()
            hooks.append(h)
            at = row + 1
        res = dict(hooks=hooks, table=st.filter_table(), psi=st.get_state(), moments=np.asarray(st.moments()), cols=cols,
                   base=base())
        if extras:
            res["ptable"] = st.period_totals_table()
            res["ttable"] = st.filter_temper_table()
        if delta:
            res["rtable"] = st.filter_rejuvenation_table()
            res["shrinkage"] = st.filter_rejuvenation_shrinkage()
        return res
    finally:
        st.close()


# ---- 1. against the restatement -----------------------------------------------------------------------------------------
CASES = [(1, 1, 100, "numpy", False), (1, 3, 2500, "philox", False), (300, 1, 2500, "numpy", False),
         (300, 3, 100, "philox", False), (1, 2, 100, "philox", True)]


@pytest.mark.parametrize("well, P, mpp, noise, extras", CASES)
def test_the_move_the_moments_and_the_table_are_the_restatements(well, P, mpp, noise, extras):
    """2 500 members: ten tiles of the spread passes, the last one partial.  The twin without the key supplies the
    resampled vectors; its psi, ancestry and table are this run's bits, because the move touches the base vectors only
    and nothing is stepped after the assimilation."""
    from hydromodel_amd.stepper import filter_rejuvenation_of, rejuvenation_shrinkage
    got = _run(well, P, mpp, DELTA, noise, extras=extras)
    twin = _run(well, P, mpp, 0.0, noise, extras=extras)
    h, h1 = got["hooks"][0], twin["hooks"][0]
    D = got["cols"].dim_d
    assert D == {1: 101, 300: 300}[well]
    assert _same(h["psi"], h1["psi"]) and _same(h["anc"], h1["anc"]) and _same(got["table"], twin["table"])
    assert _same(got["moments"], twin["moments"]) and _same(h["eps"], h1["eps"])     # the normals are stateless
    if extras:
        assert _same(got["ptable"], twin["ptable"]) and _same(got["ttable"], twin["ttable"])
    assert not np.array_equal(h["anc"], np.arange(P * mpp))
    assert got["shrinkage"] == (DELTA, rejuvenation_shrinkage(DELTA)[0])
    eps, z = h["eps"], h1["base"]
    assert abs(eps.mean()) < 6.0 / np.sqrt(eps.size) and abs(eps.std() - 1.0) < 6.0 / np.sqrt(2.0 * eps.size)
    assert np.unique(eps.reshape(-1)).size == eps.size
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        survivors = int(got["table"][p, 1, 3])
        assert 0 < survivors < mpp and survivors == np.unique(h["anc"][sl]).size
        want = filter_rejuvenation_of(z[sl], eps[sl], DELTA, survivors=survivors)
        assert want["applied"] and not want["refused"].any()
        zerr = np.abs(h["base"][sl] - want["z"]) / np.maximum(1.0, np.abs(want["z"]))
        merr = max(np.abs(h["mom"][p, 0] - want["mean"]).max(), np.abs(h["mom"][p, 1] - want["s"]).max(),
                   np.abs(h["mom"][p, 2] - want["s_after"]).max())
        row = got["rtable"][p, 1]
        terr = np.abs(row - want["row"]).max()
        print(f"\n well {well} P={P} N_p={mpp} {noise} point {p}: survivors {survivors}, max z error {zerr.max():.2e}, "
              f"moments {merr:.2e}, table {terr:.2e}, spread {row[2]:.6f} -> {row[3]:.6f}")
        assert zerr.max() <= 1e-9 and merr <= 1e-10 and terr <= 1e-10
        assert row[0] == 1.0 and row[1] == 0.0
        assert not (h["base"][sl] == z[sl]).all(axis=1).any()                        # every member's vector moved
        assert np.unique(h["base"][sl], axis=0).shape[0] == mpp
        assert abs(row[3] / row[2] - 1.0) <= _variance_bar(DELTA, mpp)
    assert np.isnan(got["rtable"][:, 0]).all() and np.isnan(got["rtable"][:, 2:]).all()


def _normal_restated(seed, gid, row, d):
    """eps of global member ``gid`` at node d with Python's integers: counter (0x80000000 | d >> 1, row, gid_lo, gid_hi)
    under the filter's seed, Box-Muller as the noise's normals: the cosine for even d, the sine for odd d."""
    from test_gpu_enkf import M32, _philox
    r = _philox((0x80000000 | (d >> 1), row, gid & M32, gid >> 32), (seed & M32, seed >> 32))
    a, b = (r[1] << 32) | r[0], (r[3] << 32) | r[2]
    u1 = ((a >> 11) + 0.5) / 9007199254740992.0
    u2 = ((b >> 11) + 0.5) / 9007199254740992.0
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * (np.sin(2.0 * np.pi * u2) if d & 1 else np.cos(2.0 * np.pi * u2))


def test_the_normals_are_the_documented_philox_stream():
    """The hook -- the update kernel's own device function -- against a Philox written with Python integers: a sweep handle
    whose points' member bases are not contiguous, before any step (hc_set_filter uploaded the keys), and a single point
    with a member offset past 2^32.  |eps| < 9 and libm's log, sin and cos are good to a few ulp: 1e-12 absolute."""
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(1)
    D, mpp, seed = cols.dim_d, 70, (0xABCDEF01 << 32) | 0x2345
    spots = [(0, 0), (0, 1), (3, 2), (3, 3), (69, 100), (69, 99), (17, 50)]         # (member of the point, node)
    st = EnsembleStepper([cols] * 3, forcing, 3 * mpp)
    try:
        st.set_state(np.array(_initial(3 * mpp, 1)))
        st.set_noise_philox(SEED, 0)
        bases = [5 * mpp, 2 * mpp, (1 << 33) + 7]
        st.set_point_member_bases(np.array(bases, dtype=np.int64))
        st.set_filter(STRIDE, 5.0, seed)
        for row in (48, 4800):
            eps = st.filter_rejuvenation_normals(row).reshape(3, mpp, D)
            assert _same(eps[1, 10:20], st.filter_rejuvenation_normals(row, mpp + 10, 10))
            for p, base in enumerate(bases):
                for j, d in spots:
                    assert abs(eps[p, j, d] - _normal_restated(seed, base + j, row, d)) <= 1e-12, (row, p, j, d)
    finally:
        st.close()
    st = EnsembleStepper(cols, forcing, mpp)
    try:
        st.set_state(np.array(_initial(mpp, 1)))
        st.set_noise_philox(SEED, (1 << 32) + 11)
        st.set_filter(STRIDE, 5.0, 3)
        eps = st.filter_rejuvenation_normals(96)
        for j, d in spots:
            assert abs(eps[j, d] - _normal_restated(3, (1 << 32) + 11 + j, 96, d)) <= 1e-12, (j, d)
    finally:
        st.close()


# ---- 2. flat weights ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["philox", "numpy"])
def test_flat_weights_leave_every_bit_of_the_run_without_the_key(noise):
    got = _run(1, 2, 100, DELTA, noise, rows=(48, 96), sigma_dz=1e30)
    twin = _run(1, 2, 100, 0.0, noise, rows=(48, 96), sigma_dz=1e30)
    for key in ("psi", "base", "table", "moments"):
        assert _same(got[key], twin[key]), key
    for h, h1 in zip(got["hooks"], twin["hooks"]):
        assert np.array_equal(h["anc"], np.arange(200)) and _same(h["base"], h1["base"]) and _same(h["psi"], h1["psi"])
    for slot in (1, 2):
        assert got["rtable"][:, slot, :2].tolist() == [[0.0, 0.0]] * 2 and np.isnan(got["rtable"][:, slot, 2:]).all()


def test_flat_weights_write_the_file_of_the_run_without_the_key(tmp_path, monkeypatch, capsys):
    """The CLI at sigma = 1e30, an ensemble and a sweep, with profile statistics and the distribution on: every array of
    the file without the key is in the file with it, to the bit; the key's own arrays say that nothing was moved."""
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    params = _cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    pts = [{"Soil_Properties": {"n": 1.6}}, {"Soil_Properties": {"n": 2.4}}]
    flat = {"Stride": 24, "Sigma_cm": 1e30}
    for kind, extra in (("ens", {}), ("sweep", {"Points": pts})):
        files = {}
        for tag, filt in (("off", flat), ("on", {**flat, "Rejuvenation": 0.95})):
            params["Output_Name"] = f"Run_{kind}_{tag}"
            params["Ensemble"] = {"Members": 64, "Seed": 3, "Days": 2, "Profiles": 48,
                                  "Distribution": {"Stride": 48}, "Filter": filt, **extra}
            (tmp_path / f"{kind}_{tag}.json").write_text(json.dumps(params))
            cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{kind}_{tag}.json")])
            files[tag] = loadResults(tmp_path / f"Run_{kind}_{tag}_ensemble.h5")
            capsys.readouterr()
        off, on = files["off"], files["on"]
        assert set(on) - set(off) == REJUV_KEYS and {"moments", "wtd_hist", "filter_survivors"} <= set(off)
        for key in sorted(off):
            assert _same(off[key], on[key]), (kind, key)
        assert np.all(np.asarray(off["filter_survivors"]) == 64)
        assert not np.asarray(on["filter_rejuvenated"]).any() and not np.asarray(on["filter_rejuvenation_refused"]).any()
        assert np.isnan(on["filter_noise_std_resampled"]).all() and np.isnan(on["filter_noise_std_rejuvenated"]).all()


# ---- 3. the same bits ---------------------------------------------------------------------------------------------------
def test_launch_length_and_the_dealing_of_points_do_not_change_a_bit():
    well, P, mpp, rows = 1, 2, 2500, (48, 96)
    whole = _run(well, P, mpp, DELTA, rows=rows)
    assert np.all(whole["rtable"][:, 1, 0] == 1.0)
    short = _run(well, P, mpp, DELTA, rows=rows, rpl=7)
    for key in ("psi", "base", "table", "rtable", "moments"):
        assert _same(whole[key], short[key]), key
    for a, b in zip(whole["hooks"], short["hooks"]):
        for key in ("anc", "base", "mom", "eps"):
            assert _same(a[key], b[key]), (a["row"], key)
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        part = _run(well, P, mpp, DELTA, rows=rows, point=p)
        assert _same(part["psi"], whole["psi"][sl]) and _same(part["base"], whole["base"][sl])
        assert _same(part["table"][0], whole["table"][p]) and _same(part["rtable"][0], whole["rtable"][p])
        for a, b in zip(part["hooks"], whole["hooks"]):
            assert _same(a["eps"], b["eps"][sl]) and _same(a["mom"][0], b["mom"][p]) and _same(a["base"], b["base"][sl])


SWEEP_N = (1.8, 2.4, 1.6, 2.1)          # van Genuchten n of the sweep's points, not monotone: the cost-sorted walk moves
SWEEP_MPP, SWEEP_ROWS = 100, (48, 96)


def _sweep_handle(ids, psi_all, rows_per_launch=0):
    """The handle that runs the sweep points ``ids`` (global member ids point-major, each point keyed by its first global
    member), rejuvenated, through the assimilations at rows 48 and 96: the hooks after each and the results per point."""
    from hydromodel_amd.stepper import EnsembleStepper
    from test_gpu_filter_window import _point_like
    pts = [_point_like(SWEEP_N[k]) for k in ids]
    n = len(ids)
    st = EnsembleStepper([c for _, c, _ in pts], pts[0][2], n * SWEEP_MPP)
    try:
        st.set_generic_exponents(True)
        st.set_state(np.concatenate([psi_all[k * SWEEP_MPP:(k + 1) * SWEEP_MPP] for k in ids]))
        st.set_noise_philox(21, ids[0] * SWEEP_MPP)
        if n > 1:
            st.set_point_member_bases(np.array(ids, dtype=np.int64) * SWEEP_MPP)
        st.set_rows_per_launch(rows_per_launch)
        st.set_filter(STRIDE, SIGMA_DZ * st.cols.dz, 8)
        st.set_filter_rejuvenation(DELTA)
        out, at = {}, 1
        for row in SWEEP_ROWS:
            st.step_rows(at, row + 1 - at)
            out[f"anc{row}"] = st.filter_ancestors().reshape(n, SWEEP_MPP) - (np.arange(n) * SWEEP_MPP)[:, None]
            out[f"mom{row}"] = st.filter_rejuvenation_moments()
            out[f"eps{row}"] = st.filter_rejuvenation_normals(row).reshape(n, SWEEP_MPP, -1)
            out[f"base{row}"] = st.filter_base().reshape(n, SWEEP_MPP, -1)
            at = row + 1
        out.update(psi=st.get_state().reshape(n, SWEEP_MPP, -1), table=st.filter_table(),
                   rtable=st.filter_rejuvenation_table(), moments=np.asarray(st.moments()).reshape(n, 3, -1),
                   base=st.filter_base().reshape(n, SWEEP_MPP, -1), costs=st.point_costs())
        return out
    finally:
        st.close()


def test_point_order_launch_length_and_the_dealing_of_unequal_points_do_not_change_a_bit(monkeypatch):
    """Four points of unequal cost: the default walk sorts them by cost after the first launch, HYDROCOL_POINT_ORDER=fixed
    keeps the point order; then what two ranks of the sweep run, each with two points whose ids are not contiguous."""
    psi_all = _spread(golden("g1_tables_1.npz")["initial_cond"], 4 * SWEEP_MPP, seed=4)
    everyone = list(range(4))
    monkeypatch.delenv("HYDROCOL_POINT_ORDER", raising=False)
    whole = _sweep_handle(everyone, psi_all)
    costs = whole.pop("costs")
    walk = list(np.argsort(-costs.astype(np.int64), kind="stable"))      # the library's: descending cost, ties in point order
    print(f"\n RHS evaluations per point {costs.tolist()}: the cost-sorted walk is {walk}")
    assert walk != everyone                                             # a condition of the input: the sorted walk is another one
    assert np.all(whole["rtable"][:, 1, 0] == 1.0) and np.isfinite(whole["rtable"][:, 1]).all()              # row 48 moved every point
    others = [_sweep_handle(everyone, psi_all, 7)]
    monkeypatch.setenv("HYDROCOL_POINT_ORDER", "fixed")
    others += [_sweep_handle(everyone, psi_all), _sweep_handle(everyone, psi_all, 7)]
    monkeypatch.delenv("HYDROCOL_POINT_ORDER", raising=False)
    for other in others:
        other.pop("costs")
        for k in whole:
            assert _same(whole[k], other[k]), k
    for ids in ([0, 2], [1, 3]):
        part = _sweep_handle(ids, psi_all)
        part.pop("costs")
        for j, k in enumerate(ids):
            for key in whole:
                assert whole[key][k].tobytes() == part[key][j].tobytes(), (ids, k, key)


def test_dump_and_restore_continue_a_rejuvenated_run_bit_for_bit(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(1)
    kw = dict(seed=6, psi0=np.array(_initial(300, 1)), filter_stride=STRIDE, filter_sigma_cm=SIGMA_DZ * cols.dz,
              filter_rejuvenation=DELTA)

    def state(sim):
        return [sim.stepper.get_state(), sim.filter_table(), sim.filter_rejuvenation_table(), sim.moments(),
                sim.stepper.filter_base()]

    whole = EnsembleSimulation(cols, forcing, 300, **kw)
    try:
        whole.advance(60)                                           # between the assimilations at rows 48 and 96
        path = whole.dump(tmp_path / "ck.h5")
        whole.advance(48)
        want, summary = state(whole), whole.filter_summary()
    finally:
        whole.close()
    back = EnsembleSimulation.restore(path, cols, forcing)
    try:
        assert back.next_row == 61 and back.filter_rejuvenation == DELTA and back.stepper.filter_rejuvenation == DELTA
        assert _same(back.filter_rejuvenation_table()[1], want[2][1])
        back.advance(48)
        got = state(back)
    finally:
        back.close()
    for a, b in zip(want, got):
        assert _same(a, b)
    # row 96, the first assimilation after the restore, moved the vectors too: the restored discount was at work
    assert summary["rows"].tolist() == [48, 96] and summary["rejuvenated"].tolist() == [1, 1]
    assert summary["rejuvenated_rows"] == 2 and np.isfinite(summary["noise_std_rejuvenated"]).all()
    assert summary["rejuvenation_refused"].tolist() == [0, 0]


# ---- 4. diversity -------------------------------------------------------------------------------------------------------
def test_the_fields_stay_distinct_over_ten_days():
    """Without the key the distinct base vectors of a point only ever get fewer; with it every row that was rejuvenated
    from at least two survivors ends with N_p of them (a single survivor has s = 0: the documented limit)."""
    N, days = 256, 10
    rows = tuple(48 * d for d in range(1, days + 1))
    plain, got = _run(1, 1, N, 0.0, rows=rows), _run(1, 1, N, DELTA, rows=rows)
    counts = [np.unique(h["base"], axis=0).shape[0] for h in plain["hooks"]]
    print(f"\n distinct base vectors without the key: {counts}")
    assert counts[-1] < N and all(b <= a for a, b in zip([N] + counts, counts))
    rt, surv = got["rtable"][0], got["table"][0, :, 3]
    moved = [np.unique(h["base"], axis=0).shape[0] for h in got["hooks"]]
    print(f" with it: {moved}; survivors {surv[1:days + 1].astype(int).tolist()}; "
          f"spread kept {(rt[1:days + 1, 3] / rt[1:days + 1, 2]).round(4).tolist()}")
    proper = 0
    for d, h in enumerate(got["hooks"], start=1):
        applied = rt[d, 0] == 1.0
        assert applied == (0 < surv[d] < N)
        if applied and surv[d] >= 2:
            proper += 1
            assert moved[d - 1] == N and rt[d, 1] == 0.0
            assert abs(rt[d, 3] / rt[d, 2] - 1.0) <= _variance_bar(DELTA, N)
    assert proper >= 1


# ---- 5. the CLI ---------------------------------------------------------------------------------------------------------
REJUV_KEYS = {"filter_rejuvenation_discount", "filter_rejuvenation_shrinkage", "filter_rejuvenated",
              "filter_rejuvenation_refused", "filter_noise_std_resampled", "filter_noise_std_rejuvenated"}


def test_cli_key_adds_the_datasets_and_the_closing_line(tmp_path, monkeypatch, capsys):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    from hydromodel_amd.stepper import rejuvenation_shrinkage
    params = _cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    files, logs = {}, {}
    pts = [{"Soil_Properties": {"n": 1.6}}, {"Soil_Properties": {"n": 2.4}}]
    base = {"Stride": 24, "Sigma_cm": 2.0}
    for tag, extra in (("plain", {"Filter": base}),
                       ("ens", {"Filter": {**base, "Rejuvenation": 0.95}}),
                       ("sweep", {"Points": pts, "Filter": {**base, "Rejuvenation": 0.75}})):
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 64, "Seed": 3, "Days": 2, **extra}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = loadResults(tmp_path / f"Run_{tag}_ensemble.h5")
        logs[tag] = capsys.readouterr().out
    plain, ens, sweep = files["plain"], files["ens"], files["sweep"]
    assert "rejuvenation" not in logs["plain"] and not REJUV_KEYS & set(plain)
    assert set(ens) - set(plain) == REJUV_KEYS and REJUV_KEYS <= set(sweep)
    assert ens["filter_rows"].tolist() == [24, 48, 72, 96]
    assert float(ens["filter_rejuvenation_discount"]) == 0.95 and float(sweep["filter_rejuvenation_discount"]) == 0.75
    assert float(ens["filter_rejuvenation_shrinkage"]) == rejuvenation_shrinkage(0.95)[0]
    for key in REJUV_KEYS - {"filter_rejuvenation_discount", "filter_rejuvenation_shrinkage"}:
        assert ens[key].shape == (4,) and sweep[key].shape == (2, 4), key
    assert _same(ens["filter_rows"], plain["filter_rows"]) and _same(ens["filter_count"], plain["filter_count"])
    assert _same(ens["filter_ess"][0], plain["filter_ess"][0])       # one forecast up to the first assimilation
    for tag, label, data in (("ens", "Ensemble x64", ens), ("sweep", "Sweep 2 points x64", sweep)):
        moved = np.asarray(data["filter_rejuvenated"]).reshape(-1, 4) > 0
        surv = np.asarray(data["filter_survivors"]).reshape(-1, 4)
        assert np.array_equal(moved, (surv > 0) & (surv < 64))
        before = np.asarray(data["filter_noise_std_resampled"]).reshape(-1, 4)
        after = np.asarray(data["filter_noise_std_rejuvenated"]).reshape(-1, 4)
        assert np.isfinite(before[moved]).all() and np.isnan(before[~moved]).all() and np.isnan(after[~moved]).all()
        line = re.search(rf"\[{label}\] filter rejuvenation: (\d+) of 4 rows, noise-field spread kept ([0-9.naN]+) of "
                         rf"resampled", logs[tag])
        assert line, logs[tag]
        assert int(line.group(1)) == int(moved.any(axis=0).sum())
        ok = moved & (before > 0)               # (members that start from one profile may keep their bin: no row moved)
        if ok.any():
            assert abs(float(line.group(2)) - float((after[ok] / before[ok]).mean())) <= 1e-4
        else:
            assert line.group(2) == "nan"
        assert logs[tag].index("filter log-likelihood") < logs[tag].index("filter rejuvenation")


# ---- 6. refusals and what turns it off ----------------------------------------------------------------------------------
def test_refusals_and_what_removes_the_rejuvenation():
    from hydromodel_amd._lib import HcError
    from hydromodel_amd.ensemble import EnsembleSimulation
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(1)
    st = EnsembleStepper(cols, forcing, 64)
    try:
        st.set_state(np.array(_initial(64, 1)))
        st.set_noise_philox(SEED, 0)
        with pytest.raises(HcError, match="the particle filter is off"):
            st.set_filter_rejuvenation(0.9)
        st.set_filter_rejuvenation(0.0)                             # off stays off without a filter
        st.set_filter(STRIDE, 5.0, 1)
        with pytest.raises(HcError, match="not rejuvenated"):
            st.filter_rejuvenation_table()
        for bad in (1.0, 0.49, -0.5, float("nan"), float("inf"), True):
            with pytest.raises(ValueError, match="filter rejuvenation = .* must be"):
                st.set_filter_rejuvenation(bad)
        for bad in (1.0, 0.49, float("nan")):
            assert st.lib.hc_set_filter_rejuvenation(st.h, bad) != 0
            assert b"must be 0 (off) or finite with 0.5 <= discount < 1" in st.lib.hc_last_error()
        assert st.filter_rejuvenation_shrinkage() == (0.0, 0.0)
        st.set_filter_rejuvenation(0.9)
        assert st.filter_rejuvenation == 0.9 and np.isnan(st.filter_rejuvenation_table()).all()
        assert st.filter_rejuvenation_table().shape == (1, (st.T - 1) // STRIDE + 1, 4)
        with pytest.raises(HcError, match="no assimilation since"):
            st.filter_rejuvenation_moments()
        assert st.filter_rejuvenation_normals(48, 3, 5).shape == (5, cols.dim_d)
        with pytest.raises(HcError, match="bad argument"):
            st.filter_rejuvenation_normals(48, 60, 5)
        # a sharded single point: each of the two refuses while the other is set, and names both
        with pytest.raises(HcError, match=r"hc_set_filter_shard: the base vectors are rejuvenated \(hc_set_filter_rejuvenation\)"):
            st.set_filter_shard([0, 64], 0, None)
        st.set_filter(STRIDE, 5.0, 1)                               # hc_set_filter removes it, as it removes a record
        assert st.filter_rejuvenation == 0.0 and st.filter_rejuvenation_shrinkage() == (0.0, 0.0)
        with pytest.raises(HcError, match="not rejuvenated"):
            st.filter_rejuvenation_table()
        st.set_filter_shard([0, 64], 0, None)
        with pytest.raises(ValueError, match="sharded"):
            st.set_filter_rejuvenation(0.9)
        assert st.lib.hc_set_filter_rejuvenation(st.h, 0.9) != 0
        err = st.lib.hc_last_error()
        assert b"hc_set_filter_rejuvenation" in err and b"hc_set_filter_shard" in err
        st.set_filter_shard(None)
        st.set_filter_rejuvenation(0.9)
        st.set_filter_rejuvenation(0.0)
        with pytest.raises(HcError, match="not rejuvenated"):
            st.filter_rejuvenation_moments()
    finally:
        st.close()
    with pytest.raises(ValueError, match="filter_shard and filter_rejuvenation exclude each other"):
        EnsembleSimulation(cols, forcing, 64, filter_stride=STRIDE, filter_sigma_cm=5.0, filter_rejuvenation=0.9,
                           filter_shard=([0, 64], 0, None))
    with pytest.raises(ValueError, match="filter_rejuvenation needs the particle filter"):
        EnsembleSimulation(cols, forcing, 64, filter_rejuvenation=0.9)
