"""Correlated noise fields on the GPU (include/hydrocol.h hc_set_noise_correlation): the fill kernel against the NumPy
restatement of the recursion, to the bit, at every edge of its tiling; a correlated Philox run as the host-noise run of
the same vectors; the neutral table; shards; the filters on top of it; the field's statistics; checkpoint and CLI.
70 members: one full tile of 64 and a partial one."""
import json

import numpy as np
import pytest

from helpers import WELLS, digest, golden
from helpers import run_cli_ranks as _run_ranks

pytestmark = pytest.mark.gpu
N70 = 70


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _spread(psi0, N, seed=12, width=60.0):
    return np.asarray(psi0)[None, :] + np.random.default_rng(seed).uniform(-width, width, size=N)[:, None]


def _tables(cols, length=50.0, layers=True):
    from hydromodel_amd.stepper import noise_correlation_breaks, noise_correlation_tables
    return noise_correlation_tables(cols.z, length, noise_correlation_breaks(cols.layers, cols.z) if layers else ())


def _stepper(well, N, seed=7, offset=0, spread=False, psi=None):
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(well)
    st = EnsembleStepper(cols, forcing, N)
    psi0 = golden(f"g1_tables_{well}.npz")["initial_cond"]
    st.set_state(psi if psi is not None else _spread(psi0, N) if spread else psi0)
    st.set_noise_philox(seed, offset)
    return st, cols, forcing


# ---- 1. the hook and the base vectors against the restatement
@pytest.mark.parametrize("well, N, offset", [(1, N70, 0), (200, N70, 0), (581, N70, 0), (200, N70, 1000), (200, 1, 0)])
def test_hook_and_base_are_the_restatement_of_the_philox_normals(well, N, offset):
    from hydromodel_amd.stepper import noise_correlate
    st, cols, _ = _stepper(well, N, offset=offset)
    try:
        a, b = _tables(cols)
        if well == 1:
            assert np.flatnonzero(a == 0.0).tolist() == [0, int(np.flatnonzero(cols.z >= 50.0)[0]),
                                                         int(np.flatnonzero(cols.z >= 200.0)[0])]
        assert st.noise_correlation() is None
        white = st.noise_field_normals(offset, 1)
        assert _same(white, st.philox_normals(offset, 1))            # off: the hook is hc_philox_normals
        st.set_noise_correlation(a, b)
        on = st.noise_correlation()
        assert on is not None and _same(on[0], a[None]) and _same(on[1], b[None])
        for m in sorted({0, min(63, N - 1), min(64, N - 1), N - 1}):
            for k in (0, 1, 5):
                xi = st.philox_normals(offset + m, k)
                assert _same(st.noise_field_normals(offset + m, k), noise_correlate(xi, a, b)), (m, k)
        assert not _same(st.noise_field_normals(offset, 1), white)
        base = st.noise_field_base()
        want = noise_correlate(np.stack([st.philox_normals(offset + m, 0) for m in range(N)]), a, b)
        assert _same(base, want)
    finally:
        st.close()


def test_three_points_keyed_out_of_order_take_their_own_tables():
    from hydromodel_amd.stepper import EnsembleStepper, noise_correlate
    _, cols, forcing = digest(200)
    P, mpp, bases = 3, N70, np.array([140, 0, 70], dtype=np.int64)
    st = EnsembleStepper([cols] * P, forcing, P * mpp)
    try:
        st.set_state(golden("g1_tables_200.npz")["initial_cond"])
        st.set_noise_philox(9, 0)
        st.set_point_member_bases(bases)
        ab = [_tables(cols, length) for length in (25.0, 50.0, 100.0)]
        a, b = np.stack([t[0] for t in ab]), np.stack([t[1] for t in ab])
        st.set_noise_correlation(a, b)
        base = st.noise_field_base().reshape(P, mpp, -1)
        for p in range(P):
            xi = np.stack([st.philox_normals(int(bases[p]) + j, 0) for j in range(mpp)])
            assert _same(base[p], noise_correlate(xi, a[p], b[p])), p
            for j, k in ((0, 1), (63, 5), (64, 1), (69, 5)):
                got = st.noise_field_normals(int(bases[p]) + j, k)
                assert _same(got, noise_correlate(st.philox_normals(int(bases[p]) + j, k), a[p], b[p])), (p, j, k)
        st.set_point_member_bases(bases[::-1].copy())                # new keys: the correlation is off with the filters
        assert st.noise_correlation() is None
    finally:
        st.close()


# ---- 2. a correlated run is the host-noise run of the same vectors, at any launch length
def _corr_run(rows_per_launch, monkeypatch, well=300, rows=150, seed=5):
    if rows_per_launch:
        monkeypatch.setenv("HYDROCOL_ROWS_PER_LAUNCH", str(rows_per_launch))
    else:
        monkeypatch.delenv("HYDROCOL_ROWS_PER_LAUNCH", raising=False)
    st, cols, _ = _stepper(well, N70, seed=seed)
    try:
        st.set_wtd_hist(48)
        st.set_noise_correlation(*_tables(cols))
        st.step_rows(1, rows)
        return st.get_state(), st.moments(), st.wtd_hist_table()
    finally:
        st.close()
        monkeypatch.delenv("HYDROCOL_ROWS_PER_LAUNCH", raising=False)


def test_a_correlated_run_is_the_host_noise_run_of_the_same_vectors(monkeypatch):
    from hydromodel_amd.stepper import noise_correlate
    rows, seed = 150, 5
    got = _corr_run(0, monkeypatch, rows=rows, seed=seed)
    short = _corr_run(7, monkeypatch, rows=rows, seed=seed)
    ref, cols, forcing = _stepper(300, N70, seed=seed)
    try:
        a, b = _tables(cols)
        live = forcing.refresh.astype(bool) & (forcing.wtd_obs >= 0)
        draw = np.cumsum(live)
        normals = lambda k: np.stack([ref.philox_normals(m, k) for m in range(N70)])   # noqa: E731
        base = noise_correlate(normals(0), a, b)
        fresh = np.stack([noise_correlate(normals(int(draw[row])), a, b) for row in range(1, rows + 1) if live[row]])
        assert fresh.shape[0] >= 3
        ref.set_noise_host(base)
        ref.set_wtd_hist(48)
        ref.step_rows(1, rows, fresh_noise=fresh)
        want = (ref.get_state(), ref.moments(), ref.wtd_hist_table())
    finally:
        ref.close()
    for x, y, z in zip(got, want, short):
        assert _same(x, y) and _same(z, y)


# ---- 3. the neutral table
def test_an_all_break_table_is_the_plain_philox_run_and_none_restores_it():
    plain, cols, _ = _stepper(200, N70, seed=11)
    st, _, _ = _stepper(200, N70, seed=11)
    try:
        st.set_noise_correlation(np.zeros(cols.dim_d), np.ones(cols.dim_d))
        plain.step_rows(1, 96)
        st.step_rows(1, 96)
        assert _same(st.get_state(), plain.get_state()) and _same(st.moments(), plain.moments())
        st.set_noise_correlation(None)
        assert st.noise_correlation() is None
        with pytest.raises(Exception, match="noise correlation"):
            st.noise_field_base()
        # (no attempt of these 96 rows was abandoned, so the scales the in-kernel source resumes with are the plain run's)
        assert np.all(plain.noise_scale() == 1.0)
        plain.step_rows(97, 48)
        st.step_rows(97, 48)
        assert _same(st.get_state(), plain.get_state()) and _same(st.moments(), plain.moments())
    finally:
        plain.close()
        st.close()


# ---- 4. shards
def test_two_shards_hold_the_rows_of_the_one_handle():
    psi = _spread(golden("g1_tables_200.npz")["initial_cond"], N70, width=20.0)
    out = {}
    for lo, hi in ((0, N70), (0, 33), (33, N70)):
        st, cols, _ = _stepper(200, hi - lo, seed=13, offset=lo, psi=psi[lo:hi])
        try:
            st.set_noise_correlation(*_tables(cols))
            st.step_rows(1, 96)
            out[lo, hi] = (st.get_state(), st.noise_field_base(), np.asarray(st.moments()))
        finally:
            st.close()
    whole = out[0, N70]
    for lo, hi in ((0, 33), (33, N70)):
        assert _same(out[lo, hi][0], whole[0][lo:hi]) and _same(out[lo, hi][1], whole[1][lo:hi])
    assert np.array_equal(out[0, 33][2] + out[33, N70][2], whole[2])


# ---- 5. with the filters
def _filtered_run(rows_per_launch):
    from hydromodel_amd.stepper import noise_correlate
    st, cols, forcing = _stepper(200, N70, seed=7, spread=True)
    try:
        st.set_rows_per_launch(rows_per_launch)
        a, b = _tables(cols)
        st.set_noise_correlation(a, b)
        st.set_filter(48, 1.5 * cols.dz, 11)
        start = st.filter_base()
        want = noise_correlate(np.stack([st.philox_normals(m, 0) for m in range(N70)]), a, b)
        assert _same(start, want) and _same(st.noise_field_base(), want)
        assert forcing.wtd_obs[48] >= 0 and forcing.refresh[48]
        st.step_rows(1, 47)
        base_pre = st.filter_base()
        st.step_rows(48, 1)
        anc, base_post = st.filter_ancestors(), st.filter_base()
        st.step_rows(49, 48)
        return anc, base_pre, base_post, st.get_state(), st.filter_table(), st.moments(), st.filter_base()
    finally:
        st.close()


def test_a_particle_filter_on_a_correlated_source_carries_the_correlated_base():
    anc, base_pre, base_post, *run = _filtered_run(0)
    assert not np.array_equal(anc, np.arange(N70))                  # resampling chose
    assert _same(base_post, base_pre[anc])                          # (row 48 refreshes: no damping)
    for x, y in zip([anc, base_pre, base_post] + run, _filtered_run(5)):
        assert _same(x, y)


def test_the_enkf_noise_field_starts_from_the_correlated_base():
    from hydromodel_amd.stepper import noise_correlate
    st, cols, _ = _stepper(200, N70, seed=7, spread=True)
    try:
        a, b = _tables(cols)
        st.set_noise_correlation(a, b)
        st.set_enkf(48, 1.5 * cols.dz, 0.0, 3)
        st.set_enkf_noise_field(True, 0.5)
        want = noise_correlate(np.stack([st.philox_normals(m, 0) for m in range(N70)]), a, b)
        assert _same(st.enkf_noise_base(), want)
        st.step_rows(1, 48)                                          # one analysis of the correlated vectors
        after = st.enkf_noise_base()
        assert np.all(np.isfinite(after)) and not _same(after, want)
    finally:
        st.close()


def test_refusals():
    from hydromodel_amd._lib import HcError
    st, cols, forcing = _stepper(200, N70, spread=True)
    try:
        a, b = _tables(cols)
        st.set_filter(48, 10.0, 1)
        with pytest.raises(HcError, match="particle filter is on .* set the correlation first"):
            st.set_noise_correlation(a, b)
        st.set_filter(0)
        st.set_enkf(48, 10.0, 0.0, 1)
        st.set_enkf_noise_field(True, 0.0)
        with pytest.raises(HcError, match="EnKF's noise field is on .* set the correlation first"):
            st.set_noise_correlation(a, b)
        assert st.noise_correlation() is None
        st.set_enkf(0)
        st.set_noise_correlation(a, b)
        with pytest.raises(HcError, match="set the correlation after the spin-up"):
            st.spinup(forcing.zwtd_cm[0], cols.z[0], forcing_row=0, max_iterations=5)
        with pytest.raises(HcError, match="set the correlation after the spin-up"):
            st.step_rows(1, 1, spinup=True)
        with pytest.raises(HcError, match="set the correlation after the spin-up"):
            st.set_noise_scale(np.full(N70, 0.8))
        # the tables' own rules
        for bad_a, bad_b, msg in ((np.where(np.arange(cols.dim_d) == 0, 0.5, a), b, "a_0"),
                                  (np.where(np.arange(cols.dim_d) == 3, 1.0, a), b, r"outside \[0, 1\)"),
                                  (a, np.where(np.arange(cols.dim_d) == 3, -b, b), "<= 0"),
                                  (a, np.where(np.arange(cols.dim_d) == 3, 0.5 * b, b), "unit-variance"),
                                  (np.where(np.arange(cols.dim_d) == 3, 0.0, a), b, "unit-variance"),
                                  (np.where(np.arange(cols.dim_d) == 3, np.nan, a), b, "not finite")):
            with pytest.raises(HcError, match=msg):
                st.set_noise_correlation(bad_a, bad_b)
            assert st.noise_correlation() is None                    # refused: off
        st.set_noise_host(np.zeros((N70, cols.dim_d)))
        with pytest.raises(HcError, match="needs a Philox run"):
            st.set_noise_correlation(a, b)
    finally:
        st.close()


# ---- 6. the field's statistics (fixed seeds: nothing is left to chance at run time)
def test_statistics_of_the_base_vectors():
    N = 4096
    st, cols, _ = _stepper(1, N, seed=2024)
    try:
        a, _ = _tables(cols, 50.0, layers=True)
        st.set_noise_correlation(*_tables(cols, 50.0, layers=True))
        z = st.noise_field_base()
    finally:
        st.close()
    rho = float(np.exp(-cols.dz / 50.0))
    var = z.var(axis=0, ddof=1)
    assert np.all(np.abs(var - 1.0) <= 6.0 * np.sqrt(2.0 / (N - 1)))
    corr = lambda i, j: float(np.corrcoef(z[:, i], z[:, j])[0, 1])   # noqa: E731
    brk = int(np.flatnonzero(cols.z >= 50.0)[0])
    assert a[brk] == 0.0 and np.all(a[20:26] == rho) and brk < 20
    assert abs(corr(20, 21) - rho) <= 6.0 * (1.0 - rho ** 2) / np.sqrt(N - 1)
    assert abs(corr(20, 25) - rho ** 5) <= 6.0 * (1.0 - rho ** 10) / np.sqrt(N - 1)
    assert abs(corr(brk - 1, brk)) <= 6.0 / np.sqrt(N)


# ---- 7. checkpoint
def test_dump_and_restore_continue_a_correlated_run_bit_for_bit(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(1)
    psi0 = _spread(golden("g1_tables_1.npz")["initial_cond"], N70, width=20.0)
    kw = dict(seed=6, psi0=psi0, wtd_hist_stride=48, noise_correlation={"length_cm": 50.0, "layers": True})
    whole = EnsembleSimulation(cols, forcing, N70, **kw)
    try:
        assert whole.noise_correlation_break_count() == 2
        whole.advance(60)
        path = whole.dump(tmp_path / "ck.h5")
        whole.advance(36)
        want = [whole.stepper.get_state(), whole.moments(), whole.wtd_hist_table(), whole.stepper.noise_field_base()]
    finally:
        whole.close()
    back = EnsembleSimulation.restore(path, cols, forcing)
    try:
        assert back.next_row == 61 and back.noise_correlation == {"length_cm": 50.0, "layers": True}
        assert _same(back.stepper.noise_correlation()[0][0], _tables(cols)[0])
        back.advance(36)
        got = [back.stepper.get_state(), back.moments(), back.wtd_hist_table(), back.stepper.noise_field_base()]
    finally:
        back.close()
    for x, y in zip(want, got):
        assert _same(x, y)
    # a file without the keys restores as before
    plain = EnsembleSimulation(cols, forcing, N70, seed=6, psi0=psi0)
    try:
        plain.advance(10)
        path = plain.dump(tmp_path / "plain.h5")
    finally:
        plain.close()
    back = EnsembleSimulation.restore(path, cols, forcing)
    try:
        assert back.noise_correlation is None and back.stepper.noise_correlation() is None
    finally:
        back.close()


# ---- 8. the CLI
CORR_KEYS = {"noise_correlation_length_cm", "noise_correlation_layers", "noise_correlation_a"}
PLAIN_KEYS = {"moments", "wtd_mean_cm", "wtd_std_cm", "rows", "members", "gpus", "initial_cond"}


def _well_1_params(tmp_path):
    from hydromodel_amd.synthetic import default_parameters, write_forcing_csv, write_site_information
    params = default_parameters()
    params["Site_Information"] = str(write_site_information(tmp_path / "site.json", {10: WELLS[1]}))
    params["Data_Filename"] = str(write_forcing_csv(tmp_path / "forcing.csv", 1))
    return params


def test_cli_sweep_with_a_filter_takes_one_table_per_point(tmp_path, monkeypatch, capsys):
    from helpers import cli_params
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    params = cli_params(tmp_path)                                    # the synthetic well, D = 200
    monkeypatch.chdir(tmp_path)
    params["Output_Name"] = "Run_sweep"
    params["Ensemble"] = {"Members": 64, "Seed": 3, "Days": 2, "Filter": {"Stride": 48, "Sigma_cm": 10.0},
                          "Points": [{"Soil_Properties": {"n": 1.6}}, {"Soil_Properties": {"n": 2.4}}],
                          "Noise_Correlation": {"Length_cm": 25.0, "Layers": True}}
    (tmp_path / "sweep.json").write_text(json.dumps(params))
    cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "sweep.json")])
    out, said = loadResults(tmp_path / "Run_sweep_ensemble.h5"), capsys.readouterr().out
    _, cols, _ = digest(200)
    a = _tables(cols, 25.0)[0]
    assert CORR_KEYS <= set(out) and "filter_loglik" in out
    assert _same(np.asarray(out["noise_correlation_a"], dtype=np.float64), np.stack([a, a]))
    assert f" [Sweep 2 points x64] noise correlation: length 25 cm, {2 * int((a[1:] == 0.0).sum())} breaks" in said.splitlines()


def test_cli_block_writes_the_datasets_on_one_rank_and_on_two(tmp_path, monkeypatch, capsys):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    params = _well_1_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    block = {"Noise_Correlation": {"Length_cm": 50.0, "Layers": True}}
    files, logs = {}, {}
    for tag, extra in (("plain", {}), ("corr", block)):
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 64, "Seed": 3, "Days": 2, **extra}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = loadResults(tmp_path / f"Run_{tag}_ensemble.h5")
        logs[tag] = capsys.readouterr().out
    plain, corr = files["plain"], files["corr"]
    assert set(plain) == PLAIN_KEYS and "noise correlation" not in logs["plain"]
    assert set(corr) - set(plain) == CORR_KEYS
    _, cols, _ = digest(1)
    assert float(corr["noise_correlation_length_cm"]) == 50.0 and int(corr["noise_correlation_layers"]) == 1
    assert _same(np.asarray(corr["noise_correlation_a"], dtype=np.float64), _tables(cols)[0])
    said = [s for s in logs["corr"].splitlines() if s.strip()]
    assert " [Ensemble x64] noise correlation: length 50 cm, 2 breaks" in said
    assert said.index(" [Ensemble x64] noise correlation: length 50 cm, 2 breaks") == len(said) - 2   # then " Simulation completed."
    params["Ensemble"] = {"Members": 64, "Seed": 3, "Days": 2, **block}
    two, log2 = _run_ranks(tmp_path, "two", params, 2)
    assert set(two) == set(corr) and int(two["gpus"]) == 2
    for k in sorted(set(corr) - {"gpus"}):
        assert _same(np.asarray(two[k]), np.asarray(corr[k])), k
    assert log2.count("noise correlation: length 50 cm, 2 breaks") == 1
