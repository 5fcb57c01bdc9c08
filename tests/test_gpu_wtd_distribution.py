"""Ensemble water-table distributions on the GPU (include/hydrocol.h hc_set_wtd_hist, hc_wtd_distribution): the int32
histograms against np.bincount of the members' wtd_out and against the independent moment table, their invariance under
launch length, member split and parameter points, the quantiles against np.quantile(method="inverted_cdf"), the CRPS
against an exact restatement with Python integers and, for one member, against the reference's abs_error; no side
effects on the run, resume, and the CLI's "Ensemble": {"Distribution": ...} block.
Reference surface: wtd_est / abs_error of Simulation.run, simulation.py:612-615."""
import json
from fractions import Fraction

import numpy as np
import pytest

from helpers import WELLS, digest, forcing_frame, golden
from helpers import cli_params as _cli_params, run_cli_ranks as _run_ranks

pytestmark = pytest.mark.gpu
ROWS = 96                                                   # two days
LEVELS = (0.0, 0.05, 0.5, 0.95, 1.0)


def _stepper(well, N, stride, noise="philox", seed=7, offset=0):
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(well)
    st = EnsembleStepper(cols, forcing, N)
    st.set_state(golden(f"g1_tables_{well}.npz")["initial_cond"])
    if noise == "numpy":
        st.set_noise_host(np.random.default_rng(seed + offset).standard_normal((N, cols.dim_d)))
    else:
        st.set_noise_philox(seed, offset)
    st.set_wtd_hist(stride)
    return st, cols, forcing


def _skip_row(st, forcing, row):
    """Row `row` becomes a skip row (observation off the grid, simulation.py:582-588)."""
    st.lib.hc_set_forcing_row(st.h, row, float(forcing.precip[row]), float(forcing.atm[row]),
                              int(forcing.daylight[row]) | (int(forcing.wet_season[row]) << 1), -1)


def _crps_exact(h, obs, dz):
    """dz S / n^2 with S = sum_{b < D-1} (c_b - n [b >= obs])^2 in Python integers, rounded once."""
    c = np.cumsum(np.asarray(h).astype(object))
    n = int(c[-1])
    S = sum((int(c[b]) - (n if b >= obs else 0)) ** 2 for b in range(len(h) - 1))
    return float(Fraction(S) * Fraction(dz) / (n * n))


@pytest.mark.parametrize("noise", ["philox", "numpy"])
@pytest.mark.parametrize("stride", [1, 48])
@pytest.mark.parametrize("well", [1, 300, 401, 581])        # D = 101, 300, 401 and 581 (the split column)
def test_table_is_the_bincount_of_wtd_out_and_matches_the_moments(well, stride, noise):
    N = 64
    st, cols, forcing = _stepper(well, N, stride, noise=noise)
    T, D = forcing.dim_t, cols.dim_d
    skip = 5 if stride == 1 else 48
    try:
        _skip_row(st, forcing, skip)
        kw = {}
        if noise == "numpy":
            kw["fresh_noise"] = np.random.default_rng(1).standard_normal((st.n_refresh(1, ROWS), N, D))
        wtd = st.step_rows(1, ROWS, want_wtd=True, **kw)["wtd"]
        table, moments = st.wtd_hist_table(), st.moments()
    finally:
        st.close()
    n_hrow = (T - 1) // stride + 1
    assert table.shape == (1, n_hrow, D) and table.dtype == np.int32
    want = np.zeros((n_hrow, D), dtype=np.int64)
    for r in range(stride, ROWS + 1, stride):
        if r != skip:
            want[r // stride] = np.bincount(wtd[r - 1], minlength=D)
    assert np.array_equal(table[0], want)
    assert not table[0, 0].any() and not table[0, skip // stride].any()        # row 0 and the skip row are empty
    b = np.arange(D, dtype=np.int64)
    for j in range(1, n_hrow):                                                # the independent reduction, exactly
        r = j * stride
        h = table[0, j].astype(np.int64)
        assert [h.sum(), (b * h).sum(), (b * b * h).sum()] == [int(moments[0, r]), int(moments[1, r]), int(moments[2, r])]
    assert int(table[0, 1:ROWS // stride + 1].sum()) == N * (ROWS // stride - 1)


def _table(well, N, stride, rpl=0, offset=0, rows=ROWS):
    st, _, _ = _stepper(well, N, stride, offset=offset)
    try:
        if rpl:
            st.set_rows_per_launch(rpl)
        st.step_rows(1, rows)
        return st.wtd_hist_table()
    finally:
        st.close()


def test_table_does_not_depend_on_launch_length_or_member_split():
    ref = _table(300, 64, 1)
    assert ref[0, 1:ROWS + 1].sum(axis=1).tolist() == [64] * ROWS
    assert np.array_equal(_table(300, 64, 1, rpl=1), ref)
    halves = _table(300, 32, 1, rpl=7).astype(np.int64) + _table(300, 32, 1, rpl=13, offset=32)
    assert np.array_equal(halves, ref)


def test_sweep_handle_equals_the_stand_alone_points():
    from hydromodel_amd.digest import ColumnTables, ForcingDigest
    from hydromodel_amd.ensemble import SweepSimulation, merge_parameters
    from hydromodel_amd.synthetic import default_parameters
    params = default_parameters()
    pts = [{"Soil_Properties": {"n": 2.0}}, {"Soil_Properties": {"n": 1.6, "a0": 0.02}},
           {"Soil_Properties": {"psi_sat": -0.3}, "Hydraulic_Conductivity": {"Lambda_Exponent": 1.2}}]
    cols_all = [ColumnTables(merge_parameters(params, p), WELLS[1]) for p in pts]
    forcing = ForcingDigest(params, forcing_frame(1), cols_all[0])
    ic = golden("g1_tables_1.npz")["initial_cond"]
    psi0 = np.stack([ic, ic + 3.0, ic - 5.0])
    big = SweepSimulation(cols_all, forcing, 24, seed=9, psi0=psi0, wtd_hist_stride=2)
    big.advance(ROWS)
    table, dist = big.wtd_hist_table(), big.wtd_distribution(LEVELS)
    big.close()
    assert table.shape == (3, (forcing.dim_t - 1) // 2 + 1, 101)
    assert dist["crps_cm"].shape == table.shape[:2] and dist["quantile_cm"].shape == table.shape[:2] + (len(LEVELS),)
    assert dist["crps_mean_cm"].shape == (3,)
    for k in range(3):
        one = SweepSimulation([cols_all[k]], forcing, 24, seed=9, first_point=k, psi0=psi0[k], wtd_hist_stride=2)
        one.advance(ROWS)
        assert np.array_equal(one.wtd_hist_table()[0], table[k]), k
        one.close()


def test_quantiles_and_crps_of_a_run_against_numpy_and_python_integers():
    N = 64
    st, cols, forcing = _stepper(401, N, 1)
    try:
        wtd = st.step_rows(1, ROWS, want_wtd=True)["wtd"]
        table = st.wtd_hist_table()
    finally:
        st.close()
    from hydromodel_amd.stepper import wtd_distribution
    d = wtd_distribution(table[0], forcing.wtd_obs, LEVELS, cols.dz, cols.z)
    assert np.array_equal(d["rows"], np.arange(forcing.dim_t))
    assert np.isnan(d["crps_cm"][0]) and np.all(d["quantile_idx"][0] == -1) and np.isnan(d["quantile_cm"][0]).all()
    crps = []
    for r in range(1, ROWS + 1):
        idx = wtd[r - 1]
        want_q = [int(np.quantile(idx, q, method="inverted_cdf")) for q in LEVELS]
        assert d["quantile_idx"][r].tolist() == want_q, r
        assert np.array_equal(d["quantile_cm"][r], cols.z[want_q])
        want = _crps_exact(table[0, r], int(forcing.wtd_obs[r]), cols.dz)
        assert abs(d["crps_cm"][r] - want) <= np.spacing(want), r
        assert d["count"][r] == N
        crps.append(d["crps_cm"][r])
    assert np.all(d["count"][ROWS + 1:] == 0) and np.isnan(d["crps_cm"][ROWS + 1:]).all()
    assert d["crps_mean_cm"] == pytest.approx(np.mean(crps), rel=1e-14)


def test_summary_of_synthetic_tables_at_the_edges():
    from hydromodel_amd.stepper import wtd_distribution
    D, dz = 300, 5.0
    z = np.arange(D) * dz
    big = (1 << 31) - 1
    rows = [(np.bincount([40] * 7, minlength=D), 40),                        # all mass on the observation: CRPS 0
            (np.bincount([0, 3, 3, 299, 150], minlength=D), 0),              # observation at bin 0
            (np.bincount([0, 3, 3, 299, 150], minlength=D), D - 1)]          # ... and at D - 1
    h = np.zeros(D, dtype=np.int64)
    h[0], h[D - 1] = big, big                                                # n ~ 2^32: S ~ 2^72 > 2^64
    rows.append((h, 150))
    h = np.zeros(D, dtype=np.int64)
    h[[10, 200, 201]] = [big, big - 5, 12345]
    rows.append((h, 0))
    rows.append((np.zeros(D, dtype=np.int64), 20))                            # n = 0
    rows.append((np.bincount([17], minlength=D), 250))                        # one member
    table = np.stack([r[0] for r in rows])
    d = wtd_distribution(table, np.array([r[1] for r in rows]), LEVELS, dz, z)
    for j, (h, o) in enumerate(rows):
        n = int(h.sum())
        assert d["count"][j] == n
        if n == 0:
            assert np.isnan(d["crps_cm"][j]) and np.all(d["quantile_idx"][j] == -1)
            continue
        want = _crps_exact(h, o, dz)
        assert abs(d["crps_cm"][j] - want) <= np.spacing(want), j
        c = np.cumsum(h.astype(np.int64))
        for lv, got in zip(LEVELS, d["quantile_idx"][j]):
            k = max(1, int(np.ceil(float(n) * lv)))
            assert got == int(np.argmax(c >= k)), (j, lv)
    assert d["crps_cm"][0] == 0.0
    assert d["crps_cm"][6] == abs(z[250] - z[17])
    assert d["crps_mean_cm"] == pytest.approx(np.nanmean(d["crps_cm"]), rel=1e-14)
    idx = np.array([0, 3, 3, 299, 150])
    assert d["quantile_idx"][1].tolist() == [int(np.quantile(idx, q, method="inverted_cdf")) for q in LEVELS]


def test_one_member_crps_is_the_reference_abs_error():
    st, cols, forcing = _stepper(300, 1, 1)
    try:
        wtd = st.step_rows(1, ROWS, want_wtd=True)["wtd"]
        table = st.wtd_hist_table()
    finally:
        st.close()
    from hydromodel_amd.stepper import wtd_distribution
    d = wtd_distribution(table, forcing.wtd_obs, (0.5,), cols.dz, cols.z)
    solved = [r for r in range(1, ROWS + 1) if forcing.wtd_obs[r] >= 0]
    assert len(solved) == ROWS
    for r in solved:
        abs_error = np.abs(forcing.zwtd_cm[r] - cols.z[wtd[r - 1, 0]])          # simulation.py:615
        assert d["crps_cm"][0, r] == abs_error, r
        assert d["quantile_idx"][0, r, 0] == wtd[r - 1, 0]


@pytest.mark.parametrize("well", [300, 581])
def test_histograms_leave_the_run_alone(well):
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(well)
    ic = golden(f"g1_tables_{well}.npz")["initial_cond"]
    res = []
    for stride in (0, 1):
        st = EnsembleStepper(cols, forcing, 64)
        st.set_state(ic)
        st.set_noise_philox(3, 0)
        if stride:
            st.set_wtd_hist(stride)
        out = st.step_rows(1, ROWS, want_wtd=True)
        res.append((st.get_state(), out["wtd"], st.moments(), st.counters()))
        st.close()
    (a_psi, a_w, a_m, a_c), (b_psi, b_w, b_m, b_c) = res
    assert np.array_equal(a_psi.view(np.int64), b_psi.view(np.int64))
    assert np.array_equal(a_w, b_w) and np.array_equal(a_m, b_m) and a_c == b_c


def test_resume_from_a_dump_gives_the_uninterrupted_table_and_summary(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(300)
    ic = golden("g1_tables_300.npz")["initial_cond"]
    full = EnsembleSimulation(cols, forcing, 64, seed=9, psi0=ic, wtd_hist_stride=3)
    full.advance(ROWS)
    want, want_d = full.wtd_hist_table(), full.wtd_distribution()
    full.close()
    first = EnsembleSimulation(cols, forcing, 64, seed=9, psi0=ic, wtd_hist_stride=3)
    first.advance(50)
    path = first.dump(tmp_path / "ckpt.h5")
    first.close()
    resumed = EnsembleSimulation.restore(path, cols, forcing)
    resumed.advance(ROWS - 50)
    got, got_d = resumed.wtd_hist_table(), resumed.wtd_distribution()
    resumed.close()
    assert resumed.wtd_hist_stride == 3 and np.array_equal(got, want)
    for k in ("count", "quantile_idx", "quantile_cm", "crps_cm"):
        assert np.array_equal(got_d[k], want_d[k], equal_nan=got_d[k].dtype.kind == "f"), k
    assert got_d["crps_mean_cm"] == want_d["crps_mean_cm"]


NEW_KEYS = {"wtd_hist", "wtd_hist_rows", "wtd_hist_count", "wtd_quantile_levels", "wtd_quantile_cm", "wtd_crps_cm",
            "wtd_crps_mean_cm"}


def test_cli_distribution_block_writes_the_new_datasets_and_leaves_the_rest_alone(tmp_path, monkeypatch, capsys):
    from hydromodel_amd import cli
    from hydromodel_amd.simulation import loadResults
    params = _cli_params(tmp_path)
    monkeypatch.chdir(tmp_path)
    files, logs = {}, {}
    pts = [{"Soil_Properties": {"n": 1.6}}, {"Soil_Properties": {"n": 2.4}}]
    for tag, extra in (("plain", {}), ("dist", {"Distribution": {"Stride": 24, "Quantiles": [0.05, 0.5, 0.95]}}),
                       ("sweep", {"Points": pts, "Distribution": {"Stride": 48}})):
        params["Output_Name"] = f"Run_{tag}"
        params["Ensemble"] = {"Members": 128, "Seed": 3, "Days": 2, **extra}
        (tmp_path / f"{tag}.json").write_text(json.dumps(params))
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / f"{tag}.json")])
        files[tag] = loadResults(tmp_path / f"Run_{tag}_ensemble.h5")
        logs[tag] = capsys.readouterr().out
    plain, dist, sweep = files["plain"], files["dist"], files["sweep"]
    T, D = len(plain["moments"][0]), plain["initial_cond"].shape[-1]
    assert set(plain) == {"moments", "wtd_mean_cm", "wtd_std_cm", "rows", "members", "gpus", "initial_cond"}
    assert "CRPS" not in logs["plain"]
    assert set(dist) - set(plain) == NEW_KEYS
    n_hrow = (T - 1) // 24 + 1
    assert dist["wtd_hist"].shape == (n_hrow, D) and dist["wtd_hist"].dtype == np.int32
    assert dist["wtd_hist_rows"].tolist() == list(range(0, T, 24))
    assert dist["wtd_hist_count"].shape == (n_hrow,) and dist["wtd_hist_count"][1:5].tolist() == [128] * 4
    assert dist["wtd_quantile_levels"].tolist() == [0.05, 0.5, 0.95]
    assert dist["wtd_quantile_cm"].shape == (n_hrow, 3) and dist["wtd_crps_cm"].shape == (n_hrow,)
    assert np.isfinite(dist["wtd_crps_cm"][1:5]).all() and np.isnan(dist["wtd_crps_cm"][5:]).all()
    assert float(dist["wtd_crps_mean_cm"]) == pytest.approx(dist["wtd_crps_cm"][1:5].mean(), rel=1e-14)
    assert f"[Ensemble x128] CRPS = {float(dist['wtd_crps_mean_cm']):.3f} cm over 4 rows" in logs["dist"]
    for k in plain:                                          # every pre-existing dataset, byte for byte
        a, b = np.asarray(plain[k]), np.asarray(dist[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    n_hrow = (T - 1) // 48 + 1
    assert {k for k in sweep if k.startswith(("wtd_hist", "wtd_quantile", "wtd_crps"))} == NEW_KEYS
    assert sweep["wtd_hist"].shape == (2, n_hrow, D) and sweep["wtd_hist_count"].shape == (2, n_hrow)
    assert sweep["wtd_quantile_cm"].shape == (2, n_hrow, 5) and sweep["wtd_crps_cm"].shape == (2, n_hrow)
    assert sweep["wtd_crps_mean_cm"].shape == (2,) and np.isfinite(sweep["wtd_crps_mean_cm"]).all()
    assert sweep["wtd_hist_count"][:, 1:3].tolist() == [[128, 128], [128, 128]]
    assert "[Sweep 2 points x128] CRPS = " in logs["sweep"]


@pytest.mark.parametrize("sweep", [False, True])
def test_two_ranks_sharing_the_card_write_what_one_rank_writes(tmp_path, sweep):
    params = _cli_params(tmp_path)
    ens = {"Members": 250, "Seed": 5, "Days": 2, "Distribution": {"Stride": 12, "Quantiles": [0.1, 0.5, 0.9]}}
    if sweep:
        ens.update(Members=32, Points=[{"Soil_Properties": {"n": n}} for n in (1.6, 2.0, 2.4)])
    params["Ensemble"] = ens
    one, log1 = _run_ranks(tmp_path, "one", params, 1)
    two, log2 = _run_ranks(tmp_path, "two", params, 2)
    for k in ("wtd_hist", "wtd_hist_count", "wtd_quantile_cm", "wtd_crps_cm", "wtd_crps_mean_cm"):
        a, b = np.asarray(one[k]), np.asarray(two[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    line = [s for s in log1.splitlines() if "CRPS" in s]
    assert len(line) == 1 and line == [s for s in log2.splitlines() if "CRPS" in s]
