"""Ensemble conductivity profiles reduced on the GPU (include/hydrocol.h hc_set_conductivity_stats): the hook against the
plugin call and the reference's golden values, the table against the NumPy restatement for every noise source (the row's
noise vector rebuilt on the host from the draws, the scales and the failed attempts), its independence of launch length,
staging and member split, the layers' effective conductivity, the filters' forecast, resume and the CLI's key."""
from functools import lru_cache

import numpy as np
import pytest

from helpers import WELLS, cli_params, digest, digest_point, forcing_frame, golden, rel_err, run_cli_ranks
from test_gpu_enkf import _spread

pytestmark = pytest.mark.gpu

ROWS, STRIDE = 96, 24                                       # two days: profile rows 0 (snapshot), 24, 72 and the refresh rows 48, 96
PROWS = (0, 24, 48, 72, 96)
LAYERS_CM = [(0.0, 100.0), (50.0, 300.0), (0.0, 1.0e4)]     # overlap, a partial tile, the whole column
SEED = 7


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _ranges(cols):
    from hydromodel_amd.stepper import layer_ranges
    return layer_ranges(cols.z, [(a, min(b, float(cols.z[-1]) + cols.dz)) for a, b in LAYERS_CM])


def _columns(well, points):
    """The handle's columns: the well's default point, or two points (the second with lambda = 1.3: generic exponents)."""
    _, cols, forcing = digest(well)
    return ([cols, digest_point("a03l13", well=well)[1]] if points == 2 else cols), cols, forcing


def _psi0(well, N):
    return _spread(golden(f"g1_tables_{well}.npz")["initial_cond"], N)


def _parts(st, table=None):
    from hydromodel_amd.stepper import split_conductivity_table
    t = st.conductivity_table() if table is None else table
    return split_conductivity_table(t, st.P, st.T, st.D, len(st.conductivity_ranges), st.profile_stride)


# ---- 1. the hook against the plugin call ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["vrettas_fung", "vanGenuchten"])
def test_the_hook_returns_the_plugins_conductivities_and_their_logarithms(model):
    from hydromodel_amd.digest import ColumnTables, ForcingDigest
    from hydromodel_amd.stepper import EnsembleStepper
    params, _, _ = digest(1, model)
    cols = ColumnTables(params, WELLS[1])                   # (a private copy: one of its cells is taken out of every layer)
    cols.noisec_node = np.array(cols.noisec_node)
    cols.noisec_node[3] = -1.0
    forcing = ForcingDigest(params, forcing_frame(1), cols)
    N, D = 6, cols.dim_d
    assert D == 101
    psi = _psi0(1, N)
    psi[1] = 10.0                                           # a saturated column
    psi[2] = -1.0e200                                       # a very dry one: theta sits at theta_res, K_hrc is exactly 0
    base = np.random.default_rng(3).standard_normal((N, D))
    st = EnsembleStepper(cols, forcing, N)
    try:
        st.set_state(psi)
        st.set_noise_host(base)
        got, want = st.conductivity_eval(1), st.model_nodes()         # row 1 does not refresh: the base vectors
        assert got.shape == (4, N, D)
        assert _same(got[0], want["K"]) and _same(got[1], want["K_bkg"])
        if model == "vrettas_fung":
            assert np.all(got[0][2] == 0.0) and np.all(np.isneginf(got[2][2]))
        assert np.ptp(got[1][:, 3]) == 0.0 and np.ptp(got[1][:, 4]) > 0.0 or model != "vrettas_fung"   # the cell in no layer
        assert np.all(got[0][1] == got[1][1])                          # saturated: K_hrc = K_bkg
        with np.errstate(divide="ignore"):
            ln = np.log(got[:2])
        finite = np.isfinite(ln)
        assert np.array_equal(finite, np.isfinite(got[2:])) and finite[:, [0, 1, 3, 4, 5]].all()
        assert np.max(np.abs(got[2:][finite] - ln[finite])) < 1e-12
    finally:
        st.close()


# ---- 2. the reference's values --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,tag", [("vrettas_fung", "vf"), ("vanGenuchten", "vg")])
def test_exp_of_the_hooks_logarithms_meets_the_reference(model, tag):
    """The bound test_model_nodes_matches_reference_golden holds hc_model_nodes to on the same fixture: 1e-9."""
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(300, model)
    g = golden("g2_pointwise_300.npz")
    names = ("sweep", "ic", "moist", "dry")
    Y = np.array([g[f"psi_{n}"] for n in names])
    st = EnsembleStepper(cols, forcing, len(Y))
    try:
        st.set_state(Y)
        st.set_noise_host(np.tile(g["n_rnd"], (len(Y), 1)))
        out = st.conductivity_eval(1)
        for k, name in enumerate(names):
            assert rel_err(np.exp(out[3][k]), g[f"{tag}_{name}_node_kbkg"]) < 1e-9
            assert rel_err(np.exp(out[2][k]), g[f"{tag}_{name}_node_K"]) < 1e-9
    finally:
        st.close()


# ---- 3. the table against the restatement, every noise source -----------------------------------------------------------
def _start(well, N, points, source, ranges=None, budget=0, rpl=0, offset=0, psi=None, uptake=False, on=True, vectors=None):
    """A handle with the profile statistics at STRIDE and the conductivity table on, row 0 counted; (stepper, caller's
    fresh vectors or None)."""
    from hydromodel_amd.stepper import (EnsembleStepper, layer_cells, noise_correlation_tables, period_ends)
    columns, cols, forcing = _columns(well, points)
    st = EnsembleStepper(columns, forcing, N)
    st.set_state(_psi0(well, N) if psi is None else psi)
    fresh = None
    if source == "host":
        rng = np.random.default_rng(SEED + offset)
        base, fresh = vectors or (rng.standard_normal((N, cols.dim_d)), rng.standard_normal((2, N, cols.dim_d)))
        st.set_noise_host(base)
    else:
        st.set_noise_philox(SEED, offset)
        if source == "correlated":
            st.set_noise_correlation(*noise_correlation_tables(cols.z, 50.0, ()))
    if budget:
        st.set_iteration_budget(budget)
    if rpl:
        st.set_rows_per_launch(rpl)
    st.set_profile_stats(STRIDE)
    if on:
        st.set_conductivity_stats(_ranges(cols) if ranges is None else ranges)
    st.profile_snapshot(0)
    if uptake:                                              # every row staged (stage_all)
        st.set_period_totals(period_ends(forcing.dim_t, 48), [], 0, (0, 0))
        st.set_root_uptake(layer_cells(cols.z, [(0.0, 100.0)]), 0)
    return st, fresh


def _row_noise(st, source, fresh, base0, scale0, failed, offset=0):
    """[ROWS + 1][N][D]: the noise vector of every row 0 .. ROWS as its solve left it (conductivity_noise_of), from the
    draws, the scales and the failed attempts -- nothing the table's kernels computed."""
    from hydromodel_amd.stepper import conductivity_noise_of
    refresh = np.asarray(st.forcing.refresh[1:ROWS + 1], dtype=bool)
    draws = np.cumsum(np.asarray(st.forcing.refresh, dtype=np.int64))[1:ROWS + 1][refresh]
    out = np.empty((ROWS + 1, st.N, st.D))
    for m in range(st.N):
        gid = offset + m
        if source == "host":
            vec, fr, scale = base0[m], fresh[:, m], None
        elif source == "correlated":
            vec, fr, scale = base0[m], np.array([st.noise_field_normals(gid, d) for d in draws]), None
        else:
            vec, fr, scale = st.philox_normals(gid, 0), np.array([st.philox_normals(gid, d) for d in draws]), scale0[m]
        out[0, m] = vec if scale is None else vec * scale
        out[1:, m] = conductivity_noise_of(vec, fr, refresh, failed[:, m], scale)
    return out


def _restated(st, psi_rows, noise):
    """The table of the profile rows from the states and the rebuilt noise: K and ln K from the hook on a second handle fed
    (psi, nu) as caller noise (test 1 ties the hook to the plugin call), quantised on the host."""
    from hydromodel_amd.stepper import EnsembleStepper, conductivity_tables_of
    ev = EnsembleStepper(st.points if st.P > 1 else st.cols, st.forcing, st.N)
    try:
        lnk, k = [], []
        for r in PROWS:
            ev.set_state(psi_rows[r])
            ev.set_noise_host(noise[r])
            e = ev.conductivity_eval(1)
            lnk.append(e[2:])
            k.append(e[0])
    finally:
        ev.close()
    mpp = st.N // st.P
    return [conductivity_tables_of(np.array(lnk)[:, :, p * mpp:(p + 1) * mpp], st.conductivity_ranges,
                                   k_rows=np.array(k)[:, p * mpp:(p + 1) * mpp]) for p in range(st.P)]


def _check_against_restatement(st, source, fresh, want_psi=True):
    from hydromodel_amd.stepper import split_conductivity_table
    base0 = st.get_noise_base() if source == "host" else st.noise_field_base() if source == "correlated" else None
    scale0 = st.noise_scale() if source == "philox" else None
    psi0 = st.get_state()
    out = st.step_rows(1, ROWS, fresh_noise=fresh, want_psi=True, want_stats=True)
    assert (st.forcing.wtd_obs[:ROWS + 1] >= 0).all()
    noise = _row_noise(st, source, fresh, base0, scale0, out["failed"])
    psi_rows = np.concatenate([psi0[None], out["psi"]])
    L = len(st.conductivity_ranges)
    got = _parts(st)
    for p, table in enumerate(_restated(st, psi_rows, noise)):
        want = split_conductivity_table(table, 1, len(PROWS), st.D, L, 1)
        for name in ("kmom", "kcnt", "kmom_layer", "kcnt_layer"):
            assert np.array_equal(got[name][p, :len(PROWS)], want[name][0]), (source, p, name)
            assert not got[name][p, len(PROWS):].any()
        assert int(want["ovf"][0]) == 0
    assert st.conductivity_overflow() == 0
    refresh = np.asarray(st.forcing.refresh[1:ROWS + 1], dtype=bool)
    damped_fresh = int((out["failed"][[r - 1 for r in PROWS[1:] if refresh[r - 1]]] > 0).sum())
    damped_base = int((out["failed"][~refresh] > 0).any(axis=0).sum())
    return damped_fresh, damped_base, noise, out


@pytest.mark.parametrize("N, points", [(6, 1), (70, 1), (70, 2)])
@pytest.mark.parametrize("source", ["philox", "host", "correlated"])
def test_the_table_equals_the_restatement_on_the_rebuilt_noise(source, N, points):
    st, fresh = _start(1, N, points, source)
    try:
        assert st.D == 101 and st.conductivity_layout()[0]
        _check_against_restatement(st, source, fresh)
        counts = _parts(st)["kcnt"][:, :len(PROWS)]
        assert counts.max() == N // points and (counts[..., 1] == N // points).all()     # K_bkg is always counted
    finally:
        st.close()


def test_failed_attempts_damp_the_refresh_vector_and_the_base():
    """A budget of 24 phase iterations abandons the costly attempts (tests/test_gpu_round2.py): the table still equals the
    restatement, on rows whose refresh vector was damped and on members whose base was."""
    st, fresh = _start(1, 70, 1, "philox", budget=24)
    try:
        damped_fresh, damped_base, _, _ = _check_against_restatement(st, "philox", fresh)
        print(f"refresh vectors damped on profile rows: {damped_fresh}, members with a damped base: {damped_base}")
        assert damped_fresh >= 1 and damped_base >= 1
        assert (st.noise_scale() < 1.0).sum() == damped_base
    finally:
        st.close()


# ---- 4. invariance -------------------------------------------------------------------------------------------------------
def _run(N=6, source="philox", offset=0, psi=None, on=True, want_psi=False, **kw):
    st, fresh = _start(1, N, 1, source, offset=offset, psi=psi, on=on, **kw)
    try:
        st.step_rows(1, ROWS, fresh_noise=fresh, want_psi=want_psi)
        return (st.conductivity_table() if on else None), st.get_state(), st.profile_table(), st.last_launches
    finally:
        st.close()


@lru_cache(maxsize=None)
def _whole():
    return _run()


def test_the_table_does_not_depend_on_launches_staging_or_member_split():
    table, state, prof, launches = _whole()
    assert launches == 4                                    # a launch ends on each of the rows 24, 48, 72, 96
    for kw in (dict(rpl=7), dict(rpl=48), dict(want_psi=True), dict(rpl=7, want_psi=True), dict(uptake=True)):
        t, s, p, _ = _run(**kw)
        assert _same(t, table) and _same(s, state) and _same(p, prof), kw
    psi = _psi0(1, 6)
    halves = [_run(3, offset=o, psi=psi[o:o + 3]) for o in (0, 3)]
    assert _same(halves[0][0] + halves[1][0], table)
    assert _same(np.concatenate([h[1] for h in halves]), state)
    # the cut launches change no state: a run without the table
    none, s, p, n = _run(on=False)
    assert none is None and _same(s, state) and _same(p, prof) and n == 1


# ---- 5. layers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("well", [1, 300])
def test_the_layers_effective_conductivity_equals_the_restatement(well):
    from hydromodel_amd.stepper import EnsembleStepper, conductivity_layer_of, conductivity_tables_of, split_conductivity_table
    _, cols, forcing = digest(well)
    N, D, ranges = 9, cols.dim_d, _ranges(cols)
    assert ranges.tolist() == [[0, 20], [10, 60], [0, D]]
    psi = _psi0(well, N)
    psi[4, 15] = -1.0e200                                   # one node with K_hrc = 0: in layers 0, 1 and 2 ...
    psi[5, 40] = -1.0e200                                   # ... and one in layers 1 and 2 only
    st = EnsembleStepper(cols, forcing, N)
    try:
        st.set_state(psi)
        st.set_noise_philox(SEED, 0)
        st.set_profile_stats(STRIDE)
        st.set_conductivity_stats(ranges)
        st.profile_snapshot(0)
        e = st.conductivity_eval(0)
        assert e[0][4, 15] == 0.0 and e[0][5, 40] == 0.0 and (np.delete(e[0], [4, 5], axis=0) > 0.0).all()
        want = split_conductivity_table(conductivity_tables_of(e[2:][None], ranges, k_rows=e[0][None]), 1, 1, D, 3, 1)
        got = _parts(st)
        assert got["kcnt_layer"][0, 0].tolist() == [N - 1, N - 2, N - 2] == want["kcnt_layer"][0, 0].tolist()
        for name in ("kmom", "kcnt", "kmom_layer"):
            assert np.array_equal(got[name][0, 0], want[name][0, 0]), name
        stats = st.conductivity_stats()
        keff = conductivity_layer_of(e[0], ranges)
        ok = np.isfinite(np.log(np.where(keff > 0, keff, np.nan)))
        for l in range(3):
            assert abs(stats["lnK_eff_mean"][0, l] - np.log(keff[ok[:, l], l]).mean()) < 1e-9
            assert abs(stats["K_eff_geomean"][0, l] / np.exp(np.log(keff[ok[:, l], l]).mean()) - 1.0) < 1e-8
    finally:
        st.close()


# ---- 6. with the filters: the table describes the forecast -------------------------------------------------------------
def _assimilate(st, owner, sigma):
    if owner == "filter":
        st.set_filter(STRIDE, sigma, 3)
    else:
        st.set_enkf(STRIDE, sigma, 0.0, 11)
        st.set_enkf_noise_field(True, 0.25 if sigma < 1e20 else 0.0)


def _base(st, owner):
    return st.filter_base() if owner == "filter" else st.enkf_noise_base()


@pytest.mark.parametrize("owner", ["filter", "enkf_noise"])
def test_an_assimilation_rows_table_is_the_restatement_on_the_forecast_base(owner):
    """Row 72 is a profile row, an assimilation row and no refresh row: its noise is the members' base as the analyses of
    rows 24 and 48 and the solves up to row 72 left it, before the analysis of row 72 moves it."""
    from hydromodel_amd.stepper import conductivity_noise_of, conductivity_tables_of, EnsembleStepper, split_conductivity_table
    N, sigma = 64, 7.5
    st, _ = _start(1, N, 1, "philox")
    try:
        _assimilate(st, owner, sigma)
        st.step_rows(1, 71)
        before = _base(st, owner)                           # (a run stopped one row earlier)
        out = st.step_rows(72, 1, want_psi=True, want_stats=True)
        after = _base(st, owner)
        noise = np.stack([conductivity_noise_of(before[m], np.zeros((0, st.D)), [False], out["failed"][:, m])[0] for m in range(N)])
        assert not np.array_equal(after, noise)             # the analysis of row 72 moved the vectors: the table must not see it
        ev = EnsembleStepper(st.cols, st.forcing, N)
        try:
            ev.set_state(out["psi"][0])
            ev.set_noise_host(noise)
            e = ev.conductivity_eval(1)
        finally:
            ev.close()
        L = len(st.conductivity_ranges)
        want = split_conductivity_table(conductivity_tables_of(e[2:][None], st.conductivity_ranges, k_rows=e[0][None]), 1, 1, st.D, L, 1)
        got = _parts(st)
        for name in ("kmom", "kcnt", "kmom_layer", "kcnt_layer"):
            assert np.array_equal(got[name][0, 3], want[name][0, 0]), name
        stopped = st.conductivity_table()
    finally:
        st.close()
    whole, _ = _start(1, N, 1, "philox")
    try:
        _assimilate(whole, owner, sigma)
        whole.step_rows(1, ROWS)
        got = _parts(whole)
        for name, part in _parts(whole, stopped).items():
            assert np.array_equal(got[name][:, :4] if name != "ovf" else got[name], part[:, :4] if name != "ovf" else part), name
        assert got["kcnt"][0, 4].max() == N
    finally:
        whole.close()


@pytest.mark.parametrize("owner", ["filter", "enkf_noise"])
def test_a_neutral_analysis_leaves_the_plain_runs_table(owner):
    """The plain run is the one without a filter on the same noise path: the handle of a filtered Philox run keeps the
    vectors in memory, so its twin is the caller-noise run fed the same normals (tests/test_gpu_filter.py's neutral filter)."""
    N = 64
    probe, _ = _start(1, N, 1, "philox", on=False)
    try:
        vectors = (np.stack([probe.philox_normals(m, 0) for m in range(N)]),
                   np.stack([[probe.philox_normals(m, d) for m in range(N)] for d in (1, 2)]))
    finally:
        probe.close()
    plain, fresh = _start(1, N, 1, "host", vectors=vectors)
    try:
        plain.step_rows(1, ROWS, fresh_noise=fresh)
        want = plain.conductivity_table()
    finally:
        plain.close()
    st, _ = _start(1, 64, 1, "philox")
    try:
        _assimilate(st, owner, 1e30)
        st.step_rows(1, ROWS)
        assert _same(st.conductivity_table(), want)
    finally:
        st.close()


# ---- 7. checkpoint and the CLI -----------------------------------------------------------------------------------------
def test_a_restore_between_two_profile_rows_continues_bit_for_bit(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(1)
    kw = dict(seed=SEED, psi0=golden("g1_tables_1.npz")["initial_cond"], profile_stride=STRIDE,
              conductivity={"layers_cm": [(0.0, 100.0), (50.0, 300.0)]})
    whole = EnsembleSimulation(cols, forcing, 6, **kw)
    try:
        whole.advance(ROWS)
        want = (whole.conductivity_table(), whole.stepper.get_state(), whole.stepper.profile_table())
        stats = whole.conductivity_stats()
        assert stats["lnK_hrc_mean"].shape == (whole.stepper.diag_counts()["prows"], cols.dim_d)
        assert stats["lnK_eff_mean"].shape[1] == 2 and stats["nodes"].tolist() == [[0, 20], [10, 60]]
        assert np.isfinite(stats["lnK_bkg_mean"][:5]).all() and np.isnan(stats["lnK_bkg_mean"][5:]).all()
    finally:
        whole.close()
    first = EnsembleSimulation(cols, forcing, 6, **kw)
    try:
        first.advance(60)
        path = first.dump(tmp_path / "ck.npz")
    finally:
        first.close()
    again = EnsembleSimulation.restore(path, cols, forcing)
    try:
        assert again.next_row == 61 and again.conductivity_ranges.tolist() == [[0, 20], [10, 60]]
        again.advance(ROWS - 60)
        got = (again.conductivity_table(), again.stepper.get_state(), again.stepper.profile_table())
    finally:
        again.close()
    for a, b in zip(got, want):
        assert _same(a, b)


def test_the_cli_writes_the_datasets_and_without_the_key_the_file_is_the_parents(tmp_path):
    params = cli_params(tmp_path)
    ens = {"Members": 12, "Days": 2, "Seed": 3, "Profiles": 24}
    off, printed_off = run_cli_ranks(tmp_path, "off", dict(params, Ensemble=dict(ens)), 1)
    on, printed = run_cli_ranks(tmp_path, "on", dict(params, Ensemble=dict(
        ens, Conductivity={"Layers_cm": [[0, 100], [100, 300]]})), 1)
    D, T_out = 200, len(off["profile_rows"])
    new = {"conductivity_rows": (T_out,), "conductivity_count": (T_out, D, 2), "conductivity_overflow": (),
           "K_eff_layers_cm": (2, 2), "K_eff_nodes": (2, 2), "K_eff_count": (T_out, 2)}
    for q, width in (("hrc", D), ("bkg", D), ("eff", 2)):
        new.update({f"lnK_{q}_mean": (T_out, width), f"lnK_{q}_std": (T_out, width), f"K_{q}_geomean": (T_out, width)})
    assert set(on) - set(off) == set(new) and set(off) <= set(on)
    for name, shape in new.items():
        assert np.shape(on[name]) == shape, name
    assert np.array_equal(on["conductivity_rows"], on["profile_rows"]) and int(on["conductivity_overflow"]) == 0
    assert (on["conductivity_count"][:5, :, 1] == 12).all() and not on["conductivity_count"][5:].any()
    assert np.allclose(on["K_bkg_geomean"][:5], np.exp(on["lnK_bkg_mean"][:5]), rtol=1e-15)
    assert " [Ensemble x12] conductivity: 200 nodes and 2 layers on 5 rows" in printed
    assert "conductivity" not in printed_off
    # the run without the key: every dataset it writes is in the other file too, byte for byte (the cut launches change
    # no state and no other table)
    for name, value in off.items():
        assert _same(np.asarray(on[name]), np.asarray(value)), name
