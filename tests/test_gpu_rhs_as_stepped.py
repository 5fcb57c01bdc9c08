"""The RHS the two-waves-per-SIMD step kernels really run (`hc_rhs_ex`, variant "step": `rhs_eval<..., ONE_BALLOT = true>`)
against the plain instantiation, BIT FOR BIT, and against the CPU oracle -- on the state bank of tests/rhs_states.py, whose
reach tests/test_rhs_states_cpu.py proves on the CPU.

Per case (a depth, a cell model, the split column on or off) and flag set, the bank is evaluated in launches of <= 40
members (every state twice, as neighbours) on every row type:

(a) variants "step" and "hook_layout" give the same bytes: dy/dt, c, s, f, pL and both diagnostics, with host noise and
    with Philox noise.  No tolerance -- the units are compiled with -ffp-contract=on and every shortcut of the step
    kernels' instantiation claims equal bits.  A failure names depth, state, row, quantity, the first differing node and
    both values in hex.  (`hc_rhs` itself, the "hook" variant without aux, is checked to be "hook_layout"'s dy/dt.)
(b) variant "step" against the oracle at the tiers of test_gpu_parity.py: c 1e-11 (floor 1e-7), s 1e-11 (floor 1e-3),
    f 1e-11, pL 1e-12 absolute, dy/dt 1e-7 (floor 1), 1e-4 with hydraulic lift (test_gpu_round3.py).  The flux and dy/dt
    are compared wherever the ORACLE's value is determined to a tenth of its tier (`_determined`): at an unsaturated cell
    next to saturation (|psi| of 0.005 ... 0.5 cm) S_e is 1 - 1e-9 ... 1 - 1e-5 and one rounding of it moves K by up to
    1e-10 (rhs_states.conductivity_uncertainty) -- there the tier cannot be met by any evaluation, the oracle's included,
    and no other tier is put in its place (LAB_NOTES.md section 34 has the measured figures: flux up to 5.6e-11 on the
    `range_*` states, the same from both variants, the one-wave kernels and the split column).  c, s and pL are compared
    at every cell.
(c) the diagnostics against the oracle's interior call: |d| <= 1e-11 dz sum|s_i| + 1e-11 |value| (the sink tier applied
    term by term; it dominates the reordering bound D 2^-53 sum|s_i|).  Where the sink is lateral flow alone (no
    evapo-transpiration on the row, monitoring mode) the midpoints it acts on are those of [wtd_est, wtd_obs) with
    psi > 0, wtd_est from the oracle's find_wtd.
(d) the two copies of a state give equal bytes (on a split column they sit in two wave pairs of one workgroup), and a
    split column's aux equals the one-wave kernel's of the same depth at the tiers of (b).

Nothing here steps a row or builds a library; a case takes a few seconds."""
import numpy as np
import pytest

import rhs_states as rs
from helpers import rel_err

pytestmark = pytest.mark.gpu

CHUNK = 20                      # states per launch, each twice: 40 members
QUANTITIES = ("dydt", "c", "s", "f", "pL", "diag")


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("these tests need a GPU")
    import __graft_entry__ as ge
    ge.build()
    from hydromodel_amd import stepper
    return stepper


def _evaluate(st, row, spin, variant):
    dydt, x = st.rhs(row, spinup=spin, want_aux=True, want_diag=True, variant=variant)
    return dict(x, dydt=dydt)


def _same_bytes(a, b, where, names):
    """(a): every quantity of every member, byte for byte; the message localises the first difference."""
    for q in QUANTITIES:
        x, y = np.ascontiguousarray(a[q]), np.ascontiguousarray(b[q])
        if x.tobytes() == y.tobytes():
            continue
        xb, yb = x.view(np.uint64).reshape(len(names), -1), y.view(np.uint64).reshape(len(names), -1)
        m, node = (int(v[0]) for v in np.nonzero(xb != yb))
        xv, yv = x.reshape(len(names), -1)[m, node], y.reshape(len(names), -1)[m, node]
        raise AssertionError(f"{where}, state {names[m]} (member {m}): {q}[{node}] differs: step {float(xv).hex()} ({xv!r}) "
                             f"against hook {float(yv).hex()} ({yv!r}); {int((xb != yb).sum())} entries of {q} differ in this launch")


def _launches(names, Y, Z):
    """The bank in launches of CHUNK states, each state twice as neighbouring members (the last launch padded with its
    first state): -> [(names of the members, Y, Z)]"""
    out = []
    for lo in range(0, len(names), CHUNK):
        idx = list(range(lo, min(lo + CHUNK, len(names))))
        idx += [idx[0]] * (CHUNK - len(idx))
        idx = np.repeat(idx, 2)
        out.append(([names[i] for i in idx], Y[idx], Z[idx]))
    return out


def _worst(got, ref, floor, where=None):
    """rel_err's figure with the node it comes from (`where`: the entries that count)"""
    e = np.abs(got - ref) / np.maximum(floor, np.abs(ref))
    if where is not None:
        e = np.where(where, e, 0.0)
    k = int(np.argmax(e))
    return float(e[k]), f"node {k}: {got[k]!r} against {ref[k]!r}"


def _determined(cols, y, z, ref, ra, dydt_tier):
    """-> (midpoints [D - 1], nodes [D]) at which the oracle's flux / dy/dt is determined to a tenth of its tier: the flux
    carries K's uncertainty u (two evaluations, each with S_e within an ulp: 4 u |f|), dy/dt_i that of f_i and f_{i-1}
    over h (c_i + c_{i-1}) -- the assembly of richards_pde.py:108-156 with (c, f)_{-1} = (0, -pL), (c, f)_{D-1} = 0."""
    df = 4.0 * rs.conductivity_uncertainty(cols, y, z) * np.abs(ra["f"])
    df[~np.isfinite(df)] = np.inf
    f_ok = df <= 0.1 * 1e-11 * np.maximum(1.0, np.abs(ra["f"]))
    den = 0.5 * cols.dz * (np.append(ra["c"], 0.0) + np.append(0.0, ra["c"]))
    dd = (np.append(df, 0.0) + np.append(0.0, df)) / np.where(den == 0.0, 1.0, den)
    return f_ok, dd <= 0.1 * dydt_tier * np.maximum(1.0, np.abs(ref))


def run_case(gpu, cols, forcing, rows, label, flag_sets=rs.FLAG_SETS, collect_aux=None):
    """(a) - (d) for one column on the handle layout the environment selects.
    Returns the comparisons against the oracle that missed (the caller asserts there are none)."""
    from oracle.oracle import Oracle
    D, dz, psi_sat = cols.dim_d, cols.dz, cols.soil.psi_sat
    names, Y, Z = rs.case_bank(cols)
    launches = _launches(names, Y, Z)
    counts = {"a": 0, "b": 0, "c": 0, "d": 0, "lf_sets": 0}
    seen = {"sat_in_root": 0, "transpiring": 0, "c_clamped": 0, "jstar_targets": set(), "jstar_none": 0}
    seen.update({f"lf:{r}": 0 for r, _, _ in rows})
    misses, left_out, undetermined = [], {"f": 0, "dydt": 0, "cells": 0}, {"f": 0.0, "dydt": 0.0}
    for fname, flags in flag_sets.items():
        o = Oracle(cols, forcing.surface_evap, flags=flags)
        fl = dict(cols.flags, **(flags or {}))
        st = gpu.EnsembleStepper(cols, forcing, 2 * CHUNK, flags=flags)
        for members, Yl, Zl in launches:
            st.set_state(Yl)
            for noise in ("host", "philox"):
                if noise == "host":
                    st.set_noise_host(Zl)
                else:
                    st.set_noise_philox(20 + D, 0)
                for rname, row, spin in rows:
                    where = f"{label}, flags {fname}, {noise} noise, row {rname}"
                    step, hook = _evaluate(st, row, spin, "step"), _evaluate(st, row, spin, "hook_layout")
                    _same_bytes(step, hook, where, members)                                   # (a)
                    assert st.rhs(row, spinup=spin).tobytes() == hook["dydt"].tobytes(), where   # hc_rhs is the hook
                    counts["a"] += len(set(members))
                    if noise == "philox":
                        continue                                                               # (each member has its own stream)
                    for q in QUANTITIES:                                                       # (d) the two copies
                        assert step[q][0::2].tobytes() == step[q][1::2].tobytes(), (where, q)
                    counts["d"] += len(set(members))
                    if collect_aux is not None:
                        collect_aux[(fname, rname, members[0])] = step
                    orow = rs.oracle_row(forcing, row, spin)
                    for m in range(0, len(members), 2):
                        if m >= 2 and members[m] == members[0]:
                            continue                                                           # padding
                        y, z, tag = Yl[m], Zl[m], (where, members[m])
                        ref, ra = o.rhs(orow, y, z, want_aux=True)
                        # ---- (b)  (every miss of the case is collected, so that a failure shows all of them)
                        dydt_tier = 1e-4 if fl["HLIFT"] else 1e-7
                        f_ok, d_ok = _determined(cols, y, z, ref, ra, dydt_tier)
                        left_out["f"] += int((~f_ok).sum())
                        left_out["dydt"] += int((~d_ok).sum())
                        left_out["cells"] += f_ok.size
                        for q, (err, at), tier in (("c", _worst(step["c"][m], ra["c"], 1e-7), 1e-11),
                                                   ("s", _worst(step["s"][m], ra["s"], 1e-3), 1e-11),
                                                   ("f", _worst(step["f"][m], ra["f"], 1.0, f_ok), 1e-11),
                                                   ("pL", (abs(step["pL"][m] - ra["pL"]), ""), 1e-12),
                                                   ("dydt", _worst(step["dydt"][m], ref, 1.0, d_ok), dydt_tier)):
                            if not err < tier:
                                misses.append(f"{where}, state {members[m]}: {q} {err:.2e} (tier {tier:.0e}) {at}")
                        for q, got, want, ok in (("f", step["f"][m], ra["f"], f_ok), ("dydt", step["dydt"][m], ref, d_ok)):
                            if not ok.all():                   # the figures where nothing is asserted (printed, LAB_NOTES 34)
                                undetermined[q] = max(undetermined[q], _worst(got, want, 1.0, ~ok)[0])
                        counts["b"] += 1
                        # ---- (c)
                        sum_s = float(np.abs(ra["s"]).sum())
                        for k in (0, 1):
                            want = ra["tr_lf_int"][k]
                            err, bound = abs(step["diag"][m, k] - want), 1e-11 * dz * sum_s + 1e-11 * abs(want)
                            if not err <= bound:
                                misses.append(f"{where}, state {members[m]}: diag[{k}] {step['diag'][m, k]!r} against {want!r}, "
                                              f"|d| {err:.2e} (bound {bound:.2e})")
                        counts["c"] += 1
                        ym = rs.midpoints(y)
                        et_row = fl["ET"] and not spin and forcing.daylight[row]
                        if fl["LF"] and not fl["PREDICT"] and not et_row:
                            kk = D - 2
                            est = Oracle.find_wtd(ym[1:D - 1] >= psi_sat)
                            obs = min(int(forcing.wtd_obs[row]), kk - 1)
                            acts = np.zeros(D - 1, dtype=bool)
                            acts[1 + est:1 + max(obs, est)] = True
                            assert np.array_equal(step["s"][m] != 0.0, acts & (ym > 0.0)), tag
                            assert est == min(max(rs.deepest_unsaturated(cols, y), 0), kk - 1), tag
                            counts["lf_sets"] += 1
                        # ---- the predicates of tests/test_rhs_states_cpu.py, on what the GPU ran
                        if fname == "default":
                            sat = ym >= psi_sat
                            seen[f"lf:{rname}"] += bool(step["diag"][m, 1] > 0.0)
                            seen["transpiring"] += bool(step["diag"][m, 0] > 0.0)
                            seen["c_clamped"] += bool(((step["c"][m] == max(cols.soil.epsilon, 1e-8)) & ~sat)[1:].any())
                            seen["sat_in_root"] += bool(sat[1:1 + cols.n_root_int].any())
                            j = rs.deepest_unsaturated(cols, y)
                            seen["jstar_targets"].add(j)
                            seen["jstar_none"] += j == -1
        st.close()
    if "default" in flag_sets:
        assert all(seen[f"lf:{r}"] >= 1 for r, _, _ in rows), seen
        assert seen["transpiring"] >= 1 and seen["c_clamped"] >= 1 and seen["sat_in_root"] >= 1 and seen["jstar_none"] >= 1, seen
        assert set(rs.ballot_targets(D)) <= seen["jstar_targets"]
    print(f"[{label}] {len(names)} states x {len(rows)} rows x {len(flag_sets)} flag sets: (a) {counts['a']} (state, row, flags, noise) cases, "
          f"(b) {counts['b']}, (c) {counts['c']} and (d) {counts['d']} (state, row, flags) cases, "
          f"lateral-flow index sets {counts['lf_sets']}; {len(misses)} misses; the oracle's flux / dy/dt not determined to a tenth "
          f"of the tier at {left_out['f']} / {left_out['dydt']} of {left_out['cells']} cells (differences there: "
          f"{undetermined['f']:.1e} / {undetermined['dydt']:.1e})")
    # the cut leaves the comparison whole: at most 2 % of the cells (a sixth of the two range states' and one of `thr_below`)
    assert left_out["f"] <= 0.03 * left_out["cells"] and left_out["dydt"] <= 0.03 * left_out["cells"], left_out
    return misses


def _none_missed(misses):
    assert not misses, f"{len(misses)} comparisons against the oracle miss their tier:\n  " + "\n  ".join(misses[:40])


@pytest.mark.parametrize("D", rs.DEPTHS_DEFAULT)
def test_default_exponents(gpu, D):
    cols, forcing, rows = rs.case_column(D)
    assert rs.cells_per_lane(D) in (4, 5, 6, 7)
    _none_missed(run_case(gpu, cols, forcing, rows, f"D = {D}"))


@pytest.mark.parametrize("D", rs.DEPTHS_SPLIT)
def test_split_column(gpu, D, monkeypatch):
    """Both layouts of a deep column: the split-column kernel (two-waves-per-SIMD instantiation on both halves, the water
    table found on each before the mailbox exchange) and, with the split off, the one-wave kernel of 9 / 10 cells per
    lane, where the two variants are one kernel.  (d): the split column's aux against the one-wave kernel's."""
    cols, forcing, rows = rs.case_column(D)
    aux = {}
    for mode in ("split", "one-wave"):
        monkeypatch.setenv("HYDROCOL_SPLIT_COLUMN", "0" if mode == "one-wave" else "1")
        aux[mode] = {}
        _none_missed(run_case(gpu, cols, forcing, rows, f"D = {D} ({mode})", collect_aux=aux[mode]))
    assert aux["split"].keys() == aux["one-wave"].keys() and len(aux["split"]) > 0
    for key, a in aux["split"].items():
        b = aux["one-wave"][key]
        assert rel_err(a["c"], b["c"], 1e-7) < 1e-11 and rel_err(a["s"], b["s"], 1e-3) < 1e-11, key
        assert rel_err(a["f"], b["f"]) < 1e-11 and np.max(np.abs(a["pL"] - b["pL"])) < 1e-12, key
        assert rel_err(a["dydt"], b["dydt"]) < (1e-4 if key[0] == "hlift" else 1e-7), key


@pytest.mark.parametrize("D", rs.DEPTHS_GENERIC)
@pytest.mark.parametrize("model,n,lam", rs.GENERIC)
def test_generic_exponents(gpu, D, model, n, lam):
    cols, forcing, rows = rs.case_column(D, model=model, n=n, lam=lam)
    _none_missed(run_case(gpu, cols, forcing, rows, f"D = {D}, {model} n = {n} lambda = {lam}"))


@pytest.mark.parametrize("D", rs.DEPTHS_CRAFTED)
def test_crafted_tables(gpu, D):
    """Cells outside every layer and the uptake's tot_x > 1 renormalisation (rhs_states.crafted_column)."""
    cols, forcing, rows = rs.case_column(D, crafted=True)
    _none_missed(run_case(gpu, cols, forcing, rows, f"D = {D}, crafted tables"))


def test_where_the_step_kernel_is_the_plain_kernel_the_variants_are_one_kernel(gpu):
    """8 cells per lane: two_of is false, "step" adds no kernel -- the comparison (a) must hold trivially, and (b), (c) check
    the hook as before."""
    cols, forcing, rows = rs.case_column(rs.DEPTH_PLAIN)
    assert rs.cells_per_lane(rs.DEPTH_PLAIN) == 8
    _none_missed(run_case(gpu, cols, forcing, rows, f"D = {rs.DEPTH_PLAIN}"))


def test_unknown_variant_is_an_error(gpu):
    from hydromodel_amd import _lib
    cols, forcing, _ = rs.case_column(200)
    st = gpu.EnsembleStepper(cols, forcing, 1)
    st.set_state(cols.z - 300.0)
    st.set_noise_host(np.zeros((1, cols.dim_d)))
    out = np.empty((1, cols.dim_d))
    assert st.lib.hc_rhs_ex(st.h, 2, 0, 7, _lib.dptr(out), None, None) != 0
    assert b"variant" in st.lib.hc_last_error()
    st.close()
