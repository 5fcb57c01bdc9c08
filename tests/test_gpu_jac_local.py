"""The three FD-Jacobian column groups of the 5-cells-per-lane step kernel (csrc/hc_step.h, JAC3) against the host's five,
forced in the same binary with HYDROCOL_JAC_LOCAL3=0: the same bytes everywhere.

On a row whose RHS is local (night, spin-up, ET off) and whose water-table search no FD step can move, the kernel evaluates
the groups i % 3 instead of scipy's five (tests/test_jac_local_groups_cpu.py holds the claim on the oracle).  Here the kernel
itself: D = 257, 300 and 320 (the edges and the middle of 5 cells per lane), 384 members through 96 rows of the synthetic
record -- two nights, two days, refresh rows, rain rows -- with the switch on and at 0.  States, noise scales, moments,
per-row water-table indices, per-row solver statistics, failed attempts and counters must agree byte for byte.

Members: the constructions of tests/rhs_pack_states.py -- water tables at every midpoint 70 .. 84, a perched lens, a dry and
a saturated column, threshold midpoints AT psi_sat and one ulp below it -- and, next to them, threshold midpoints within one
FD step of psi_sat (psi_sat (1 +- 1e-9): sqrt(eps) |y| is 1.5e-8 |y|), which the guard must hand to the five groups; the rest
are hydrostatic columns with the water table spread over nodes 60 .. 100.

Handles: the default flags at the three depths; at D = 300 also ET off (every row local), LF off, HLIFT on, PREDICT on,
HYDROCOL_MODEL_PACK=0, a per-member spin-up (iteration counts equal member by member), a small iteration budget (the
attempts that end on the budget end there in both settings: the same guard trips, the same failed attempts), and the FD
retry pass forced by the debug threshold, with and without a budget."""
import numpy as np
import pytest

import rhs_pack_states as ps
import rhs_states as rs

pytestmark = pytest.mark.gpu
N, ROWS = 384, 96


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("these tests need a GPU")
    import __graft_entry__ as ge
    ge.build()
    from hydromodel_amd import stepper
    return stepper


_COLUMNS = {}


def _column(D):
    if D not in _COLUMNS:
        from hydromodel_amd.digest import ColumnTables, ForcingDigest
        from hydromodel_amd.synthetic import default_parameters, synthetic_forcing_frame, synthetic_well
        params = default_parameters()
        cols = ColumnTables(params, synthetic_well(D))
        forcing = ForcingDigest(params, synthetic_forcing_frame(1), cols)
        assert rs.cells_per_lane(cols.dim_d) == ps.CPL and cols.n_groups == 5
        sl = slice(1, 1 + ROWS)
        day = forcing.daylight[sl].astype(bool)
        assert day.any() and not day.all() and forcing.refresh[sl].any() and (forcing.precip[sl] != 0).any()
        _COLUMNS[D] = (cols, forcing, _members(cols))
    return _COLUMNS[D]


def _members(cols):
    """[N][D]: the crafted states first, hydrostatic columns behind them."""
    psi_sat = cols.soil.psi_sat
    _, Y, _, _ = ps.pack_states(cols)
    near = [ps.threshold(cols, a, psi_sat * (1.0 + s * 1e-9)) for a in (ps.PACK_END - 6, ps.PACK_END) for s in (-1.0, 1.0)]
    crafted = np.concatenate([Y, np.array(near)])
    # what the crafted part must contain
    deepest = [rs.deepest_unsaturated(cols, y) for y in Y]
    assert set(ps.WT_TARGETS) <= set(deepest)
    mids = [rs.midpoints(y) for y in crafted]
    assert any((m == psi_sat).any() for m in mids) and any((m == np.nextafter(psi_sat, -np.inf)).any() for m in mids)
    assert all((np.abs(rs.midpoints(y) / psi_sat - 1.0) < 2e-9).any() for y in near)
    return np.concatenate([crafted, ps.hydrostatic_spread(cols, N - len(crafted))])


def _run(gpu, D, flags=None, budget=0):
    cols, forcing, psi = _column(D)
    st = gpu.EnsembleStepper(cols, forcing, N, flags=flags)
    if budget:
        st.set_iteration_budget(budget)
    st.set_state(psi)
    st.set_noise_philox(77, 0)
    out = st.step_rows(1, ROWS, want_wtd=True, want_stats=True)
    res = {"psi": st.get_state(), "noise_scale": st.noise_scale(), "moments": np.asarray(st.moments()),
           "wtd": out["wtd"], "stats": out["stats"], "failed": out["failed"], "counters": st.counters()}
    st.close()
    return res


COUNTED = ("jac_retry", "failed_attempts", "guard_trips")     # (guard_last_*: the last writer among the waves wins, run by run)


def _counts(counters):
    return {k: counters[k] for k in COUNTED}


def _same(on, off, what):
    assert _counts(on["counters"]) == _counts(off["counters"]), (what, on["counters"], off["counters"])
    for q in ("psi", "noise_scale", "moments", "wtd", "stats", "failed"):
        assert np.ascontiguousarray(on[q]).tobytes() == np.ascontiguousarray(off[q]).tobytes(), (what, q)


def _both(gpu, monkeypatch, D, **kw):
    monkeypatch.delenv("HYDROCOL_JAC_LOCAL3", raising=False)
    on = _run(gpu, D, **kw)
    monkeypatch.setenv("HYDROCOL_JAC_LOCAL3", "0")
    off = _run(gpu, D, **kw)
    return on, off


@pytest.mark.parametrize("D", ps.DEPTHS)
def test_two_days_on_three_groups_and_on_five(gpu, monkeypatch, D):
    on, off = _both(gpu, monkeypatch, D)
    _same(on, off, f"D = {D}")
    solved = on["stats"][:, :, 3] > 0
    print(f"D = {D}: rows with accepted steps {int(solved.sum())} of {solved.size}, failed attempts "
          f"{on['counters']['failed_attempts']}, FD retry passes {on['counters']['jac_retry']}, "
          f"water-table index {on['wtd'].min()} .. {on['wtd'].max()}")
    assert solved.any() and np.isfinite(on["psi"][len(on["psi"]) // 2:]).all()


@pytest.mark.parametrize("name,flags", [("et_off", {"ET": False}), ("lf_off", {"LF": False}), ("hlift", {"HLIFT": True}),
                                        ("predict", {"PREDICT": True})])
def test_flag_sets(gpu, monkeypatch, name, flags):
    on, off = _both(gpu, monkeypatch, 300, flags=flags)
    _same(on, off, name)


def test_without_the_packed_cell_model(gpu, monkeypatch):
    monkeypatch.setenv("HYDROCOL_MODEL_PACK", "0")
    on, off = _both(gpu, monkeypatch, 300)
    _same(on, off, "HYDROCOL_MODEL_PACK=0")


def test_a_small_iteration_budget_ends_the_same_attempts(gpu, monkeypatch):
    # an ordinary attempt takes a few dozen phase-loop trips: a budget inside that range ends some attempts and not others
    hits = []
    for budget in (24, 40):
        on, off = _both(gpu, monkeypatch, 300, budget=budget)
        _same(on, off, f"budget {budget}")
        hits.append(on["counters"]["guard_trips"])
    print(f"guard trips at budgets 24 / 40: {hits}")
    assert hits[0] > 0


@pytest.mark.parametrize("reject", [1e-2, 0.3])
def test_the_retry_pass_finishes_in_the_grouping_it_began_with(gpu, monkeypatch, reject):
    """num_jac's retry pass (columns that moved f by too little, again with a 10x step) never runs with the real threshold:
    the debug hook raises it (as tests/test_gpu_parity.py does against the oracle).  With a budget on top, the trips of the
    retry pass count as the host's groups would have taken them."""
    monkeypatch.setenv("HYDROCOL_DEBUG_JAC_REJECT", repr(reject))
    for budget in (0, 60):
        on, off = _both(gpu, monkeypatch, 300, budget=budget)
        _same(on, off, f"reject {reject}, budget {budget}")
        print(f"reject {reject}, budget {budget}: FD retry passes {on['counters']['jac_retry']}, guard trips "
              f"{on['counters']['guard_trips']}, failed attempts {on['counters']['failed_attempts']}")
        assert on["counters"]["jac_retry"] > 0


def test_spinup_iteration_counts(gpu, monkeypatch):
    cols, forcing, _ = _column(300)
    from hydromodel_amd.ensemble import pressure_head
    y0, _ = pressure_head(cols, cols.por_raw)
    res = []
    for switch in (None, "0"):
        if switch is None:
            monkeypatch.delenv("HYDROCOL_JAC_LOCAL3", raising=False)
        else:
            monkeypatch.setenv("HYDROCOL_JAC_LOCAL3", switch)
        st = gpu.EnsembleStepper(cols, forcing, 16)
        st.set_state(y0)
        st.set_noise_philox(5, 0)
        iters, _ = st.spinup(forcing.zwtd_cm[0], cols.z[0], max_iterations=400)
        res.append((iters.copy(), st.get_state(), st.counters()))
        st.close()
    (it_on, y_on, c_on), (it_off, y_off, c_off) = res
    print(f"spin-up iterations: {it_on.tolist()}")
    assert (it_on == it_off).all() and y_on.tobytes() == y_off.tobytes() and _counts(c_on) == _counts(c_off)
    assert (it_on != 0).all()
