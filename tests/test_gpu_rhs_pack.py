"""The packed cell model of the 5-cells-per-lane step kernel (csrc/hc_device.h, rhs_eval: HC_MODEL_PACK) against the full
evaluation, BIT FOR BIT, on states on both sides of its boundary -- tests/rhs_pack_states.py, whose claims
tests/test_rhs_pack_states_cpu.py proves on the CPU.

`hc_rhs_ex` variant "step" runs the step kernel's own instantiation of rhs_eval (the one that can take the packed path),
variant "hook_layout" the plain one (which never does).  Per depth (257, 300, 320: the edges and the middle of 5 cells per
lane), on the site's tables and on the crafted ones (cells of no layer inside the packed row and in the saturated zone, where
the packed path reads K from its table), on the bank's night, day and spin-up rows and the flag sets default, no_et, no_lf
and hlift:

(a) "step" against "hook_layout": dy/dt, c, s, f, pL and the diagnostics byte for byte;
(b) "step" against the CPU oracle, at the tiers of tests/test_gpu_rhs_as_stepped.py -- its `run_case`, unchanged, on the
    joint bank (rhs_states' states, so that its coverage conditions hold, followed by the boundary states);
(c) "step" with HYDROCOL_MODEL_PACK=0 (the full evaluation forced in the same binary): byte for byte what it is without.

Nothing here steps a row or builds a library; a case takes a few seconds."""
import numpy as np
import pytest

import rhs_pack_states as ps
import rhs_states as rs
import test_gpu_rhs_as_stepped as base

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("these tests need a GPU")
    import __graft_entry__ as ge
    ge.build()
    from hydromodel_amd import stepper
    return stepper


@pytest.mark.parametrize("crafted", (False, True), ids=("site", "crafted"))
@pytest.mark.parametrize("D", ps.DEPTHS)
def test_packed_against_plain_and_oracle(gpu, D, crafted, monkeypatch):
    """(a) and (b)"""
    cols, forcing, rows = rs.case_column(D, crafted=crafted)
    assert rs.cells_per_lane(D) == ps.CPL
    monkeypatch.setattr(rs, "case_bank", lambda c, _bank=rs.case_bank: _joint(c, _bank))
    label = f"D = {D}{', crafted tables' if crafted else ''}, packed cell model"
    base._none_missed(base.run_case(gpu, cols, forcing, rows, label, flag_sets=ps.FLAG_SETS))


def _joint(cols, rs_bank):
    n0, Y0, Z0 = rs_bank(cols)
    n1, Y1, Z1, _ = ps.pack_states(cols)
    return list(n0) + list(n1), np.concatenate([Y0, Y1]), np.concatenate([Z0, Z1])


def _step_outputs(gpu, cols, forcing, rows, Y, Z, flags):
    st = gpu.EnsembleStepper(cols, forcing, len(Y), flags=flags)
    st.set_state(Y)
    st.set_noise_host(Z)
    out = {}
    for rname, row, spin in rows:
        dydt, x = st.rhs(row, spinup=spin, want_aux=True, want_diag=True, variant="step")
        out[rname] = dict(x, dydt=dydt)
    st.close()
    return out


@pytest.mark.parametrize("crafted", (False, True), ids=("site", "crafted"))
@pytest.mark.parametrize("D", ps.DEPTHS)
def test_the_off_switch_gives_the_same_bytes(gpu, D, crafted, monkeypatch):
    """(c): the variable is read when the handle is made."""
    cols, forcing, rows = rs.case_column(D, crafted=crafted)
    names, Y, Z = ps.pack_bank(cols)
    for fname, flags in ps.FLAG_SETS.items():
        monkeypatch.delenv("HYDROCOL_MODEL_PACK", raising=False)
        on = _step_outputs(gpu, cols, forcing, rows, Y, Z, flags)
        monkeypatch.setenv("HYDROCOL_MODEL_PACK", "0")
        off = _step_outputs(gpu, cols, forcing, rows, Y, Z, flags)
        for rname in on:
            for q in base.QUANTITIES:
                a, b = np.ascontiguousarray(on[rname][q]), np.ascontiguousarray(off[rname][q])
                if a.tobytes() != b.tobytes():
                    m = int(np.nonzero((a.reshape(len(names), -1).view(np.uint64) != b.reshape(len(names), -1).view(np.uint64)).any(axis=1))[0][0])
                    raise AssertionError(f"D = {D}, flags {fname}, row {rname}: {q} of state {names[m]} differs with HYDROCOL_MODEL_PACK=0")
