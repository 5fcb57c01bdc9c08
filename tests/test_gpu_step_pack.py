"""Two stepped days with the packed cell model of the 5-cells-per-lane kernel (csrc/hc_device.h, rhs_eval: HC_MODEL_PACK)
and with HYDROCOL_MODEL_PACK=0, the full evaluation forced in the same binary: the same bytes everywhere.

D = 300, 512 members, hydrostatic columns with the water table spread over nodes 60 .. 100 -- on both sides of midpoint 80,
where the packed path ends (tests/test_rhs_pack_states_cpu.py checks the spread) -- through 96 rows: daylight and night,
refresh rows included.  The member states, the noise damping, the moment table, the per-row water-table indices and the
solver statistics must agree byte for byte.  That both paths were taken is a condition on the states the kernel classified,
not a measurement: members that start AND end with every unsaturated cell inside the packed row, members that start and
end outside it, and members that cross the boundary during the run."""
import numpy as np
import pytest

import rhs_pack_states as ps
import rhs_states as rs

pytestmark = pytest.mark.gpu
N, ROWS = 512, 96


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("these tests need a GPU")
    import __graft_entry__ as ge
    ge.build()
    from hydromodel_amd import stepper
    return stepper


def _run(gpu, cols, forcing, psi):
    st = gpu.EnsembleStepper(cols, forcing, N)
    st.set_state(psi)
    st.set_noise_philox(77, 0)
    out = st.step_rows(1, ROWS, want_wtd=True, want_stats=True)
    res = {"psi": st.get_state(), "noise_scale": st.noise_scale(), "moments": np.asarray(st.moments()),
           "wtd": out["wtd"], "stats": out["stats"], "failed": out["failed"], "counters": st.counters()}
    st.close()
    return res


def test_two_days_with_and_without_the_packed_path(gpu, monkeypatch):
    from hydromodel_amd.digest import ColumnTables, ForcingDigest
    from hydromodel_amd.synthetic import default_parameters, synthetic_forcing_frame, synthetic_well
    params = default_parameters()
    cols = ColumnTables(params, synthetic_well(300))
    forcing = ForcingDigest(params, synthetic_forcing_frame(1), cols)
    assert rs.cells_per_lane(cols.dim_d) == ps.CPL
    sl = slice(1, 1 + ROWS)
    assert forcing.daylight[sl].any() and not forcing.daylight[sl].all() and forcing.refresh[sl].any()
    psi = ps.hydrostatic_spread(cols, N)
    monkeypatch.delenv("HYDROCOL_MODEL_PACK", raising=False)
    on = _run(gpu, cols, forcing, psi)
    monkeypatch.setenv("HYDROCOL_MODEL_PACK", "0")
    off = _run(gpu, cols, forcing, psi)
    assert on["counters"] == off["counters"], (on["counters"], off["counters"])
    for q in ("psi", "noise_scale", "moments", "wtd", "stats", "failed"):
        assert np.ascontiguousarray(on[q]).tobytes() == np.ascontiguousarray(off[q]).tobytes(), q
    assert np.isfinite(on["psi"]).all()
    # both paths were taken: by the predicate the kernel branches on, at the states it started from and ended in
    start = np.array([ps.takes_packed_path(cols, y) for y in psi])
    end = np.array([ps.takes_packed_path(cols, y) for y in on["psi"]])
    print(f"packed at the start / at the end: {int(start.sum())} / {int(end.sum())} of {N} members; "
          f"crossed: {int((start != end).sum())}; water-table index at the row ends {on['wtd'].min()} .. {on['wtd'].max()}")
    assert (start & end).sum() >= 1 and (~start & ~end).sum() >= 1 and (start != end).sum() >= 1
