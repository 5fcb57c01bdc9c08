"""The step kernel of 5 cells per lane with its RHS's latency chains side by side (csrc/hc_device.h, HC_RHS_ILP) against
the kernel before that change: 256 members through 96 rows at D = 300, compared BYTE FOR BYTE with recorded values.

HC_RHS_ILP moves independent instructions of `rhs_eval` (the five divisions of the assembly of dy/dt line by line across
the cells; table reads of the two ET calls issued earlier and together); no statement's arithmetic changes and the unit is
compiled with -ffp-contract=on, so every byte the kernel returns must be the earlier kernel's.

Members: the constructions of tests/rhs_pack_states.py -- water tables at every midpoint 70 .. 84 (both sides of the
lane-15/16 boundary: the packed and the full cell model), a perched lens inside and across the boundary, a dry and a saturated
column, threshold midpoints at psi_sat and one ulp below it -- and hydrostatic columns with the water table spread over nodes
60 .. 100 behind them.  Rows 1 .. 96 of the synthetic record: two nights, two days, refresh rows, rain rows.  Philox noise.

Compared: states, noise scales, moments, per-row water-table indices, per-row solver statistics, failed attempts, and the
counters that do not depend on the order in which waves finish.

tests/golden/g43_step_ilp_300.npz was recorded on an MI355X by this file (`python tests/test_gpu_step_ilp.py <library>
<out.npz>`) from the library of commit 22568a7 ("Run settings: one definition from constructor to checkpoint to CLI"), the
parent of the commit that introduced HC_RHS_ILP."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N, ROWS, D = 256, 96, 300
GOLDEN = "g43_step_ilp_300.npz"
ARRAYS = ("psi", "noise_scale", "moments", "wtd", "stats", "failed")
COUNTED = ("jac_retry", "failed_attempts", "guard_trips")     # (guard_last_*: the last writer among the waves wins, run by run)


def _case():
    import rhs_pack_states as ps
    import rhs_states as rs
    from hydromodel_amd.digest import ColumnTables, ForcingDigest
    from hydromodel_amd.synthetic import default_parameters, synthetic_forcing_frame, synthetic_well
    params = default_parameters()
    cols = ColumnTables(params, synthetic_well(D))
    forcing = ForcingDigest(params, synthetic_forcing_frame(1), cols)
    assert rs.cells_per_lane(cols.dim_d) == ps.CPL
    day = forcing.daylight[1:1 + ROWS].astype(bool)
    assert day.any() and not day.all() and forcing.refresh[1:1 + ROWS].any() and (forcing.precip[1:1 + ROWS] != 0).any()
    _, Y, _, claims = ps.pack_states(cols)
    packed = [p for _, p in claims.values()]
    assert any(packed) and not all(packed)                      # both sides of the boundary
    assert set(ps.WT_TARGETS) <= {rs.deepest_unsaturated(cols, y) for y in Y}
    psi = np.concatenate([Y, ps.hydrostatic_spread(cols, N - len(Y))])
    assert psi.shape == (N, D)
    return cols, forcing, psi


def run(stepper):
    """-> {name: array}: what 96 rows leave behind"""
    cols, forcing, psi = _case()
    st = stepper.EnsembleStepper(cols, forcing, N)
    st.set_state(psi)
    st.set_noise_philox(43, 0)
    out = st.step_rows(1, ROWS, want_wtd=True, want_stats=True)
    counters = st.counters()
    res = {"psi": st.get_state(), "noise_scale": st.noise_scale(), "moments": np.asarray(st.moments()),
           "wtd": np.asarray(out["wtd"]), "stats": np.asarray(out["stats"]), "failed": np.asarray(out["failed"]),
           "counted": np.array([int(counters[k]) for k in COUNTED], dtype=np.int64)}
    st.close()
    return res


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("these tests need a GPU")
    import __graft_entry__ as ge
    ge.build()
    from hydromodel_amd import stepper
    return stepper


def test_96_rows_give_the_recorded_bytes(gpu):
    from helpers import golden
    want = golden(GOLDEN)
    got = run(gpu)
    assert int(want["members"]) == N and int(want["rows"]) == ROWS and int(want["depth"]) == D
    assert np.isfinite(got["psi"]).all()
    assert dict(zip(COUNTED, got["counted"].tolist())) == dict(zip(COUNTED, want["counted"].tolist()))
    for q in ARRAYS:
        a, b = np.ascontiguousarray(got[q]), np.ascontiguousarray(want[q])
        assert a.dtype == b.dtype and a.shape == b.shape, (q, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            diff = np.nonzero(a.reshape(-1).view(np.uint8).reshape(a.size, -1) != b.reshape(-1).view(np.uint8).reshape(b.size, -1))[0]
            k = np.unravel_index(int(diff[0]), a.shape)
            raise AssertionError(f"{q}{list(k)} differs from the recorded value: {a[k]!r} against {b[k]!r}; "
                                 f"{len(set(diff.tolist()))} of {a.size} entries differ")


if __name__ == "__main__":       # record: python tests/test_gpu_step_ilp.py <libhydrocol.so> <out.npz>
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import pathlib
    from hydromodel_amd import _lib
    _lib.LIB_PATH = pathlib.Path(sys.argv[1]).resolve()
    from hydromodel_amd import stepper
    res = run(stepper)
    np.savez_compressed(sys.argv[2], members=N, rows=ROWS, depth=D, kernels=_lib.kernel_hash(), **res)
    print(sys.argv[2], os.path.getsize(sys.argv[2]), "bytes;", {k: (v.dtype.str, v.shape) for k, v in res.items()},
          dict(zip(COUNTED, res["counted"].tolist())))
