"""The assimilation tables through a checkpoint with every option of an owner on at once (stepper.ASSIM_TABLES): a
particle filter with sensors, tempering, rejuvenation and a window, and an EnKF with sensors, a window, the square-root
scheme, relaxation and the noise field.  A run dumped between a lagged row and its assimilation row continues to the bit
of the unbroken run, every table of the owner included; the checkpoint holds exactly the keys written out below, and a
run with the owner alone holds none of the options' keys."""
import numpy as np
import pytest

from helpers import digest, golden
from test_gpu_enkf import _spread

pytestmark = pytest.mark.gpu
N, ROWS, CUT, STRIDE, OFFSETS = 64, 96, 36, 24, (6, 12)         # the dump after row 36 = 48 - 12: captured, rows 42 and 48 ahead
DEPTHS_CM = (30.0, 225.0)

BASE_KEYS = ("psi", "noise_scale", "moments", "next_row", "seed", "member_offset", "n_members", "dim_d", "dim_t",
             "initial_cond")
# the keys a dump of the commit before the registry held (EnsembleSimulation.dump, one hand-written line each)
OWNER_KEYS = {"filter": ("filter_stride", "filter_sigma_cm", "filter_seed", "filter_table", "filter_base"),
              "enkf": ("enkf_stride", "enkf_sigma_cm", "enkf_localisation_cm", "enkf_seed", "enkf_table")}
OPTION_KEYS = {"filter": ("filter_sm_nodes", "filter_sm_table", "filter_ess_floor", "filter_temper_table",
                          "filter_rejuvenation", "filter_rejuvenation_table", "filter_window_offsets",
                          "filter_window_table", "filter_window_index", "filter_window_rows"),
               "enkf": ("enkf_method", "enkf_relaxation", "enkf_sm_nodes", "enkf_sm_table", "enkf_window_offsets",
                        "enkf_window_table", "enkf_window_y", "enkf_window_rows", "enkf_noise_relaxation",
                        "enkf_noise_table", "enkf_noise_base")}
TABLES = {"filter": ("filter", "filter_sm", "filter_temper", "filter_rejuvenation", "filter_window"),
          "enkf": ("enkf", "enkf_sm", "enkf_window", "enkf_noise")}


def _record(cols, T):
    from hydromodel_amd.stepper import soil_moisture_record
    v = np.full((T, len(DEPTHS_CM)), np.nan)
    v[STRIDE::STRIDE] = (0.24, 0.36)
    v[2 * STRIDE, 1] = np.nan                                   # one sensor silent on row 48
    return soil_moisture_record(cols.z, DEPTHS_CM, v, (0.05, 0.08))


def _settings(owner, cols, forcing, options=True):
    rec = _record(cols, forcing.dim_t)
    if owner == "filter":
        kw = dict(filter_stride=STRIDE, filter_sigma_cm=2.0 * cols.dz, filter_seed=11)
        if options:
            kw.update(filter_soil_moisture=rec, filter_ess_floor=0.5, filter_rejuvenation=0.98,
                      filter_window_offsets=OFFSETS)
    else:
        kw = dict(enkf_stride=STRIDE, enkf_sigma_cm=2.0 * cols.dz, enkf_seed=11)
        if options:
            kw.update(enkf_soil_moisture=rec, enkf_window_offsets=OFFSETS, enkf_method="sqrt", enkf_relaxation=0.5,
                      enkf_noise_field=True)
    return kw, ({owner + "_soil_moisture": rec} if options else {})


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _state(sim, owner):
    base = sim.stepper.filter_base() if owner == "filter" else sim.stepper.enkf_noise_base()
    out = {"psi": sim.stepper.get_state(), "moments": sim.moments(), "base": base}
    out.update((key + "_table", getattr(sim, key + "_table")()) for key in TABLES[owner])
    return out


def _checkpoint_keys(path):
    from hydromodel_amd import hdf5io
    return set(np.load(path).files) if path.suffix == ".npz" else set(hdf5io.read(path))


@pytest.mark.parametrize("owner", ["filter", "enkf"])
def test_every_option_at_once_resumes_bit_for_bit_with_the_key_set_of_before(owner, tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(1)
    psi0 = _spread(golden("g1_tables_1.npz")["initial_cond"], N)
    kw, again = _settings(owner, cols, forcing)
    whole = EnsembleSimulation(cols, forcing, N, seed=6, psi0=psi0, **kw)
    try:
        whole.advance(ROWS)
        want = _state(whole, owner)
    finally:
        whole.close()
    first = EnsembleSimulation(cols, forcing, N, seed=6, psi0=psi0, **kw)
    try:
        first.advance(CUT)
        capture = getattr(first.stepper, owner + "_window_capture")()
        assert CUT in capture[1].tolist()                       # offset 12's row 36 is held for row 48: the capture is live
        path = first.dump(tmp_path / "ck.h5")
    finally:
        first.close()
    assert _checkpoint_keys(path) == set(BASE_KEYS + OWNER_KEYS[owner] + OPTION_KEYS[owner])
    back = EnsembleSimulation.restore(path, cols, forcing, **again)
    try:
        assert back.next_row == CUT + 1
        held = getattr(back.stepper, owner + "_window_capture")()
        assert all(_bits(a).tobytes() == _bits(b).tobytes() for a, b in zip(capture, held))
        back.advance(ROWS - CUT)
        got = _state(back, owner)
    finally:
        back.close()
    for key in want:
        a, b = _bits(want[key]), _bits(got[key])
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), key
    for key in TABLES[owner]:                                    # every table took part: none is the untouched NaN fill
        assert np.isfinite(want[key + "_table"]).any(), key
    assert (want[owner + "_table"][1:5, 0] > 0).all()            # rows 24, 48, 72, 96 were assimilated


@pytest.mark.parametrize("owner", ["filter", "enkf"])
def test_the_owner_alone_writes_none_of_the_option_keys(owner, tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(1)
    psi0 = _spread(golden("g1_tables_1.npz")["initial_cond"], N)
    kw, _ = _settings(owner, cols, forcing, options=False)
    sim = EnsembleSimulation(cols, forcing, N, seed=6, psi0=psi0, **kw)
    try:
        sim.advance(STRIDE)
        path = sim.dump(tmp_path / "ck.h5")
    finally:
        sim.close()
    assert _checkpoint_keys(path) == set(BASE_KEYS + OWNER_KEYS[owner])
