"""A checkpoint across the families of options: each of the four datasets that can carry the members' base noise vectors
(settings.base_carrier: the filter's, the EnKF noise field's, the correlated field's, or none but ``noise_scale``) with every
diagnostic table, the perturbed forcing and, where it is allowed, the noise correlation on at once.  A run dumped after
row 36, inside the first period, continues to the bit of the unbroken run, and the checkpoint holds exactly the union of
the key lists the families' own tests write out."""
import numpy as np
import pytest

from helpers import digest, golden
from test_gpu_assim_tables import BASE_KEYS, OWNER_KEYS, _settings
from test_gpu_diag_tables import DATASETS, SETTING_KEYS, SETTINGS
from test_gpu_enkf import _spread

pytestmark = pytest.mark.gpu
N, ROWS, CUT = 64, 96, 36
CORRELATION = {"length_cm": 50.0, "layers": True}
PERTURBATION = {"precipitation_sigma": 0.3, "demand_sigma": 0.1, "correlation_days": 3.0, "seed": 5}
NOISE_KEYS = ("noise_correlation_length_cm", "noise_correlation_layers", "noise_correlation_a", "noise_correlation_b")
FORCING_KEYS = ("forcing_precipitation_sigma", "forcing_demand_sigma", "forcing_correlation_days", "forcing_seed",
                "forcing_state", "forcing_state_day")
# carrier -> (the options beside the diagnostics and the perturbed forcing, the keys they add to the checkpoint)
CASES = {"filter_base": (lambda c, f: dict(_settings("filter", c, f, options=False)[0], noise_correlation=CORRELATION),
                         OWNER_KEYS["filter"] + NOISE_KEYS),
         "enkf_noise_base": (lambda c, f: dict(_settings("enkf", c, f, options=False)[0], enkf_noise_field=True,
                                               noise_correlation=CORRELATION),
                             OWNER_KEYS["enkf"] + ("enkf_noise_relaxation", "enkf_noise_table", "enkf_noise_base") + NOISE_KEYS),
         "noise_field_base": (lambda c, f: dict(noise_correlation=CORRELATION), NOISE_KEYS + ("noise_field_base",)),
         "noise_scale": (lambda c, f: {}, ())}


def _bytes(a):
    a = np.ascontiguousarray(a)
    return a.dtype.str, a.shape, a.tobytes()


def _state(sim, carrier):
    st = sim.stepper
    out = {"psi": st.get_state(), "moments": sim.moments(), "base": getattr(st, carrier)()}
    out["forcing_state"], out["forcing_day"] = st.forcing_state()
    out.update(("diag " + key, st.diag_raw(key)) for key in sim.diag_tables_on())
    out.update(("assim " + key, st.assim_table(key)) for key in sim.assim_tables_on())
    return {k: _bytes(v) for k, v in out.items()}


@pytest.mark.parametrize("carrier", list(CASES))
def test_a_run_across_the_families_resumes_bit_for_bit_with_the_union_of_their_keys(carrier, tmp_path):
    from hydromodel_amd import hdf5io, settings
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(1)
    psi0 = _spread(golden("g1_tables_1.npz")["initial_cond"], N)
    options, keys = CASES[carrier]
    kw = dict(options(cols, forcing), forcing_perturbation=PERTURBATION, **SETTINGS)
    whole = EnsembleSimulation(cols, forcing, N, seed=6, psi0=psi0, **kw)
    try:
        assert settings.base_carrier(whole.on) == carrier and len(whole.diag_tables_on()) == 12
        whole.advance(ROWS)
        want = _state(whole, carrier)
    finally:
        whole.close()
    first = EnsembleSimulation(cols, forcing, N, seed=6, psi0=psi0, **kw)
    try:
        first.advance(CUT)
        held = _state(first, carrier)
        path = first.dump(tmp_path / "ck.h5")
    finally:
        first.close()
    data = set(np.load(path).files) if path.suffix == ".npz" else set(hdf5io.read(path))
    assert data == set(BASE_KEYS + SETTING_KEYS + FORCING_KEYS + keys) | set(DATASETS)
    back = EnsembleSimulation.restore(path, cols, forcing)
    try:
        assert back.next_row == CUT + 1 and _state(back, carrier) == held          # installed as it was held ...
        back.advance(ROWS - CUT)
        got = _state(back, carrier)
    finally:
        back.close()
    assert got.keys() == want.keys()
    for key in want:                                                              # ... and continued to the unbroken run's
        assert got[key] == want[key], key
    tables = [k for k in want if k.startswith("diag ") and not k.endswith("_acc")]      # (row 96 ends a period: those are reset)
    assert want != held and all(np.frombuffer(want[k][2], np.uint8).any() for k in tables)
