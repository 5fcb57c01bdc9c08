"""The diagnostic tables through a checkpoint with every one of them on at once (stepper.DIAG_TABLES): profile statistics,
theta histograms, layer storage with histograms, the theta covariance, period totals with histograms, the root uptake with
histograms and the water-table histograms.  A run dumped on a row that is no profile row, inside the first period,
continues to the bit of the unbroken run, every table and every outside and overflow count included; the checkpoint holds
exactly the datasets written out below -- the key set, dtypes and shapes of the commit before the registry -- and a run
with none of them on holds none of their keys.  Reset, set, get and export go one path for every entry."""
import numpy as np
import pytest
import torch  # (before the library: the export test's buffers are torch's, one HIP runtime serves both)

from helpers import digest, golden
from test_gpu_enkf import _spread

pytestmark = pytest.mark.gpu
N, ROWS, CUT = 64, 96, 30                                        # the dump after row 30: between profile rows 24 and 36, in period 1
SETTINGS = dict(profile_stride=12, wtd_hist_stride=12, theta_hist_bins=32, storage_layers_cm=[(0.0, 100.0), (100.0, 300.0)],
                storage_bins=32, theta_cov_stride=50, period_ends=[48, 96], period_thresholds_cm=[150.0], period_bins=32,
                period_flux_max_cm=(16.0, 4.0), uptake_layers_cm=[(0.0, 100.0), (100.0, 300.0)], uptake_bins=32)
D, T, PROWS = 101, 17520, 1460                                   # well 1: 101 nodes, a year of rows, every 12th a profile row

BASE_KEYS = ("psi", "noise_scale", "moments", "next_row", "seed", "member_offset", "n_members", "dim_d", "dim_t",
             "initial_cond")
# the settings' keys and the tables' datasets a dump of the commit before the registry held (EnsembleSimulation.dump, one
# hand-written stanza per family), the datasets with the dtype and shape it gave them
SETTING_KEYS = ("profile_stride", "theta_hist_bins", "storage_layers_cm", "storage_bins", "theta_cov_stride", "period_ends",
                "period_thresholds_cm", "period_bins", "period_flux_max_cm", "uptake_layers_cm", "uptake_bins",
                "wtd_hist_stride")
DATASETS = {"profile_table": (np.int64, (PROWS * (D * 10 + 1) + T * 12 + 1,)),
            "theta_hist": (np.int32, (1, PROWS, D, 32)), "theta_hist_outside": (np.uint64, ()),
            "storage_table": (np.int64, (PROWS * (2 * 5 + 1) + 1,)),
            "storage_hist": (np.int32, (1, PROWS, 2, 32)), "storage_hist_outside": (np.uint64, ()),
            "theta_cov_table": (np.int64, (1, PROWS, 15)), "theta_cov_outside": (np.uint64, ()),
            "period_table": (np.int64, (2 * (5 * 5 + 1) + 1,)), "period_acc": (np.int64, (5, N)),
            "period_hist": (np.int32, (2 * 2 * (32 + D),)), "period_hist_outside": (np.uint64, ()),
            "uptake_table": (np.int64, (2 * (3 * 5 + 1 + (D - 1) * 2) + 1,)), "uptake_acc": (np.int64, (3, N)),
            "uptake_hist": (np.int32, (2 * 2 * 32,)), "uptake_hist_outside": (np.uint64, ()),
            "wtd_hist": (np.int32, (1, PROWS, D))}
COUNTERS = ("profile_overflow", "theta_hist_outside", "layer_storage_outside", "layer_storage_overflow", "theta_cov_outside",
            "period_totals_outside", "period_totals_overflow", "root_uptake_outside", "root_uptake_overflow")


def _checkpoint(path):
    from hydromodel_amd import hdf5io
    return dict(np.load(path)) if path.suffix == ".npz" else hdf5io.read(path)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _state(sim):
    from hydromodel_amd.stepper import DIAG_TABLES
    out = {"psi": sim.stepper.get_state(), "moments": sim.moments(), "noise_scale": sim.stepper.noise_scale()}
    out.update((key, sim.stepper.diag_raw(key)) for key in DIAG_TABLES)
    out.update((name, np.array(getattr(sim.stepper, name)(), dtype=np.uint64)) for name in COUNTERS)
    return out


@pytest.fixture(scope="module")
def run():
    """(cols, forcing, psi0, the unbroken run's state after ROWS, the checkpoint written after CUT and what it held)."""
    from hydromodel_amd.ensemble import EnsembleSimulation
    import tempfile
    from pathlib import Path
    _, cols, forcing = digest(1)
    assert (cols.dim_d, forcing.dim_t) == (D, T)
    psi0 = _spread(golden("g1_tables_1.npz")["initial_cond"], N)
    whole = EnsembleSimulation(cols, forcing, N, seed=6, psi0=psi0, **SETTINGS)
    try:
        assert whole.diag_tables_on() == ["profile", "theta_hist", "storage", "storage_hist", "theta_cov", "period",
                                          "period_acc", "period_hist", "uptake", "uptake_acc", "uptake_hist", "wtd_hist"]
        whole.advance(ROWS)
        want = _state(whole)
    finally:
        whole.close()
    with tempfile.TemporaryDirectory() as tmp:
        first = EnsembleSimulation(cols, forcing, N, seed=6, psi0=psi0, **SETTINGS)
        try:
            first.advance(CUT)
            held = _state(first)
            path = first.dump(Path(tmp) / "ck.h5")
        finally:
            first.close()
        yield cols, forcing, want, held, path


def test_the_checkpoint_holds_the_key_set_dtypes_and_shapes_of_before(run):
    *_, held, path = run
    data = _checkpoint(path)
    assert set(data) == set(BASE_KEYS + SETTING_KEYS) | set(DATASETS)
    for name, (dtype, shape) in DATASETS.items():
        a = np.asarray(data[name])
        assert a.dtype == dtype and a.shape == shape, name
    # the accumulators are live at the cut, and what was written is what the handle held
    assert data["period_acc"].any() and data["uptake_acc"].any()
    assert _same(data["period_acc"].reshape(-1), held["period_acc"]) and _same(data["profile_table"], held["profile"])
    assert _same(data["period_hist"], held["period_hist"][:-2]) and _same(data["wtd_hist"].reshape(-1), held["wtd_hist"])
    assert _same(data["theta_cov_table"].reshape(-1), held["theta_cov"][:-1])
    assert int(data["theta_hist_outside"]) == int(held["theta_hist_outside"])


def test_the_restored_run_continues_to_the_bit_of_the_unbroken_run(run):
    from hydromodel_amd.ensemble import EnsembleSimulation
    cols, forcing, want, held, path = run
    back = EnsembleSimulation.restore(path, cols, forcing)
    try:
        assert back.next_row == CUT + 1
        again = _state(back)
        for key in held:                                         # installed as they were held ...
            assert _same(held[key], again[key]), key
        back.advance(ROWS - CUT)
        got = _state(back)
    finally:
        back.close()
    for key in want:                                             # ... and continued to the unbroken run's
        assert _same(want[key], got[key]), key
    for key in ("profile", "theta_hist", "storage", "storage_hist", "theta_cov", "period", "period_hist", "uptake",
                "uptake_hist", "wtd_hist"):                      # every table took part
        assert want[key].any(), key
    assert not _same(want["period"], held["period"]) and not _same(want["uptake"], held["uptake"])


def test_a_run_with_none_of_them_on_writes_none_of_their_keys(tmp_path):
    from hydromodel_amd.ensemble import EnsembleSimulation
    _, cols, forcing = digest(1)
    sim = EnsembleSimulation(cols, forcing, N, seed=6, psi0=_spread(golden("g1_tables_1.npz")["initial_cond"], N))
    try:
        assert sim.diag_tables_on() == []
        sim.advance(12)
        path = sim.dump(tmp_path / "ck.h5")
    finally:
        sim.close()
    assert set(_checkpoint(path)) == set(BASE_KEYS)


def test_reset_set_get_and_export_go_one_path_for_every_entry(run):
    from hydromodel_amd.ensemble import EnsembleSimulation
    from hydromodel_amd.stepper import DIAG_TABLES
    from hydromodel_amd import _lib
    cols, forcing, *_, path = run
    sim = EnsembleSimulation.restore(path, cols, forcing)
    try:
        st = sim.stepper
        sim.advance(60 - CUT)                                    # past the first end row: no table is empty, the accumulators live
        held = {key: st.diag_raw(key) for key in DIAG_TABLES}
        assert all(t.any() for t in held.values())
        for key, e in DIAG_TABLES.items():
            assert st.diag_words(key) == held[key].size, key
            if "hc_export_" + e.stem in _lib.EXPORTS:
                out = torch.full((held[key].size,), -1, dtype=torch.int64 if e.dtype == np.int64 else torch.int32,
                                 device=f"cuda:{st.device}")
                st.export_diag(key, out.data_ptr())
                assert _same(out.cpu().numpy(), held[key]), key
            else:
                with pytest.raises(ValueError, match="no device-to-device export"):
                    st.export_diag(key, 0)
        for key in DIAG_TABLES:
            st.reset_diag(key)
            assert not _same(st.diag_raw(key), held[key]), key   # (the family's reset: its other tables go with it)
            for other in DIAG_TABLES:
                st.set_diag_raw(other, held[other])
            for other in DIAG_TABLES:
                assert _same(st.diag_raw(other), held[other]), (key, other)
        parts = st.diag_parts("uptake_hist")
        with pytest.raises(ValueError, match="counts must lie in"):      # the share histograms refuse what their siblings do
            st.set_root_uptake_hist(-parts["hist"].astype(np.int64) - 1)
        with pytest.raises(ValueError, match="outside count"):
            st.set_root_uptake_hist(parts["hist"], 1 << 64)
        assert _same(st.diag_raw("uptake_hist"), held["uptake_hist"])
    finally:
        sim.close()
