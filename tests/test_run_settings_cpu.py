"""The run's options without a GPU: a recording stand-in takes the place of ``EnsembleStepper``, so that what a constructor
asks of the handle, what a checkpoint holds of the settings and what is refused can be compared with the literals below.
The call sequences and the dataset names and dtypes were recorded from the commit before the options had one definition
(its two constructors, ``_start_tables`` and the stanzas of ``dump``): they are this project's own earlier output."""
import hashlib
import inspect
import itertools

import numpy as np
import pytest

from helpers import WELLS, digest
from test_gpu_assim_tables import OPTION_KEYS, OWNER_KEYS, _settings
from test_gpu_diag_tables import SETTING_KEYS, SETTINGS

N = 8
SMOOTHER = {"stride": 12, "lag_rows": 24}
CORRELATION = {"length_cm": 50.0, "layers": True}
PERTURBATION = {"precipitation_sigma": 0.3, "demand_sigma": 0.1, "correlation_days": 3.0}


def canon(x):
    """One line per value: arrays by dtype, shape and the SHA-1 of their bytes, containers by their items, the rest by
    type and repr."""
    if isinstance(x, np.ndarray):
        return f"<{x.dtype} {list(x.shape)} {hashlib.sha1(np.ascontiguousarray(x).tobytes()).hexdigest()[:12]}>"
    if isinstance(x, (list, tuple)):
        return ("[%s]" if isinstance(x, list) else "(%s)") % ", ".join(canon(v) for v in x)
    if isinstance(x, dict):
        return "{%s}" % ", ".join(f"{k}: {canon(v)}" for k, v in sorted(x.items()))
    if x is None or isinstance(x, (bool, int, float, str, np.generic)):
        return f"{type(x).__name__} {x!r}"
    return f"<{type(x).__name__}>"


class Recorder:
    """The stand-in for ``EnsembleStepper``: every call is logged as ``name(arguments)``, and the few properties the
    constructors and ``dump`` query answer from what was set."""
    calls, made = [], 0

    def __init__(self, cols, forcing, n, device=0, flags=None):
        type(self).made += 1
        several = isinstance(cols, (list, tuple))
        self.P, self.N, self.device = len(cols) if several else 1, int(n), device
        self.D = (cols[0] if several else cols).dim_d
        self.filter_sm_nodes = self.enkf_sm_nodes = self.filter_shard = None
        self._log("EnsembleStepper", (self.P, n), dict(device=device, flags=flags))

    def _log(self, name, args, kw):
        items = [canon(a) for a in args] + [f"{k}={canon(v)}" for k, v in sorted(kw.items())]
        type(self).calls.append(f"{name}({', '.join(items)})")

    def set_filter_soil_moisture(self, nodes, values=None, sigma=None):
        self._log("set_filter_soil_moisture", (nodes, values, sigma), {})
        self.filter_sm_nodes = np.asarray(nodes)

    def set_enkf_soil_moisture(self, nodes, values=None, sigma=None):
        self._log("set_enkf_soil_moisture", (nodes, values, sigma), {})
        self.enkf_sm_nodes = np.asarray(nodes)

    filter_sm_n = property(lambda self: 0 if self.filter_sm_nodes is None else int(self.filter_sm_nodes.size))
    enkf_sm_n = property(lambda self: 0 if self.enkf_sm_nodes is None else int(self.enkf_sm_nodes.size))

    def forcing_state(self):
        self._log("forcing_state", (), {})
        return np.zeros((2, self.N)), 0

    def filter_smoother_ring(self):
        self._log("filter_smoother_ring", (), {})
        return np.zeros((3, self.N), np.int32), np.zeros((3, self.N), np.int64), np.zeros(3, np.int64), 0

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*args, **kw):
            self._log(name, args, kw)
            if name.endswith("_capture"):
                return np.zeros((2, self.N)), np.zeros(2, np.int64)
            return np.zeros((self.N, self.D)) if name.endswith("_base") or name == "get_state" else np.zeros(self.N)
        return call


@pytest.fixture
def recorder(monkeypatch):
    from hydromodel_amd import ensemble
    Recorder.calls, Recorder.made = [], 0
    monkeypatch.setattr(ensemble, "EnsembleStepper", Recorder)
    return Recorder


@pytest.fixture(scope="module")
def site():
    """(cols, a second parameter point on the same grid, forcing, psi0)."""
    from hydromodel_amd.digest import ColumnTables
    from hydromodel_amd.ensemble import merge_parameters
    params, cols, forcing = digest(1)
    other = ColumnTables(merge_parameters(params, {"Soil_Properties": {"a0": 0.003, "psi_sat": -0.001}}), WELLS[1])
    return cols, other, forcing, np.linspace(-300.0, 100.0, cols.dim_d)


def configurations(cols, forcing):
    """The six configurations of the call-sequence and round-trip tests: name -> (keywords, the records restore needs)."""
    filt, frec = _settings("filter", cols, forcing)
    enkf, erec = _settings("enkf", cols, forcing)
    plain = {k: v for k, v in filt.items() if k != "filter_rejuvenation"}
    return {"none": ({}, {}),
            "diagnostics": (dict(SETTINGS), {}),
            "filter": (dict(filt, filter_smoother=SMOOTHER), frec),
            "enkf": (enkf, erec),
            "noise": (dict(noise_correlation=CORRELATION, forcing_perturbation=PERTURBATION), {}),
            "crossed": (dict(plain, noise_correlation=CORRELATION, **SETTINGS), frec)}


CONFIGURATIONS = ("none", "diagnostics", "filter", "enkf", "noise", "crossed")


def start(kind, site, kw):
    """An ensemble or a two-point sweep with ``psi0`` given, on whatever stands in for the stepper."""
    from hydromodel_amd.ensemble import EnsembleSimulation, SweepSimulation
    cols, other, forcing, psi0 = site
    if kind == "ensemble":
        return EnsembleSimulation(cols, forcing, N, seed=6, psi0=psi0, **kw)
    return SweepSimulation([cols, other], forcing, N, seed=6, psi0=np.stack([psi0, psi0 + 1.0]), **kw)


# ---- 1. the calls a constructor makes on the handle, recorded from the commit before (arrays: dtype, shape, SHA-1) --------
_HANDLE = {"ensemble": ["EnsembleStepper(int 1, int 8, device=int 0, flags=NoneType None)",
                        "set_state(<float64 [101] 5d623f1d95cb>)", "set_noise_philox(int 6, int 0)"],
           "sweep": ["EnsembleStepper(int 2, int 16, device=int 0, flags=NoneType None)", "set_generic_exponents(bool True)",
                     "set_state(<float64 [2, 101] 24c01ca1bed8>)", "set_noise_philox(int 6, int 0)",
                     "set_point_member_bases(<int64 [2] e88d9e1ac6ad>)"]}
_CORRELATION = {"ensemble": "set_noise_correlation(<float64 [1, 101] 51cedc39d587>, <float64 [1, 101] a0cdb5bb47ba>)",
                "sweep": "set_noise_correlation(<float64 [2, 101] 0fd29f239c95>, <float64 [2, 101] dd7461e73193>)"}
_PROFILES = ["set_profile_stats(int 12)", "set_theta_hist(int 32)", "set_layer_storage(<int32 [2, 2] 1d675c6105ec>, int 32)",
             "set_theta_cov(int 50)", "profile_snapshot(int 0)", "set_wtd_hist(int 12)"]
_PERIODS = ["set_period_totals(<int64 [2] 47da5093694e>, <int32 [1] 0a03f4bcfdf1>, int 32, [int 4, int 2])",
            "set_root_uptake(<int32 [2, 2] 1d675c6105ec>, int 32)"]
_FILTER = ["set_filter(int 24, float 10.0, int 11)",
           "set_filter_soil_moisture(<int32 [2] 0b9f04c54f76>, <float64 [17520, 2] 96057fcf85cc>, <float64 [2] 783dcb0b7cbf>)",
           "set_filter_tempering(float 0.5)", "set_filter_rejuvenation(float 0.98)", "set_filter_window((int 6, int 12))",
           "set_filter_smoother(int 12, int 2)"]
_ENKF = ["set_enkf(int 24, float 10.0, float 0.0, int 11)",
         "set_enkf_soil_moisture(<int32 [2] 0b9f04c54f76>, <float64 [17520, 2] 96057fcf85cc>, <float64 [2] 783dcb0b7cbf>)",
         "set_enkf_method(str 'sqrt', float 0.5)", "set_enkf_window((int 6, int 12))",
         "set_enkf_noise_field(bool True, float 0.5)"]
_FORCING = ("set_forcing_perturbation(float 0.3, float 0.1, c=float 0.6975549304301475, member_offset=NoneType None, "
            "phi=float 0.7165313105737893, seed=int 6)")


def recorded(kind, name):
    """The parent's sequence for one configuration: the handle's own start, then the options' calls."""
    tail = {"none": [], "diagnostics": _PROFILES + _PERIODS, "filter": _FILTER, "enkf": _ENKF,
            "noise": [_CORRELATION[kind], _FORCING],
            "crossed": [_CORRELATION[kind]] + _PROFILES + _FILTER[:3] + [_FILTER[4]] + _PERIODS}[name]
    return _HANDLE[kind] + tail


@pytest.mark.parametrize("name", CONFIGURATIONS)
@pytest.mark.parametrize("kind", ["ensemble", "sweep"])
def test_a_constructor_makes_the_calls_the_parent_made(kind, name, site, recorder):
    kw, _ = configurations(site[0], site[2])[name]
    start(kind, site, kw)
    assert recorder.calls == recorded(kind, name)


# ---- 2. settings -> the settings' datasets -> constructor keywords -> settings, without a handle -------------------------
NOISE_KEYS = ("noise_correlation_length_cm", "noise_correlation_layers", "noise_correlation_a", "noise_correlation_b")
FORCING_KEYS = ("forcing_precipitation_sigma", "forcing_demand_sigma", "forcing_correlation_days", "forcing_seed")
# the dtype the parent's dump gave each dataset that holds a setting (the other keys of the lists are tables and live state)
SETTING_DTYPES = dict(
    profile_stride="int64", theta_hist_bins="int64", storage_layers_cm="float64", storage_bins="int64",
    theta_cov_stride="int64", period_ends="int64", period_thresholds_cm="float64", period_bins="int64",
    period_flux_max_cm="float64", uptake_layers_cm="float64", uptake_bins="int64", wtd_hist_stride="int64",
    filter_stride="int64", filter_sigma_cm="float64", filter_seed="uint64", filter_sm_nodes="int32",
    filter_ess_floor="float64", filter_rejuvenation="float64", filter_window_offsets="int64", filter_smoother="int64",
    enkf_stride="int64", enkf_sigma_cm="float64", enkf_localisation_cm="float64", enkf_seed="uint64", enkf_method="int64",
    enkf_relaxation="float64", enkf_sm_nodes="int32", enkf_window_offsets="int64", enkf_noise_relaxation="float64",
    noise_correlation_length_cm="float64", noise_correlation_layers="int64", noise_correlation_a="float64",
    noise_correlation_b="float64", forcing_precipitation_sigma="float64", forcing_demand_sigma="float64",
    forcing_correlation_days="float64", forcing_seed="uint64")
_FILTER_KEYS = OWNER_KEYS["filter"] + OPTION_KEYS["filter"]
KEYS_OF = {"none": (), "diagnostics": SETTING_KEYS, "filter": _FILTER_KEYS + ("filter_smoother",),
           "enkf": OWNER_KEYS["enkf"] + OPTION_KEYS["enkf"], "noise": NOISE_KEYS + FORCING_KEYS,
           "crossed": SETTING_KEYS + tuple(k for k in _FILTER_KEYS if "rejuvenation" not in k) + NOISE_KEYS}


def _normalised(site, kw):
    from hydromodel_amd import settings
    return settings.normalise("EnsembleSimulation", kw, [site[0]], 6)


@pytest.mark.parametrize("name", CONFIGURATIONS)
def test_settings_round_trip_through_their_datasets_without_a_handle(name, site):
    from hydromodel_amd import settings
    kw, records = configurations(site[0], site[2])[name]
    first = _normalised(site, kw)
    data = settings.checkpoint_datasets(first)
    assert {k: str(np.asarray(v).dtype) for k, v in data.items()} == \
        {k: SETTING_DTYPES[k] for k in KEYS_OF[name] if k in SETTING_DTYPES}                 # an option off: none of its keys
    flat = {k: np.asarray(v).reshape(-1) if np.ndim(v) else v for k, v in data.items()}      # (tables as a container gives them)
    again = _normalised(site, settings.checkpoint_keywords(flat, "ck.h5", **records))
    assert canon(vars(again)) == canon(vars(first))
    assert settings.checkpoint_datasets(again).keys() == data.keys()


# ---- 3. the refusals, one case per row of the table, with the parent's messages --------------------------------------------
_F, _E = dict(filter_stride=24, filter_sigma_cm=5.0), dict(enkf_stride=24, enkf_sigma_cm=5.0)
_FS, _ES = dict(_F, filter_shard=([0, 8], 0, None)), dict(_E, enkf_shard=(8, None))
_REC = {"nodes": np.array([6, 45], np.int32), "values": None, "sigma": 0.05}
_NEEDS_PROFILE, _NEEDS_FILTER, _NEEDS_ENKF = (" needs the profile statistics (profile_stride > 0)",
                                              " needs the particle filter (filter_stride > 0)", " needs the EnKF (enkf_stride > 0)")
REFUSED = (
    (dict(noise_correlation=CORRELATION, noise="numpy"),
     " EnsembleSimulation: noise_correlation serves the Philox noise source; a noise='numpy' caller shapes its own vectors "
     "(stepper.noise_correlate)."),
    (dict(_F, noise_correlation=CORRELATION, filter_rejuvenation=0.98),
     " EnsembleSimulation: noise_correlation and filter_rejuvenation exclude each other: the jitter is white per node and "
     "would erode the correlation by a share h^2 per move."),
    (dict(_FS, forcing_perturbation=PERTURBATION),
     "filter_shard and forcing_perturbation exclude each other: the routed columns do not carry the members' forcing state"),
    (dict(_ES, enkf_noise_field=True),
     "enkf_shard and enkf_noise_field exclude each other: the exchanged partials cover psi only"),
    (dict(_FS, filter_rejuvenation=0.98),
     "filter_shard and filter_rejuvenation exclude each other: the sharded filter gathers water-table indices only, the "
     "moments of the base vectors would need an exchange of their own"),
    (dict(_FS, filter_window_offsets=(6,)),
     "filter_shard and filter_window_offsets exclude each other: the sharded filter gathers the water-table indices of the "
     "assimilation row only"),
    (dict(_FS, period_ends=[48]),
     "period_ends and filter_shard exclude each other: the sharded filter routes the members' columns, which do not carry "
     "the period accumulators"),
    (dict(_FS, filter_smoother=SMOOTHER),
     "filter_shard and filter_smoother exclude each other: the routed columns do not carry the smoother's ring"),
    (dict(filter_shard=([0, 8], 0, None)), "filter_shard" + _NEEDS_FILTER),
    (dict(_FS, filter_soil_moisture=_REC),
     "filter_shard and filter_soil_moisture exclude each other: the sharded filter gathers water-table indices only"),
    (dict(theta_cov_stride=50), "theta_cov_stride" + _NEEDS_PROFILE),
    (dict(profile_stride=12, storage_bins=32), "storage_bins needs storage_layers_cm"),
    (dict(storage_layers_cm=[(0.0, 100.0)]), "storage_layers_cm" + _NEEDS_PROFILE),
    (dict(theta_hist_bins=32), "theta_hist_bins" + _NEEDS_PROFILE),
    (dict(filter_soil_moisture=_REC), "filter_soil_moisture" + _NEEDS_FILTER),
    (dict(filter_ess_floor=0.5), "filter_ess_floor" + _NEEDS_FILTER),
    (dict(filter_rejuvenation=0.98), "filter_rejuvenation" + _NEEDS_FILTER),
    (dict(filter_smoother=SMOOTHER), "filter_smoother" + _NEEDS_FILTER),
    (dict(enkf_soil_moisture=_REC), "enkf_soil_moisture" + _NEEDS_ENKF),
    (dict(enkf_method="sqrt"), "enkf_method / enkf_relaxation need the EnKF (enkf_stride > 0)"),
    (dict(enkf_relaxation=0.5), "enkf_method / enkf_relaxation need the EnKF (enkf_stride > 0)"),
    (dict(enkf_noise_field=True), "enkf_noise_field" + _NEEDS_ENKF),
    (dict(period_thresholds_cm=[150.0]), "period_thresholds_cm / period_bins need period_ends"),
    (dict(period_bins=32), "period_thresholds_cm / period_bins need period_ends"),
    (dict(uptake_bins=32), "uptake_bins needs uptake_layers_cm"),
    (dict(uptake_layers_cm=[(0.0, 100.0)]), "uptake_layers_cm needs period_ends: the uptake is totalled over the periods"),
    (dict(enkf_shard=(8, None)), "enkf_shard" + _NEEDS_ENKF),
)


def test_every_row_of_the_refusals_has_a_case():
    from hydromodel_amd import settings
    assert len(REFUSED) == len(settings.REFUSALS)


@pytest.mark.parametrize("case", range(len(REFUSED)))
def test_a_refusal_fires_with_the_parents_message_before_any_handle_exists(case, site, recorder):
    from hydromodel_amd.ensemble import EnsembleSimulation
    kw, message = REFUSED[case]
    with pytest.raises(ValueError) as err:
        EnsembleSimulation(site[0], site[2], N, seed=6, **kw)             # (no psi0: a handle would mean a spin-up too)
    assert str(err.value) == message and recorder.made == 0


# ---- 4. the keywords and their defaults, from the parent's two signatures --------------------------------------------------
SHARED = dict(
    seed=0, device=0, flags=None, psi0=None, profile_stride=0, wtd_hist_stride=0, filter_stride=0, filter_sigma_cm=None,
    filter_seed=None, enkf_stride=0, enkf_sigma_cm=None, enkf_localisation_cm=0.0, enkf_seed=None, enkf_soil_moisture=None,
    enkf_method="stochastic", enkf_relaxation=0.0, enkf_window_offsets=(), filter_soil_moisture=None, theta_hist_bins=0,
    storage_layers_cm=None, storage_bins=0, period_ends=None, period_thresholds_cm=(), period_bins=0,
    period_flux_max_cm=(16.0, 4.0), filter_ess_floor=0.0, filter_window_offsets=(), enkf_noise_field=None,
    filter_rejuvenation=0.0, noise_correlation=None, theta_cov_stride=0, uptake_layers_cm=None, uptake_bins=0,
    filter_smoother=None, forcing_perturbation=None)
ENSEMBLE_KEYWORDS = dict(SHARED, member_offset=0, noise="philox", spinup="shared", enkf_shard=None, filter_shard=None)
SWEEP_KEYWORDS = dict(SHARED, first_point=0, point_ids=None)


def test_the_constructors_take_the_parents_keywords_with_the_parents_defaults(site, recorder):
    from hydromodel_amd import settings
    from hydromodel_amd.ensemble import EnsembleSimulation, SweepSimulation
    assert len(ENSEMBLE_KEYWORDS) == 43 - 3 and len(SWEEP_KEYWORDS) == 35 + 2       # (43 with cols, forcing and n_members)

    def accepted(cls):                                    # the constructor's own parameters and the options both share
        own = [p for p in inspect.signature(cls.__init__).parameters.values() if p.default is not p.empty]
        assert not set(p.name for p in own) & set(settings.OPTIONS)
        return dict(((p.name, p.default) for p in own), **settings.OPTIONS)

    assert accepted(EnsembleSimulation) == ENSEMBLE_KEYWORDS and accepted(SweepSimulation) == SWEEP_KEYWORDS
    for cls, first in ((EnsembleSimulation, site[0]), (SweepSimulation, [site[0], site[1]])):
        positional = [p.name for p in inspect.signature(cls.__init__).parameters.values() if p.default is p.empty
                      and p.kind is p.POSITIONAL_OR_KEYWORD]
        assert positional[1:] == ["cols" if cls is EnsembleSimulation else "cols_list", "forcing", "n_members"]
        with pytest.raises(TypeError, match="unexpected keyword argument 'filter_strid'"):
            cls(first, site[2], N, filter_strid=24)
    for own in ("noise", "spinup", "member_offset", "enkf_shard", "filter_shard"):
        with pytest.raises(TypeError, match=f"unexpected keyword argument '{own}'"):
            SweepSimulation([site[0], site[1]], site[2], N, **{own: ENSEMBLE_KEYWORDS[own]})
    assert recorder.made == 0


# ---- 5. the dataset that carries the base vectors: what dump writes is what restore installs --------------------------------
CARRIERS = ("filter_base", "enkf_noise_base", "noise_field_base")           # ... or, with none of them, noise_scale


@pytest.mark.parametrize("filt, field, corr, pert", [c for c in itertools.product((False, True), repeat=4)
                                                     if not (c[0] and c[1])])
def test_the_base_vectors_come_back_from_the_dataset_they_went_into(filt, field, corr, pert, site, recorder, tmp_path):
    """The sixteen combinations less the four with both the filter and the EnKF's noise field: the handle refuses a
    filter beside an EnKF (stepper.set_enkf), which the stand-in does not."""
    from hydromodel_amd.ensemble import EnsembleSimulation
    kw = dict(_F if filt else {}, **(dict(_E, enkf_noise_field=True) if field else {}))
    kw.update(dict(noise_correlation=CORRELATION) if corr else {}, **(dict(forcing_perturbation=PERTURBATION) if pert else {}))
    want = "filter_base" if filt else "enkf_noise_base" if field else "noise_field_base" if corr else "noise_scale"
    sim = start("ensemble", site, kw)
    sim.stepper.moments = lambda: np.zeros((3, site[2].dim_t), np.int64)
    recorder.calls = []
    path = sim.dump(tmp_path / "ck.npz")
    read = [c[:-2] for c in recorder.calls if c[:-2] in CARRIERS]
    assert read == [k for k in CARRIERS if k == want]
    assert set(np.load(path).files) & set(CARRIERS) == {want} - {"noise_scale"}
    recorder.calls = []
    EnsembleSimulation.restore(path, site[0], site[2])
    installed = [c.split("(")[0] for c in recorder.calls if c.split("(")[0] in ["set_" + k for k in CARRIERS + ("noise_scale",)]]
    assert installed == ["set_" + want]
