"""The options of a run, each defined once: keyword and default (:data:`OPTIONS`, :data:`MORE_OPTIONS`), the normalised values and every refusal
before a handle exists (:func:`normalise`, :data:`REFUSALS`), the ordered walk that starts the handle (:data:`START`), which
tables are on (:data:`TABLE_OPTION`) and the two halves of the checkpoint (:data:`SETTING_DATASETS`, :data:`RUN_STATE`,
:data:`MEMBER_STATE`).  A new run option is one entry in each of these, plus its ``hc_set_*`` accessor on the stepper.
The options' prose is the docstring of ``ensemble._Run``."""
from types import SimpleNamespace

import numpy as np

from .stepper import (ENKF_METHODS, conductivity_ranges, conductivity_settings, enkf_window_settings,
                      filter_smoother_config, filter_window_settings, flux_max_log2_of, forcing_coefficients,
                      forcing_perturbation_settings, layer_cells, layer_ranges, noise_correlation_breaks,
                      noise_correlation_settings, noise_correlation_tables, noise_field_settings, rejuvenation_discount,
                      sensor_nodes)

# ---- 1. keywords and defaults: what EnsembleSimulation and SweepSimulation both take after their own parameters ----------
OPTIONS = dict(
    profile_stride=0, wtd_hist_stride=0, filter_stride=0, filter_sigma_cm=None, filter_seed=None, enkf_stride=0,
    enkf_sigma_cm=None, enkf_localisation_cm=0.0, enkf_seed=None, enkf_soil_moisture=None, enkf_method="stochastic",
    enkf_relaxation=0.0, enkf_window_offsets=(), filter_soil_moisture=None, theta_hist_bins=0, storage_layers_cm=None,
    storage_bins=0, period_ends=None, period_thresholds_cm=(), period_bins=0, period_flux_max_cm=(16.0, 4.0),
    filter_ess_floor=0.0, filter_window_offsets=(), enkf_noise_field=None, filter_rejuvenation=0.0, noise_correlation=None,
    theta_cov_stride=0, uptake_layers_cm=None, uptake_bins=0, filter_smoother=None, forcing_perturbation=None)
# ... and the options that joined after those: taken by both constructors in the same way, through their ``**options``
MORE_OPTIONS = dict(conductivity=None)


# ---- 2. the refusals: (option, "needs" or "excludes", the other option, message); ``{who}`` is the class ------------------
_ENKF = "enkf_stride"
_OWNER = {"profile_stride": "the profile statistics (profile_stride > 0)",
          "filter_stride": "the particle filter (filter_stride > 0)", _ENKF: "the EnKF (enkf_stride > 0)"}
REFUSALS = (
    ("noise_correlation", "excludes", "noise_numpy",
     " {who}: noise_correlation serves the Philox noise source; a noise='numpy' caller shapes its own vectors "
     "(stepper.noise_correlate)."),
    ("noise_correlation", "excludes", "filter_rejuvenation",
     " {who}: noise_correlation and filter_rejuvenation exclude each other: the jitter is white per node and would erode "
     "the correlation by a share h^2 per move."),
    ("filter_shard", "excludes", "forcing_perturbation",
     "filter_shard and forcing_perturbation exclude each other: the routed columns do not carry the members' forcing state"),
    ("enkf_shard", "excludes", "enkf_noise_field",
     "enkf_shard and enkf_noise_field exclude each other: the exchanged partials cover psi only"),
    ("filter_shard", "excludes", "filter_rejuvenation",
     "filter_shard and filter_rejuvenation exclude each other: the sharded filter gathers water-table indices only, the "
     "moments of the base vectors would need an exchange of their own"),
    ("filter_shard", "excludes", "filter_window_offsets",
     "filter_shard and filter_window_offsets exclude each other: the sharded filter gathers the water-table indices of the "
     "assimilation row only"),
    ("filter_shard", "excludes", "period_ends",
     "period_ends and filter_shard exclude each other: the sharded filter routes the members' columns, which do not carry "
     "the period accumulators"),
    ("filter_shard", "excludes", "filter_smoother",
     "filter_shard and filter_smoother exclude each other: the routed columns do not carry the smoother's ring"),
    ("filter_shard", "excludes", "filter_soil_moisture",
     "filter_shard and filter_soil_moisture exclude each other: the sharded filter gathers water-table indices only"),
    ("storage_bins", "needs", "storage_layers_cm", "storage_bins needs storage_layers_cm"),
    ("enkf_method", "needs", _ENKF, "enkf_method / enkf_relaxation need the EnKF (enkf_stride > 0)"),
    ("enkf_relaxation", "needs", _ENKF, "enkf_method / enkf_relaxation need the EnKF (enkf_stride > 0)"),
    ("period_thresholds_cm", "needs", "period_ends", "period_thresholds_cm / period_bins need period_ends"),
    ("period_bins", "needs", "period_ends", "period_thresholds_cm / period_bins need period_ends"),
    ("uptake_bins", "needs", "uptake_layers_cm", "uptake_bins needs uptake_layers_cm"),
    ("uptake_layers_cm", "needs", "period_ends", "uptake_layers_cm needs period_ends: the uptake is totalled over the periods"),
) + tuple((option, "needs", owner, f"{option} needs {_OWNER[owner]}") for option, owner in (
    ("theta_cov_stride", "profile_stride"), ("storage_layers_cm", "profile_stride"), ("theta_hist_bins", "profile_stride"),
    ("filter_shard", "filter_stride"), ("filter_soil_moisture", "filter_stride"), ("filter_ess_floor", "filter_stride"),
    ("filter_rejuvenation", "filter_stride"), ("filter_smoother", "filter_stride"), ("enkf_soil_moisture", _ENKF),
    ("enkf_noise_field", _ENKF), ("enkf_shard", _ENKF)))


def _some(value):
    return value is not None and len(value) > 0


def normalise(who, options, points, seed, lead=(), noise="philox", member_offset=0, enkf_shard=None, filter_shard=None):
    """The run's options (the keywords a constructor was given beyond its own) as the attributes the run exposes, with
    every refusal raised: an unknown keyword (TypeError), a value its validator refuses, the rows of :data:`REFUSALS`.
    ``points``: the columns of the handle's parameter points (layer ranges, sensor nodes, one correlation table per
    point); ``seed``: the run's, the default of the features' own; ``lead``: the leading shape of per-point tables.
    Returns the namespace; ``on`` in it says for every option whether the run has it."""
    for key in options:
        if key not in OPTIONS and key not in MORE_OPTIONS:
            raise TypeError(f"{who}.__init__() got an unexpected keyword argument '{key}'")
    o = SimpleNamespace(**{**OPTIONS, **MORE_OPTIONS, **options})
    cols, s = points[0], SimpleNamespace()
    corr = noise_correlation_settings(o.noise_correlation)
    pert = forcing_perturbation_settings(o.forcing_perturbation)
    # the forcing state in the EnKF's analysis is a key of the perturbation's value: its two refusals are raised here, where
    # the value is read
    forcing_enkf = pert is not None and "enkf_relaxation" in pert
    if forcing_enkf and not int(o.enkf_stride or 0):
        raise ValueError("forcing_perturbation.enkf_relaxation needs the EnKF (enkf_stride > 0)")
    if forcing_enkf and enkf_shard is not None:
        raise ValueError("enkf_shard and the forcing analysis exclude each other: the exchanged partials cover psi only")
    s.profile_stride, s.wtd_hist_stride = int(o.profile_stride), int(o.wtd_hist_stride)
    s.theta_cov_stride, s.theta_hist_bins = int(o.theta_cov_stride or 0), int(o.theta_hist_bins or 0)
    s.storage_layers_cm = np.asarray(o.storage_layers_cm, dtype=np.float64).reshape(-1, 2) if _some(o.storage_layers_cm) else None
    s.storage_bins = int(o.storage_bins or 0) if s.storage_layers_cm is not None else 0
    # the conductivity statistics' value is validated where it is read, and its one refusal is raised with it
    s.conductivity = conductivity_settings(o.conductivity)              # None: off; {"layers_cm": [L][2] or None}
    if s.conductivity is not None and not s.profile_stride:
        raise ValueError(f"conductivity needs {_OWNER['profile_stride']}")
    s.filter_stride = int(o.filter_stride or 0)
    s.filter_sigma_cm = float(o.filter_sigma_cm) if s.filter_stride else None
    s.filter_seed = (int(seed) if o.filter_seed is None else int(o.filter_seed)) if s.filter_stride else None
    s.filter_soil_moisture = o.filter_soil_moisture
    s.filter_ess_floor = float(o.filter_ess_floor or 0.0)
    s.filter_rejuvenation = rejuvenation_discount(o.filter_rejuvenation)
    s.filter_smoother = filter_smoother_config(o.filter_smoother)        # (stride, lag in record rows) or None
    s.enkf_stride = int(o.enkf_stride or 0)
    s.enkf_sigma_cm = float(o.enkf_sigma_cm) if s.enkf_stride else None
    s.enkf_localisation_cm = float(o.enkf_localisation_cm or 0.0) if s.enkf_stride else None
    s.enkf_seed = (int(seed) if o.enkf_seed is None else int(o.enkf_seed)) if s.enkf_stride else None
    s.enkf_soil_moisture = o.enkf_soil_moisture
    s.enkf_method, s.enkf_relaxation = str(o.enkf_method), float(o.enkf_relaxation)
    s.enkf_noise_relaxation = noise_field_settings(o.enkf_noise_field, s.enkf_relaxation)       # None: off
    s.period_ends = np.asarray(o.period_ends, dtype=np.int64).reshape(-1) if _some(o.period_ends) else None
    periods = s.period_ends is not None
    s.period_thresholds_cm = np.asarray(o.period_thresholds_cm if periods and o.period_thresholds_cm is not None else [],
                                        dtype=np.float64).reshape(-1)
    s.period_bins = int(o.period_bins or 0) if periods else 0
    s.period_flux_max_cm = tuple(float(v) for v in o.period_flux_max_cm) if s.period_bins else None
    s.uptake_layers_cm = np.asarray(o.uptake_layers_cm, dtype=np.float64).reshape(-1, 2) if _some(o.uptake_layers_cm) else None
    s.uptake_bins = int(o.uptake_bins or 0) if s.uptake_layers_cm is not None else 0
    sensors = [0 if rec is None else np.size(rec["nodes"]) for rec in (s.filter_soil_moisture, s.enkf_soil_moisture)]
    s.filter_window_offsets = filter_window_settings(o.filter_window_offsets, s.filter_stride, sensors[0])
    s.enkf_window_offsets = enkf_window_settings(o.enkf_window_offsets, s.enkf_stride, sensors[1])
    # which options the run has: a stride, floor or window that is not zero or empty, a table, record or dict that is given
    s.on = on = {k: v is not None if v is None or isinstance(v, (dict, np.ndarray)) else bool(v) for k, v in vars(s).items()}
    on.update(storage_bins=bool(o.storage_bins), period_bins=bool(o.period_bins), uptake_bins=bool(o.uptake_bins),
              period_thresholds_cm=_some(o.period_thresholds_cm), enkf_method=s.enkf_method != "stochastic",
              enkf_relaxation=s.enkf_relaxation != 0.0, enkf_scheme=(s.enkf_method, s.enkf_relaxation) != ("stochastic", 0.0),
              enkf_noise_field=s.enkf_noise_relaxation is not None, noise_correlation=corr is not None,
              forcing_perturbation=pert is not None, forcing_enkf=forcing_enkf, noise_numpy=noise == "numpy",
              enkf_shard=enkf_shard is not None, filter_shard=filter_shard is not None, always=True)
    for option, relation, other, message in REFUSALS:
        if on[option] and on[other] == (relation == "excludes"):
            raise ValueError(message.format(who=who))
    if s.period_bins and len(s.period_flux_max_cm) != 2:
        raise ValueError("period_flux_max_cm is (transpiration, lateral flow)")
    # what needs the columns
    s.storage_ranges = layer_ranges(cols.z, s.storage_layers_cm) if on["storage_layers_cm"] else None
    s.conductivity_ranges = conductivity_ranges(cols.z, cols.dz, s.conductivity["layers_cm"]) if on["conductivity"] else None
    s.period_threshold_nodes = sensor_nodes(cols.z, s.period_thresholds_cm) if periods else None
    s._period_flux_log2 = [flux_max_log2_of(v) for v in s.period_flux_max_cm] if s.period_bins else (0, 0)
    s.uptake_cells = layer_cells(cols.z, s.uptake_layers_cm) if on["uptake_layers_cm"] else None
    s.noise_correlation, s.noise_correlation_a, s.noise_correlation_b, s.noise_correlation_breaks_cm = None, None, None, ()
    if corr is not None:
        length, layers = corr
        breaks = [noise_correlation_breaks(c.layers, c.z) if layers else () for c in points]
        ab = [noise_correlation_tables(c.z, length, br) for c, br in zip(points, breaks)]
        a, b = np.stack([t[0] for t in ab]), np.stack([t[1] for t in ab])
        s.noise_correlation, s._noise_correlation_tables = {"length_cm": length, "layers": layers}, (a, b)
        s.noise_correlation_a = a.reshape(lead + a.shape[1:])            # [D]; a sweep: [P][D]
        s.noise_correlation_b = b.reshape(lead + b.shape[1:])
        s.noise_correlation_breaks_cm = tuple(breaks) if lead else breaks[0]
    s.forcing_perturbation = None
    if pert is not None:
        own = int(seed) if pert["seed"] is None else pert["seed"]
        phi, s._forcing_c = forcing_coefficients(pert["correlation_days"])
        s.forcing_perturbation = dict(pert, seed=int(own), phi=phi)
    # a shard of a host-noise ensemble has no stream key of its own: the forcing factors are told the first member's id
    s._forcing_offset = int(member_offset) if noise == "numpy" else None
    s.enkf_shard = (int(enkf_shard[0]), int(member_offset)) if enkf_shard is not None else None
    s.filter_shard, s._shard_exchange = None, (enkf_shard, filter_shard)
    return s


# ---- 3. starting the handle: (option, call) in the one order the handle is set up in ---------------------------------------
def _set_soil_moisture(setter):
    return lambda st, s: getattr(st, "set_" + setter)(*(getattr(s, setter)[k] for k in ("nodes", "values", "sigma")))


START = (
    # after the spin-up, before the filters: the correlated Philox vectors and the members' forcing factors
    ("noise_correlation", lambda st, s: st.set_noise_correlation(*s._noise_correlation_tables)),      # one table per point
    ("forcing_perturbation", lambda st, s: st.set_forcing_perturbation(
        s.forcing_perturbation["precipitation_sigma"], s.forcing_perturbation["demand_sigma"], seed=s.forcing_perturbation["seed"],
        phi=s.forcing_perturbation["phi"], c=s._forcing_c, member_offset=s._forcing_offset)),
    ("profile_stride", lambda st, s: st.set_profile_stats(s.profile_stride)),
    ("theta_hist_bins", lambda st, s: st.set_theta_hist(s.theta_hist_bins)),
    ("storage_layers_cm", lambda st, s: st.set_layer_storage(s.storage_ranges, s.storage_bins)),
    ("theta_cov_stride", lambda st, s: st.set_theta_cov(s.theta_cov_stride)),
    ("conductivity", lambda st, s: st.set_conductivity_stats(s.conductivity_ranges)),
    ("profile_stride", lambda st, s: st.profile_snapshot(0)),             # psi[0], theta_vol[0]: the state before any solve
    ("wtd_hist_stride", lambda st, s: st.set_wtd_hist(s.wtd_hist_stride)),
    ("filter_stride", lambda st, s: st.set_filter(s.filter_stride, s.filter_sigma_cm, s.filter_seed)),
    ("filter_soil_moisture", _set_soil_moisture("filter_soil_moisture")),
    ("filter_ess_floor", lambda st, s: st.set_filter_tempering(s.filter_ess_floor)),
    ("filter_rejuvenation", lambda st, s: st.set_filter_rejuvenation(s.filter_rejuvenation)),
    ("filter_window_offsets", lambda st, s: st.set_filter_window(s.filter_window_offsets)),
    ("filter_smoother", lambda st, s: st.set_filter_smoother(*s.filter_smoother)),      # after everything else of the filter's
    ("enkf_stride", lambda st, s: st.set_enkf(s.enkf_stride, s.enkf_sigma_cm, s.enkf_localisation_cm, s.enkf_seed)),
    ("enkf_soil_moisture", _set_soil_moisture("enkf_soil_moisture")),
    ("enkf_scheme", lambda st, s: st.set_enkf_method(s.enkf_method, s.enkf_relaxation)),
    ("enkf_window_offsets", lambda st, s: st.set_enkf_window(s.enkf_window_offsets)),
    # (after any spin-up: a Philox run then takes the caller-noise path)
    ("enkf_noise_field", lambda st, s: st.set_enkf_noise_field(True, s.enkf_noise_relaxation)),
    ("forcing_enkf", lambda st, s: st.set_enkf_forcing(True, s.forcing_perturbation["enkf_relaxation"])),
    ("period_ends", lambda st, s: st.set_period_totals(s.period_ends, s.period_threshold_nodes, s.period_bins,
                                                       s._period_flux_log2)),
    ("uptake_layers_cm", lambda st, s: st.set_root_uptake(s.uptake_cells, s.uptake_bins)),
    # the shards of an ensemble that runs on several handles (after the sensors and the window)
    ("enkf_shard", lambda st, s: st.set_enkf_shard(*s.enkf_shard, s._shard_exchange[0][1])),
    ("filter_shard", lambda st, s: st.set_filter_shard(*s._shard_exchange[1])),
)


def start(run, s):
    """Set the handle of ``run`` up for the settings ``s`` of :func:`normalise` -- every entry of :data:`START` that is on, in
    order -- and expose them as the run's attributes."""
    for option, call in START:
        if s.on[option]:
            call(run.stepper, s)
    if s.on["filter_shard"]:
        s.filter_shard = run.stepper.filter_shard
    vars(run).update(vars(s))


# ---- 4. which tables a run keeps: the option that turns each entry of the stepper's two registries on ---------------------
TABLE_OPTION = {"filter": "filter_stride", "filter_sm": "filter_soil_moisture", "filter_temper": "filter_ess_floor",
                "filter_rejuvenation": "filter_rejuvenation", "filter_window": "filter_window_offsets", "enkf": "enkf_stride",
                "enkf_sm": "enkf_soil_moisture", "enkf_window": "enkf_window_offsets", "enkf_noise": "enkf_noise_field",
                "profile": "profile_stride", "theta_hist": "theta_hist_bins", "storage": "storage_layers_cm",
                "storage_hist": "storage_bins", "theta_cov": "theta_cov_stride", "conductivity": "conductivity",
                "period": "period_ends",
                "period_acc": "period_ends", "period_hist": "period_bins", "uptake": "uptake_layers_cm",
                "uptake_acc": "uptake_layers_cm", "uptake_hist": "uptake_bins", "wtd_hist": "wtd_hist_stride"}


def tables_on(registry, on):
    """The keys of ``registry`` (stepper.ASSIM_TABLES or DIAG_TABLES) a run with the options ``on`` keeps, in its order."""
    return [key for key in registry if on[TABLE_OPTION[key]]]


# ---- 5. the checkpoint: what each option writes and, beside it, the inverse -------------------------------------------------
def base_carrier(on):
    """The dataset that carries the members' base noise vectors, and with them the damping (``noise_scale`` follows it only
    while nothing else moves the vectors).  The stepper reads it with the method of that name and installs it with
    ``set_`` + name; both directions of the checkpoint ask here."""
    if on["filter_stride"]:
        return "filter_base"             # ... and the ancestry of a filtered run
    if on["enkf_noise_field"]:
        return "enkf_noise_base"         # the analysed vectors
    if on["noise_correlation"]:
        return "noise_field_base"
    return "noise_scale"


def _array(dtype, *shape):
    return lambda a: np.asarray(a, dtype=dtype).reshape(shape or (-1,))


def _tuple(cast, dtype):
    return (lambda v: np.asarray(v, dtype=dtype)), (lambda a: tuple(cast(x) for x in np.asarray(a, dtype=dtype).reshape(-1)))


# (value -> dataset, dataset -> the constructor's value)
_I64, _U64, _F64 = (((lambda v, d=d: np.array(v, dtype=d)), cast)
                    for d, cast in ((np.int64, int), (np.uint64, int), (np.float64, float)))
_PAIRS, _ROWS, _DEPTHS = (np.asarray, _array(np.float64, -1, 2)), (np.asarray, _array(np.int64)), (np.asarray, _array(np.float64))
_LAYERS = (lambda v: np.zeros((0, 2)) if v is None else np.asarray(v, dtype=np.float64)), _array(np.float64, -1, 2)   # (none: [0][2])
_OFFSETS, _FLUX_MAX = _tuple(int, np.int64), _tuple(np.float64, np.float64)
_NODES, _TABLE = (_array(np.int32), None), (lambda a: np.asarray(a, dtype=np.float64), None)
_METHOD = (lambda m: np.array(ENKF_METHODS.index(m), dtype=np.int64)), (lambda a: ENKF_METHODS[int(a)])
_FLAG = (lambda v: np.array(int(v), dtype=np.int64)), (lambda a: bool(int(a)))
_SMOOTHER = _array(np.int64), (lambda a: {"stride": int(_array(np.int64)(a)[0]), "lag_rows": int(np.prod(_array(np.int64)(a)))})

# The settings a checkpoint holds: (the option that must be on, dataset, the two conversions, the run's attribute if it is
# not the dataset's name, the constructor's keyword if it is not the attribute's).  ``a.b``: item b of the dict a.  A run
# without the option keeps its key set.  Keyword None: not handed to the constructor -- the soil-moisture records are supplied
# again at restore, like the forcing, and the correlation's tables are rebuilt from the column and compared (_check_correlation).
SETTING_DATASETS = (
    ("profile_stride", "profile_stride", _I64),
    ("theta_hist_bins", "theta_hist_bins", _I64),
    ("theta_cov_stride", "theta_cov_stride", _I64),
    ("wtd_hist_stride", "wtd_hist_stride", _I64),
    ("storage_layers_cm", "storage_layers_cm", _PAIRS),
    ("storage_layers_cm", "storage_bins", _I64),
    ("conductivity", "conductivity_layers_cm", _LAYERS, "conductivity.layers_cm"),
    ("period_ends", "period_ends", _ROWS),
    ("period_ends", "period_thresholds_cm", _DEPTHS),
    ("period_ends", "period_bins", _I64),
    ("period_bins", "period_flux_max_cm", _FLUX_MAX),
    ("uptake_layers_cm", "uptake_layers_cm", _PAIRS),
    ("uptake_layers_cm", "uptake_bins", _I64),
    ("filter_stride", "filter_stride", _I64),
    ("filter_stride", "filter_sigma_cm", _F64),
    ("filter_stride", "filter_seed", _U64),
    ("filter_soil_moisture", "filter_sm_nodes", _NODES, "filter_soil_moisture.nodes", None),
    ("filter_ess_floor", "filter_ess_floor", _F64),
    ("filter_rejuvenation", "filter_rejuvenation", _F64),  # (the moved vectors are filter_base; the draws are stateless)
    ("filter_window_offsets", "filter_window_offsets", _OFFSETS),
    ("filter_smoother", "filter_smoother", _SMOOTHER),
    ("enkf_stride", "enkf_stride", _I64),
    ("enkf_stride", "enkf_sigma_cm", _F64),
    ("enkf_stride", "enkf_localisation_cm", _F64),
    ("enkf_stride", "enkf_seed", _U64),
    ("enkf_scheme", "enkf_method", _METHOD),               # (a default run keeps its key set)
    ("enkf_scheme", "enkf_relaxation", _F64),
    ("enkf_soil_moisture", "enkf_sm_nodes", _NODES, "enkf_soil_moisture.nodes", None),
    ("enkf_window_offsets", "enkf_window_offsets", _OFFSETS),
    ("enkf_noise_field", "enkf_noise_relaxation", _F64, "enkf_noise_relaxation", "enkf_noise_field.relaxation"),
    ("noise_correlation", "noise_correlation_length_cm", _F64, "noise_correlation.length_cm"),
    ("noise_correlation", "noise_correlation_layers", _FLAG, "noise_correlation.layers"),
    ("noise_correlation", "noise_correlation_a", _TABLE, "noise_correlation_a", None),
    ("noise_correlation", "noise_correlation_b", _TABLE, "noise_correlation_b", None),
    ("forcing_perturbation", "forcing_precipitation_sigma", _F64, "forcing_perturbation.precipitation_sigma"),
    ("forcing_perturbation", "forcing_demand_sigma", _F64, "forcing_perturbation.demand_sigma"),
    ("forcing_perturbation", "forcing_correlation_days", _F64, "forcing_perturbation.correlation_days"),
    ("forcing_perturbation", "forcing_seed", _U64, "forcing_perturbation.seed"),
    ("forcing_enkf", "forcing_enkf_relaxation", _F64, "forcing_perturbation.enkf_relaxation"),
)


def _row(option, dataset, conversions, source=None, *keyword):
    return option, dataset, conversions, source or dataset, keyword[0] if keyword else source or dataset


def checkpoint_datasets(s, stepper=None):
    """What the options of a run ``s`` (or of what :func:`normalise` returned) that are on put into a checkpoint: their
    settings and, given the run's ``stepper``, their live state beyond the registries' tables."""
    out = {}
    for option, dataset, (write, _), source, _ in (_row(*r) for r in SETTING_DATASETS):
        if s.on[option]:
            name, _, item = source.partition(".")
            out[dataset] = write(getattr(s, name)[item] if item else getattr(s, name))
    for option, write, _ in (RUN_STATE + MEMBER_STATE if stepper is not None else ()):
        if write is not None and s.on[option]:
            out.update(write(s, stepper))
    return out


def checkpoint_keywords(data, path, **records):
    """The constructor's keywords out of a checkpoint's datasets -- the inverse of :func:`checkpoint_datasets` -- with the
    soil-moisture records given again (``enkf_soil_moisture=``, ``filter_soil_moisture=``), which must be the ones the
    checkpoint holds the sensors' nodes of."""
    kw = {}
    for _, dataset, (_, read), _, keyword in (_row(*r) for r in SETTING_DATASETS):
        if keyword is not None and dataset in data:
            name, _, item = keyword.partition(".")
            if item:
                kw.setdefault(name, {})[item] = read(data[dataset])
            else:
                kw[name] = read(data[dataset])
    for owner in ("enkf", "filter"):
        arg = owner + "_soil_moisture"
        has, given = owner + "_sm_nodes" in data, records.get(arg)
        if has != (given is not None):
            raise ValueError(f" EnsembleSimulation: {path} was written {'with' if has else 'without'} a soil-moisture "
                             f"record: pass {'the same record' if has else 'none'} as {arg}.")
        if has and not np.array_equal(np.asarray(data[owner + "_sm_nodes"]).reshape(-1), np.asarray(given["nodes"]).reshape(-1)):
            raise ValueError(f" EnsembleSimulation: {path} has sensors at other nodes than {arg}.")
        if has:
            kw[arg] = given
    return kw


# The live state beyond the settings, feature by feature: what it writes from the handle and, beside it, how it goes back.
def _forcing_state(s, st):
    g, day = st.forcing_state()
    return {"forcing_state": g, "forcing_state_day": np.array(day, dtype=np.int64)}


def _set_forcing_state(sim, data, path):
    day = int(_array(np.int64)(data["forcing_state_day"])[0])
    sim.stepper.set_forcing_state(_array(np.float64, 2, -1)(data["forcing_state"]), day)


def _forcing_enkf_table(s, st):
    return {"enkf_forcing_table": st.enkf_forcing_table()}


def _set_forcing_enkf_table(sim, data, path):
    sim.stepper.set_enkf_forcing_table(np.asarray(data["enkf_forcing_table"], dtype=np.float64))


def _check_correlation(sim, data, path):
    if not (np.array_equal(np.asarray(data["noise_correlation_a"]).reshape(-1), sim.noise_correlation_a)
            and np.array_equal(np.asarray(data["noise_correlation_b"]).reshape(-1), sim.noise_correlation_b)):
        raise ValueError(f" EnsembleSimulation: {path} holds the noise correlation's tables of another column.")


def _base(s, st):
    return {base_carrier(s.on): getattr(st, base_carrier(s.on))()}


def _set_base(sim, data, path):
    name = base_carrier(sim.on)
    shape = (sim.n_members,) if name == "noise_scale" else (sim.n_members, sim.cols.dim_d)
    getattr(sim.stepper, "set_" + name)(np.asarray(data[name], dtype=np.float64).reshape(shape))


def _window_capture(owner, what, dtype):
    """What was recorded for the owner's coming assimilation travels along."""
    names = (f"{owner}_window_{what}", f"{owner}_window_rows")
    return (lambda s, st: dict(zip(names, getattr(st, owner + "_window_capture")())),
            lambda sim, data, path: getattr(sim.stepper, f"set_{owner}_window_capture")(
                _array(dtype, -1, sim.n_members)(data[names[0]]), np.asarray(data[names[1]], dtype=np.int64)))


def _smoother(s, st):
    """The tables and the ring, with the last row stepped."""
    w, ids, rows, last = st.filter_smoother_ring()
    return {"filter_smoother_hist": st.filter_smoother_hist(), "filter_smoother_paths": st.filter_smoother_paths(),
            "filter_smoother_ring_w": w, "filter_smoother_ring_id": ids, "filter_smoother_ring_rows": np.append(rows, last)}


def _set_smoother(sim, data, path):
    st, n = sim.stepper, sim.n_members
    st.set_filter_smoother_hist(np.asarray(data["filter_smoother_hist"]))
    st.set_filter_smoother_paths(np.asarray(data["filter_smoother_paths"], dtype=np.int64))
    rows = _array(np.int64)(data["filter_smoother_ring_rows"])
    st.set_filter_smoother_ring(_array(np.int32, -1, n)(data["filter_smoother_ring_w"]),
                                _array(np.int64, -1, n)(data["filter_smoother_ring_id"]), rows[:-1], int(rows[-1]))


# (option, what it writes from the handle or None, how restore installs it) in the order restore installs them: the run's
# before the members' state and the filters' tables, the members' after them
RUN_STATE = (
    ("forcing_perturbation", _forcing_state, _set_forcing_state),
    ("forcing_enkf", _forcing_enkf_table, _set_forcing_enkf_table),      # (no entry of the stepper's registry: its own row)
    ("noise_correlation", None, _check_correlation),
)
MEMBER_STATE = (
    ("always", _base, _set_base),
    ("filter_window_offsets", *_window_capture("filter", "index", np.int32)),
    ("filter_smoother", _smoother, _set_smoother),
    ("enkf_window_offsets", *_window_capture("enkf", "y", np.float64)),
)


def install_state(features, sim, data, path):
    """The live state of ``features`` (RUN_STATE or MEMBER_STATE) from a checkpoint into the handle of ``sim``."""
    for option, _, install in features:
        if sim.on[option]:
            install(sim, data, path)
