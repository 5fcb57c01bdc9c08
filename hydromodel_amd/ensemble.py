"""Ensemble driver: N stochastic realisations of one soil column on one GPU (one rank).

Per-member semantics are those of ``Simulation.run`` (``/root/reference/code/src/simulation.py:495-672``):
member k has its own noise stream, all members share forcing, tables and (by default) the
initial condition produced by the spin-up of ``Simulation.initial_conditions`` (``:389-493``).
Ranks shard members with no communication while stepping; the only collective is the final
all-reduce of the per-row water-table moments (see :func:`allreduce_moments`).
"""
import numpy as np

from . import settings
from .digest import inverse_retention
from .stepper import DIAG_TABLES, MORE_DIAG_TABLES, diag_checkpoint, diag_from_checkpoint
from .stepper import (ASSIM_TABLES, EnsembleStepper, enkf_forcing_summary, enkf_noise_summary, enkf_sm_summary, enkf_summary,
                      enkf_window_summary, filter_sm_summary, filter_smoother_summary, filter_summary, filter_window_summary, layer_ranges,
                      layer_storage_distribution, moments_to_mean_std, period_totals_distribution, root_uptake_distribution,
                      root_uptake_profile, root_uptake_stats, theta_cov_finish, theta_distribution, theta_sensor_gain,
                      wtd_distribution)


def pressure_head(cols, theta):
    """Inverse van Genuchten -- ``HydrologicalModel.pressure_head`` (hydrological_model.py:43-119).

    The reference interpolates the porosity AT the grid knots here (``self.porous(z)`` with the
    full grid), i.e. ``cols.por_node``.  Returns (psi, s_eff).
    """
    theta = np.atleast_1d(np.asarray(theta, dtype=float))
    if theta.shape[0] != cols.dim_d:
        raise ValueError(f" HydrologicalModel: Input size dimensions don't match:"
                         f" {theta.shape[0]} not equal to {cols.dim_d}.")
    soil = cols.soil
    return inverse_retention(theta, cols.por_node, cols.theta.res, soil.alpha, soil.n, soil.m,
                             max(soil.epsilon, 1.0e-8), cols.dz)


def spinup_on_gpu(cols, forcing, n_rnd, device=0, burn_in=1500, flags=None, verbose=False, well_no=None):
    """``Simulation.initial_conditions`` (simulation.py:389-493) with the solves on the GPU.

    Forcing row 0, fixed noise vector, SPINUP semantics, t_span = (0, 1); stops when the
    estimated water table is within 2*dz of the first observation and the mean squared change
    of the state is <= 0.01.  Returns (psi0, iterations, early_stop).
    """
    z = cols.z
    y0, _ = pressure_head(cols, cols.por_raw)
    st = EnsembleStepper(cols, forcing, 1, device=device, flags=flags)
    try:
        st.set_state(y0)
        st.set_noise_host(np.asarray(n_rnd, dtype=float)[None, :])
        early_stop, j = False, -1
        for j in range(burn_in):
            out = st.step_rows(0, 1, spinup=True, moments=False, want_wtd=True)
            y_j = st.get_state()[0]
            wtd_est = int(out["wtd"][0, 0])
            abs_error = np.abs(forcing.zwtd_cm[0] - z[wtd_est])
            mse_0 = np.mean((y_j - y0) ** 2)
            y0 = y_j.copy()
            if abs_error <= (2.0 * cols.dz) and (mse_0 <= 0.01):
                early_stop = True
                if verbose:
                    print(f" [Initial Conditions for Well no. {well_no}]"
                          f" finished at [itr: {j}] with [abs(error): {abs_error}]"
                          f" and [MSE: {mse_0}]")
                break
        if verbose and not early_stop:
            print(f" [Initial Conditions for Well no. {well_no}]"
                  f" finished at maximum number of iterations.")
    finally:
        st.close()
    return y0, j + 1, early_stop


PHILOX_DRAW_SPINUP = 0xFFFFFFFF          # include/hydrocol.h: HC_PHILOX_DRAW_SPINUP


def spinup_members_on_gpu(stepper, cols, forcing, burn_in=1500):
    """``Simulation.initial_conditions`` for EVERY member of `stepper` at once: each member starts
    from the hydrostatic-like profile of simulation.py:409-414, keeps the noise source already installed in
    `stepper` (host vectors or its Philox stream, draw 0), and stops by its own rule (simulation.py:468), all
    inside one kernel launch.  Returns (psi0[N][D], iterations[N]); iterations < 0 marks members that ran into
    `burn_in` (the reference prints "finished at maximum number of iterations" and carries on)."""
    y0, _ = pressure_head(cols, cols.por_raw)
    stepper.set_state(y0)
    iters, _ = stepper.spinup(forcing.zwtd_cm[0], cols.z[0], forcing_row=0, max_iterations=burn_in)
    return stepper.get_state(), iters


def member_generators(seed, n_members, member_offset=0):
    """NumPy streams of a parity-style ensemble: global member 0 consumes exactly the
    reference's ``default_rng(SeedSequence(seed))`` (simulation.py:66-70); member k >= 1 uses
    ``SeedSequence(seed, spawn_key=(k,))``."""
    from numpy.random import SeedSequence, default_rng
    gens = []
    for k in range(member_offset, member_offset + n_members):
        gens.append(default_rng(SeedSequence(seed) if k == 0 else SeedSequence(seed, spawn_key=(k,))))
    return gens


class _Run:
    """What an ensemble and a sweep share: one handle (``stepper``) stepped from ``next_row`` on, and its optional tables.

    profile_stride > 0: ensemble profile statistics (psi, theta every ``profile_stride``-th row from row 0 = the initial
    states, fluxes and abs_error every solved row) accumulated on the device: :meth:`profile_stats`.
    theta_hist_bins > 0 (32, 64 or 128; needs profile_stride): exact histograms of theta_vol at every node of the profile
    rows, counted on the device: :meth:`theta_distribution` (quantile bands of theta(z)).
    storage_layers_cm (needs profile_stride): depth layers [(top, bottom), ...] in cm (stepper.layer_ranges) whose water
    storage dz sum theta is reduced per member on the device on the profile rows: :meth:`storage_stats` (mean and sigma in
    cm) and, with ``storage_bins`` (a power of two in 32 .. 1024), :meth:`storage_distribution` (quantile bands in cm).
    theta_cov_stride > 0 (needs profile_stride): the exact second moments of theta_vol at the nodes 0, s, 2 s, ... and of
    the water table on the profile rows (include/hydrocol.h hc_set_theta_cov): :meth:`theta_covariance` (covariance and
    correlation of theta(z), cov(theta, wtd)) and, at stride 1, :meth:`layer_std_cm` (the sigma of any layer's storage).
    conductivity (needs profile_stride): ``True`` or ``{"layers_cm": [(top, bottom), ...]}``: ln K_hrc and ln K_bkg of every
    member at every node of the profile rows, evaluated with the noise vector the row was solved with, and ln of the
    layers' effective vertical conductivity n / sum 1 / K_hrc (at most 8 layers, stepper.layer_ranges), as exact integer
    moments (include/hydrocol.h hc_set_conductivity_stats): :meth:`conductivity_stats` (mean and sigma of ln K, geometric
    mean K in cm per row).  While it is on, a launch ends on every profile row; the members' states do not depend on it.
    period_ends: the inclusive end rows of periods (stepper.period_ends) over which every member's transpiration and
    lateral flow are summed, its shallowest and deepest water table kept and the rows counted on which the water table
    stood at or above each of ``period_thresholds_cm`` (at most 4 depths, mapped to nodes like a sensor's), reduced over
    the members on the device at every end row: :meth:`period_stats` and, with ``period_bins`` (a power of two in
    32 .. 1024) and ``period_flux_max_cm`` = the histograms' upper ends (transpiration, lateral flow), each a power of two
    in 2^-8 .. 2^12 cm, :meth:`period_distribution`.  Needs no profile statistics.
    wtd_hist_stride > 0: per-row histograms of the members' water-table index every ``wtd_hist_stride``-th row, counted on
    the device: :meth:`wtd_distribution` (quantiles, CRPS against the well).
    filter_stride > 0: a bootstrap particle filter on the well's water table every ``filter_stride``-th row with an
    observation (``filter_sigma_cm``: the observation error; ``filter_seed``: default the run's seed): the tables above
    describe the forecast, the states continue from the analysis; :meth:`filter_summary` (ESS, log marginal likelihood).
    filter_soil_moisture: a soil-moisture record (stepper.soil_moisture_record) that joins the well in the filter's
    weights, which then belong to a member and not to a 5 cm bin (include/hydrocol.h hc_set_filter_soil_moisture);
    :meth:`filter_sm_table`, the ``sm_*`` keys of :meth:`filter_summary`.
    filter_ess_floor: 0 < f < 1 holds the effective sample size of every resampling above f times the counted members by
    tempering the weights (include/hydrocol.h hc_set_filter_tempering); :meth:`filter_temper_table`, and
    :meth:`filter_summary` gains ``beta``, ``ess_tempered``, ``ess_target`` and ``tempered_rows``.
    filter_rejuvenation: Liu & West's discount 0.5 <= delta < 1: after every resampling that copied a member the point's
    base noise vectors -- the members' conductivity fields, which resampling otherwise only ever loses -- are pulled
    towards their mean and jittered, so that mean and variance per node stay what the resampling left and no two members
    share a field (include/hydrocol.h hc_set_filter_rejuvenation); :meth:`filter_rejuvenation_table`, and
    :meth:`filter_summary` gains ``rejuvenated``, ``rejuvenation_refused``, ``noise_std_resampled``,
    ``noise_std_rejuvenated`` and ``rejuvenated_rows``.  With a single survivor there is no spread to restore: give a
    ``filter_ess_floor`` as well.
    filter_window_offsets: rows before each assimilation row (integers in [1, filter_stride), e.g. (12, 24, 36)) whose
    observation of the well joins the members' weights too: nothing is resampled in between, so a member's weight is the
    likelihood of everything its trajectory passed (include/hydrocol.h hc_set_filter_window);
    :meth:`filter_window_table`, the ``window_*`` keys of :meth:`filter_summary`.
    enkf_stride > 0: a stochastic ensemble Kalman filter on the well's continuous water table instead (``enkf_sigma_cm``:
    the observation error; ``enkf_localisation_cm``: the Gaspari-Cohn half-width, 0 = none; ``enkf_seed``: default the
    run's seed), with the same forecast / analysis order; :meth:`enkf_summary` (log marginal likelihood).
    enkf_soil_moisture: a soil-moisture record (stepper.soil_moisture_record: ``nodes``, ``values`` [T][n], ``sigma``,
    ``depths_cm``) that joins the well in the EnKF's analyses; :meth:`enkf_sm_table`, the ``sm_*`` keys of
    :meth:`enkf_summary`.
    enkf_method: "stochastic" (perturbed observations, the default) or "sqrt" (the deterministic square-root analysis);
    enkf_relaxation: the relaxation to prior spread alpha in [0, 1] (default 0 = none) of either
    (include/hydrocol.h hc_set_enkf_method); both need the EnKF.
    enkf_noise_field: True or {"relaxation": a}: every analysis also updates the members' base noise vectors -- their
    conductivity fields -- with the same observations, draws and factor (include/hydrocol.h hc_set_enkf_noise_field),
    relaxed to prior spread with ``a`` (default: enkf_relaxation); the ``noise_*`` keys of :meth:`enkf_summary`.
    Parameters regain no spread from the dynamics: without a relaxation a long run collapses the field.
    filter_smoother: ``{"stride": s, "lag_rows": L}`` (L a multiple of s, L / s <= 64): the fixed-lag smoother of the water
    table by ancestry -- every slot carries its ancestors' water-table indices of each s-th row through the resamplings, and
    the row is counted L rows later: its distribution given the well's record up to then, the one table that describes the
    posterior (include/hydrocol.h hc_set_filter_smoother); :meth:`filter_smoothed`.  Not with filter_shard.
    enkf_window_offsets: rows before each analysis row (integers in [1, enkf_stride), e.g. (12, 24, 36)) on which the
    well's record joins that analysis too -- the asynchronous EnKF (include/hydrocol.h hc_set_enkf_window);
    :meth:`enkf_window_table`, the ``window_*`` keys of :meth:`enkf_summary`.
    forcing_perturbation: {"precipitation_sigma": .., "demand_sigma": .., "correlation_days": .., "seed": ..} or None: every
    member sees the record's rainfall and atmospheric demand times a log-normal factor of mean one of its own, constant
    over a day and an AR(1) from day to day (include/hydrocol.h hc_set_forcing_perturbation); at least one sigma, in
    [0, 1]; correlation_days in [0, 365], default 0; seed default: the ensemble's.  Set after the spin-up, before the
    filters; the particle filter moves the members' state with them; ``dump`` / ``restore`` carry it.  With the further
    key ``"enkf_relaxation": a`` (a in [0, 1]; absent or None: off) every EnKF analysis also updates the members' forcing
    state from the same observations, draws and factor (include/hydrocol.h hc_set_enkf_forcing), relaxed to prior spread
    with ``a``; it needs enkf_stride > 0 and no enkf_shard; :meth:`enkf_forcing_table`, the ``forcing_*`` keys of
    :meth:`enkf_summary`.
    noise_correlation: {"length_cm": l, "layers": bool} or None: the Philox source's base and refresh vectors become
    exponentially correlated fields of unit variance down the column (include/hydrocol.h hc_set_noise_correlation),
    with ``layers`` independent across the interfaces of ``cols.layers`` inside the column; applied after the spin-up
    and before the filters, one table per point.  Not with noise="numpy" nor with filter_rejuvenation.
    ``_lead`` is the leading shape of the per-point tables: () for an ensemble, (P,) for a sweep."""

    _lead = ()

    def noise_correlation_break_count(self):
        """Breaks of the recursion below node 0, over all points."""
        a = np.asarray(self.noise_correlation_a).reshape(-1, self.cols.dim_d)
        return int((a[:, 1:] == 0.0).sum())

    def assim_table(self, key):
        """The handle's assimilation table ``key`` (stepper.ASSIM_TABLES): [n_arow] + its trailing shape, a sweep:
        [P][n_arow] + ...  The named accessors below document each table."""
        t = self.stepper.assim_table(key)
        return t.reshape(self._lead + t.shape[1:])

    def assim_tables_on(self):
        """The keys of stepper.ASSIM_TABLES this run keeps, in the registry's order: what a checkpoint carries."""
        return settings.tables_on(ASSIM_TABLES, self.on)

    def diag_tables_on(self):
        """The keys of stepper.DIAG_TABLES this run keeps, in the registry's order: what a checkpoint carries and installs."""
        return settings.tables_on({**DIAG_TABLES, **MORE_DIAG_TABLES}, self.on)


    def enkf_noise_table(self):
        """[n_arow][4 D + 1] float64 (include/hydrocol.h hc_set_enkf_noise_field); a sweep: [P][n_arow][4 D + 1]."""
        return self.assim_table("enkf_noise")

    def enkf_noise_summary(self, table=None):
        """stepper.enkf_noise_summary of the noise field's table (``table``: e.g. the one assembled over ranks)."""
        t = self.enkf_noise_table() if table is None else table
        return enkf_noise_summary(t, self.enkf_stride, self.enkf_noise_relaxation, self.cols.dim_d)

    def advance(self, n_rows, **kw):
        """Solve the next ``n_rows`` forcing rows for every member."""
        out = self.stepper.step_rows(self.next_row, n_rows, **kw)
        self.next_row += n_rows
        self.kernel_ms += out["kernel_ms"]
        self.launches += out["launches"]
        return out

    def moments(self):
        """[3][T]; a sweep: [P][3][T]"""
        return np.asarray(self.stepper.moments()).reshape(self._lead + (3, self.forcing.dim_t))

    def profile_table(self):
        return self.stepper.profile_table()

    def profile_stats(self, table=None):
        """theta_vol / psi_press / S_eff mean and sigma [T_out][D], transpiration / lateral_flow mean and sigma and
        abs_error_mean [T], rows, count (stepper.profile_tables_to_stats), with a leading [P] axis when the handle holds
        several points; ``table``: e.g. the sum over ranks."""
        return self.stepper.profile_stats(table)

    def theta_hist_table(self):
        """[n_prow][D][B] int32: members per bin of theta at every node of every profile row (stepper.theta_hist_of); a
        sweep: [P][n_prow][D][B]."""
        return self.stepper.theta_hist_table().reshape(self._lead + (-1, self.cols.dim_d, self.theta_hist_bins))

    def theta_distribution(self, levels=(0.05, 0.25, 0.5, 0.75, 0.95), table=None):
        """Quantile bands of theta(z) per profile row (stepper.theta_distribution), with the leading shape of the table;
        ``table``: e.g. the sum over ranks.  Other levels need no rerun."""
        t = self.theta_hist_table() if table is None else table
        return theta_distribution(t, levels, self.theta_hist_bins, self.profile_stride)

    def theta_cov_table(self):
        """[n_prow][W] int64: count, S1, S2 of the selected nodes and the water table on every profile row
        (stepper.theta_cov_of); a sweep: [P][n_prow][W]."""
        t = self.stepper.theta_cov_table()
        return t.reshape(self._lead + t.shape[1:])

    def theta_covariance(self, table=None, sensor_sigma=None):
        """The ensemble's second-order structure per profile row (stepper.theta_cov_finish), with the leading shape of
        the table: ``theta_cov`` [T_out][n][n], ``wtd_theta_cov_cm`` [T_out][n], ``wtd_var_cm2`` [T_out], ``theta_wtd_corr``
        [T_out][n], ``theta_corr``, ``theta_mean``, ``wtd_mean_idx`` and ``count``, with ``rows``, ``node_stride``,
        ``nodes`` and ``depth_cm`` [n]; with ``sensor_sigma`` [m3/m3] also ``theta_sensor_gain`` [T_out][n]
        (stepper.theta_sensor_gain).  ``table``: e.g. the sum over ranks."""
        t = self.theta_cov_table() if table is None else table
        out = theta_cov_finish(t, self.cols.dz, self.theta_cov_stride, self.cols.dim_d)
        nodes = np.arange(0, self.cols.dim_d, self.theta_cov_stride, dtype=np.int64)
        out.update(rows=np.arange(np.asarray(t).shape[-2], dtype=np.int64) * self.profile_stride,
                   node_stride=self.theta_cov_stride, nodes=nodes, depth_cm=np.asarray(self.cols.z, dtype=np.float64)[nodes])
        if sensor_sigma is not None:
            out["theta_sensor_gain"] = theta_sensor_gain(out, sensor_sigma)
        return out

    def layer_std_cm(self, layers_cm, table=None):
        """The sigma [cm] of the water stored in each of the depth layers ``layers_cm`` = [(top, bottom), ...]
        (stepper.layer_ranges) per profile row, dz sqrt(1' C 1) over the layer's nodes of the covariance table:
        [T_out][L] (a sweep: [P][T_out][L]).  The layers are named after the run; needs a node stride of 1."""
        if self.theta_cov_stride != 1:
            raise ValueError("layer_std_cm needs the covariance of every node "
                             f"(theta_cov_stride = 1, not {self.theta_cov_stride})")
        C = self.theta_covariance(table)["theta_cov"]
        out = [np.sqrt(np.maximum(C[..., i0:i1, i0:i1].sum(axis=(-2, -1)), 0.0))
               for i0, i1 in layer_ranges(self.cols.z, layers_cm)]
        return float(self.cols.dz) * np.stack(out, axis=-1)


    def period_table(self):
        """The raw int64 moments table of the period totals (stepper.period_totals_table_layout)."""
        return self.stepper.period_totals_table()

    def period_hists(self):
        """(phist_flux [n_period][2][B], phist_wtd [n_period][2][D]) int32; a sweep: a leading [P] axis."""
        hf, hw = self.stepper.period_totals_hists()
        return hf.reshape(self._lead + hf.shape[1:]), hw.reshape(self._lead + hw.shape[1:])

    def period_stats(self, table=None):
        """Mean and sigma over the members of every period's transpiration and lateral-flow totals [cm], shallowest and
        deepest water table [cm depth] and rows at or above each threshold, [n_period] (a sweep: [P][n_period]), with
        end_rows, solved_rows and count (stepper.period_totals_stats); ``table``: e.g. the sum over ranks."""
        out = self.stepper.period_totals_stats(table)
        out["thresholds_cm"], out["threshold_nodes"] = self.period_thresholds_cm.copy(), self.period_threshold_nodes.copy()
        return out

    def period_distribution(self, levels=(0.05, 0.25, 0.5, 0.75, 0.95), tables=None):
        """Quantiles over the members of every period's flux totals [cm] and water-table extremes [cm depth]
        (stepper.period_totals_distribution); ``tables`` = (phist_flux, phist_wtd): e.g. the sums over ranks.  Other
        levels need no rerun."""
        hf, hw = self.period_hists() if tables is None else tables
        return period_totals_distribution(hf, hw, levels, self.stepper.period_flux_max_log2, float(self.cols.z[0]),
                                          self.cols.dz)


    def uptake_table(self):
        """The raw int64 table of the root uptake (stepper.root_uptake_table_layout)."""
        return self.stepper.root_uptake_table()

    def uptake_hist(self):
        """[n_period][L][B] int32 share histograms; a sweep: a leading [P] axis."""
        h = self.stepper.root_uptake_hist()
        return h.reshape(self._lead + h.shape[1:])

    def uptake_stats(self, table=None):
        """Mean and sigma over the members of every period's root-water uptake [cm], in total and per layer of
        ``uptake_layers_cm``, [n_period] and [n_period][L] (a sweep: a leading [P] axis), the layers' shares of the mean
        total, count and end_rows (stepper.root_uptake_stats); ``table``: e.g. the sum over ranks."""
        t = self.uptake_table() if table is None else table
        out = root_uptake_stats(t, self.stepper.P, self.period_ends, len(self.uptake_cells), self.cols.dim_d)
        out["layers_cm"], out["cells"] = self.uptake_layers_cm.copy(), self.uptake_cells.copy()
        return out

    def uptake_distribution(self, levels=(0.05, 0.5, 0.95), hist=None):
        """Quantiles over the members of each layer's share of a member's period total (stepper.root_uptake_distribution);
        ``hist``: e.g. the sum over ranks.  Needs ``uptake_bins``; other levels need no rerun."""
        return root_uptake_distribution(self.uptake_hist() if hist is None else hist, levels)

    def uptake_profile(self, table=None):
        """Every period's uptake per cm of depth at the midpoints, the mean over the members, [n_period][D - 1], and the
        depths above which 50 % and 90 % of it lie (stepper.root_uptake_profile); ``table``: e.g. the sum over ranks."""
        t = self.uptake_table() if table is None else table
        return root_uptake_profile(t, self.stepper.P, self.period_ends, len(self.uptake_cells), self.cols.dim_d, self.cols.z)

    def storage_table(self):
        """The raw int64 moments table of the layer storage (stepper.layer_storage_table_layout)."""
        return self.stepper.layer_storage_table()

    def storage_stats(self, table=None):
        """Mean and sigma of every layer's storage in cm per profile row, [T_out][L] (a sweep: [P][T_out][L]), with rows and
        count (stepper.layer_storage_stats); ``table``: e.g. the sum over ranks."""
        out = self.stepper.layer_storage_stats(table)
        out["layers_cm"], out["nodes"] = self.storage_layers_cm.copy(), self.storage_ranges.copy()
        return out

    def conductivity_table(self):
        """The raw int64 table of the conductivity statistics (stepper.conductivity_table_layout)."""
        return self.stepper.conductivity_table()

    def conductivity_stats(self, table=None):
        """Mean and sigma of ln K_hrc and ln K_bkg and the geometric-mean K per profile row and node, [T_out][D] (a sweep:
        [P][T_out][D]), with the members added per node and quantity and, with layers, the same of the layers' effective
        conductivity [T_out][L] (stepper.conductivity_stats); ``table``: e.g. the sum over ranks."""
        out = self.stepper.conductivity_stats(table)
        if self.conductivity_ranges is not None and len(self.conductivity_ranges):
            out["layers_cm"], out["nodes"] = np.asarray(self.conductivity["layers_cm"]).copy(), self.conductivity_ranges.copy()
        return out

    def storage_hist_table(self):
        """[n_prow][L][B] int32: members per bin of each layer's mean theta on every profile row; a sweep: [P][n_prow][L][B]."""
        return self.stepper.layer_storage_hist_table().reshape(self._lead + (-1, len(self.storage_ranges), self.storage_bins))

    def storage_distribution(self, levels=(0.05, 0.25, 0.5, 0.75, 0.95), table=None):
        """Quantile bands of every layer's storage in cm per profile row (stepper.layer_storage_distribution), with the
        leading shape of the table; ``table``: e.g. the sum over ranks.  Other levels need no rerun."""
        t = self.storage_hist_table() if table is None else table
        return layer_storage_distribution(t, self.storage_ranges, self.cols.dz, levels, self.profile_stride)

    def wtd_hist_table(self):
        """[n_hrow][D] int32: members per water-table index on every histogram row (stepper.wtd_hist_rows); a sweep:
        [P][n_hrow][D], one table per parameter point of this handle."""
        return self.stepper.wtd_hist_table().reshape(self._lead + (-1, self.cols.dim_d))

    def wtd_distribution(self, levels=(0.05, 0.25, 0.5, 0.75, 0.95), table=None):
        """Quantiles of the water-table depth and CRPS against the well per histogram row (stepper.wtd_distribution), with
        the leading shape of the table; ``table``: e.g. the sum over ranks."""
        t = self.wtd_hist_table() if table is None else table
        return wtd_distribution(t, self.forcing.wtd_obs, levels, self.cols.dz, self.cols.z, self.device,
                                self.wtd_hist_stride)

    def filter_table(self):
        """[n_arow][4] float64 (count, ESS, log-likelihood increment, survivors per assimilation slot); a sweep: [P][n_arow][4]."""
        return self.assim_table("filter")

    def filter_temper_table(self):
        """[n_arow][4] float64 (beta, the ESS at beta, the target, the trials; include/hydrocol.h
        hc_set_filter_tempering); a sweep: [P][n_arow][4]."""
        return self.assim_table("filter_temper")

    def filter_rejuvenation_table(self):
        """[n_arow][4] float64 (applied, members refused, the base vectors' spread before and after the move;
        include/hydrocol.h hc_set_filter_rejuvenation); a sweep: [P][n_arow][4]."""
        return self.assim_table("filter_rejuvenation")

    def filter_summary(self, table=None, sm_table=None, temper_table=None, window_table=None, rejuvenation_table=None):
        """The filter's record (stepper.filter_summary): ``rows``, ``count``, ``ess``, ``loglik_rows``, ``survivors`` over
        the assimilated rows and ``loglik``, the log marginal likelihood of the well record (log cm^-1 summed over the rows),
        with a leading [P] for a sweep; ``table``: e.g. the one assembled over ranks.  With a soil-moisture record the
        increments of the sensor rows are the joint ones, and the ``sm_*`` keys of :meth:`filter_sm_summary` come along.
        With ``filter_ess_floor`` the tempering's ``beta``, ``ess_tempered``, ``ess_target`` and ``tempered_rows`` too
        (``temper_table``: as ``table``).  With a window the ``window_*`` keys of :meth:`filter_window_summary` too.  With
        ``filter_rejuvenation`` the ``rejuvenated`` ... keys (``rejuvenation_table``: as ``table``)."""
        t = self.filter_table() if table is None else table
        if getattr(self, "filter_ess_floor", 0.0) and temper_table is None:      # (0.0: a run started without the setting)
            temper_table = self.filter_temper_table()
        if getattr(self, "filter_rejuvenation", 0.0) and rejuvenation_table is None:
            rejuvenation_table = self.filter_rejuvenation_table()
        out = filter_summary(t, self.filter_stride, self.filter_sigma_cm, temper_table=temper_table,
                             rejuvenation_table=rejuvenation_table)
        if self.filter_soil_moisture is not None:
            out.update(("sm_" + k, v) for k, v in self.filter_sm_summary(sm_table).items())
        if getattr(self, "filter_window_offsets", ()):
            out.update(("window_" + k, v) for k, v in self.filter_window_summary(window_table).items())
        return out

    def filter_smoothed(self, levels=(0.05, 0.5, 0.95), hist=None, paths=None):
        """The smoothed water-table distributions (include/hydrocol.h hc_set_filter_smoother): flushes the ring -- every
        pending row is emitted with the lag it reached -- and returns stepper.filter_smoother_summary of the tables
        (``hist`` / ``paths``: e.g. those assembled over ranks, after each rank's own flush): ``rows``, ``count``,
        ``hist``, ``quantile_cm``, ``crps_cm`` against the well, ``crps_mean_cm``, ``lag_rows`` (the lag each row really
        got) and ``unique_paths`` (towards 1 the histogram is one trajectory: hold the ESS up with filter_ess_floor, or
        take a shorter lag); a sweep: a leading [P].  This is the one table that describes the posterior."""
        if getattr(self, "filter_smoother", None) is None:
            raise ValueError(f" {self.__class__.__name__}: no smoother (filter_smoother).")
        self.stepper.filter_smoother_flush()
        h = self.stepper.filter_smoother_hist() if hist is None else np.asarray(hist)
        p = self.stepper.filter_smoother_paths() if paths is None else np.asarray(paths)
        if hist is None:
            h = h.reshape(self._lead + h.shape[1:])
        if paths is None:
            p = p.reshape(self._lead + p.shape[1:])
        return filter_smoother_summary(h, p, self.forcing.wtd_obs, levels, self.cols.dz, self.cols.z,
                                       self.filter_smoother[0], device=self.stepper.device)

    def filter_window_table(self):
        """[n_arow][n][4] float64 (include/hydrocol.h hc_set_filter_window); a sweep: [P][n_arow][n][4]."""
        return self.assim_table("filter_window")

    def filter_window_summary(self, table=None):
        """stepper.filter_window_summary of the window's table (``table``: e.g. the one assembled over ranks): per
        assimilation row and offset the lagged observation, the forecast of the members' water table there and the
        innovation."""
        t = self.filter_window_table() if table is None else table
        return filter_window_summary(t, self.filter_stride, self.filter_window_offsets, float(self.cols.z[0]))

    def filter_sm_table(self):
        """[n_arow][n][6] float64 (include/hydrocol.h hc_set_filter_soil_moisture); a sweep: [P][n_arow][n][6]."""
        return self.assim_table("filter_sm")

    def filter_sm_summary(self, table=None):
        """stepper.filter_sm_summary of the filter's sensor table (``table``: e.g. the one assembled over ranks)."""
        t = self.filter_sm_table() if table is None else table
        return filter_sm_summary(t, self.filter_stride, self.filter_soil_moisture["sigma"])

    def enkf_table(self):
        """[n_arow][8] float64 (include/hydrocol.h hc_set_enkf; depths from the top node); a sweep: [P][n_arow][8]."""
        return self.assim_table("enkf")

    def enkf_forcing_table(self):
        """[n_arow][9] float64 (include/hydrocol.h hc_set_enkf_forcing); a sweep: [P][n_arow][9]."""
        t = self.stepper.enkf_forcing_table()
        return t.reshape(self._lead + t.shape[1:])

    def enkf_forcing_summary(self, table=None):
        """stepper.enkf_forcing_summary of the forcing analysis's table (``table``: e.g. the one assembled over ranks)."""
        t = self.enkf_forcing_table() if table is None else table
        return enkf_forcing_summary(t, self.enkf_stride, self.forcing_perturbation["enkf_relaxation"])

    def enkf_summary(self, table=None, sm_table=None, window_table=None, noise_table=None, forcing_table=None):
        """The EnKF's record (stepper.enkf_summary, means at the well's depths): ``rows``, ``count``, ``prior_mean_cm``,
        ``prior_std_cm``, ``innovation_cm``, ``loglik_rows``, ``post_mean_cm``, ``post_std_cm``, ``rejected`` over the
        analysed rows and ``loglik``, the log marginal likelihood of the well record (log cm^-1), with a leading [P] for a
        sweep, and the analysis scheme, ``method`` and ``relaxation``; ``table``: e.g. the one assembled over ranks.
        With a window the ``window_*`` keys of :meth:`enkf_window_summary` too."""
        t = self.enkf_table() if table is None else table
        out = enkf_summary(t, self.enkf_stride, self.enkf_sigma_cm, float(self.cols.z[0]))
        out.update(method=self.enkf_method, relaxation=self.enkf_relaxation)
        if self.enkf_soil_moisture is not None:
            out.update(("sm_" + k, v) for k, v in self.enkf_sm_summary(sm_table).items())
        if self.enkf_window_offsets:
            out.update(("window_" + k, v) for k, v in self.enkf_window_summary(window_table).items())
        if self.enkf_noise_relaxation is not None:      # the noise_* keys (include/hydrocol.h hc_set_enkf_noise_field)
            out.update((k, v) for k, v in self.enkf_noise_summary(noise_table).items() if k.startswith("noise_"))
        if self.on["forcing_enkf"]:                     # the forcing_* keys (include/hydrocol.h hc_set_enkf_forcing)
            out.update((k, v) for k, v in self.enkf_forcing_summary(forcing_table).items() if k.startswith("forcing_"))
        return out

    def enkf_window_table(self):
        """[n_arow][n][4] float64 (include/hydrocol.h hc_set_enkf_window); a sweep: [P][n_arow][n][4]."""
        return self.assim_table("enkf_window")

    def enkf_window_summary(self, table=None):
        """stepper.enkf_window_summary of the window's table (``table``: e.g. the one assembled over ranks): per
        analysis row and offset the lagged observation, the prior of the recorded y and the innovation."""
        t = self.enkf_window_table() if table is None else table
        return enkf_window_summary(t, self.enkf_stride, self.enkf_window_offsets, float(self.cols.z[0]))

    def enkf_sm_table(self):
        """[n_arow][n][6] float64 (include/hydrocol.h hc_set_enkf_soil_moisture); a sweep: [P][n_arow][n][6]."""
        return self.assim_table("enkf_sm")

    def enkf_sm_summary(self, table=None):
        """stepper.enkf_sm_summary of the sensor table (``table``: e.g. the one assembled over ranks): per sensor the
        forecast RMSE of the mean against the record (``rmse``) and the mean innovation, over the joint analyses."""
        t = self.enkf_sm_table() if table is None else table
        return enkf_sm_summary(t, self.enkf_stride, self.enkf_soil_moisture["sigma"])

    def close(self):
        self.stepper.close()


class EnsembleSimulation(_Run):
    """N members of one parameter point on one device.

    noise="philox" (default): counter-based normals generated in the kernel, keyed by the global member id.
    noise="numpy": host NumPy streams (`member_generators`), drawn in the reference's order -- #0 spin-up,
    #1 base vector, then one vector per refresh row (simulation.py:426,561,601) -- and uploaded per launch.
    spinup="shared" (default): one spin-up (global member 0's first draw) broadcast to all members;
    spinup="member": every member spins up with its own first draw (`spinup_members_on_gpu`).
    profile_stride, theta_hist_bins, storage_layers_cm / storage_bins, theta_cov_stride, period_ends /
    period_thresholds_cm / period_bins / period_flux_max_cm, wtd_hist_stride, filter_stride / filter_sigma_cm /
    filter_seed, enkf_stride / enkf_sigma_cm / enkf_localisation_cm / enkf_seed: the optional tables, the particle filter and the EnKF (:class:`_Run`).
    enkf_shard=(n_global, exchange): these members are [member_offset, member_offset + N) of an ensemble of ``n_global``
    whose other members run elsewhere, and the EnKF analyses the whole of it (include/hydrocol.h hc_set_enkf_shard;
    ``exchange``: e.g. a ``multigpu.ShardExchange``).  member_offset must be a multiple of 256, and so must N unless the
    block is the ensemble's last.  Set up by the run: a checkpoint does not carry it.
    filter_shard=(bounds, index, exchange): these members are block ``index`` of an ensemble split at ``bounds`` whose
    other blocks run elsewhere, and the particle filter resamples the whole of it (include/hydrocol.h
    hc_set_filter_shard; ``exchange``: e.g. a ``multigpu.ShardExchange``).  member_offset must be ``bounds[index]``.
    Needs filter_stride; like enkf_shard it is set up by the run.
    """

    def __init__(self, cols, forcing, n_members, seed=0, device=0, member_offset=0, psi0=None, flags=None,
                 noise="philox", spinup="shared", enkf_shard=None, filter_shard=None, **options):
        """``options``: the run's options (settings.OPTIONS and MORE_OPTIONS; :class:`_Run` describes them), normalised and cross-checked
        before any handle exists."""
        s = settings.normalise("EnsembleSimulation", options, [cols], seed, noise=noise, member_offset=member_offset,
                               enkf_shard=enkf_shard, filter_shard=filter_shard)
        if enkf_shard is not None or filter_shard is not None:
            from . import _lib
            _lib.load(with_torch=True)             # torch before the library: the shard's buffer is a torch tensor
        self._start(cols, forcing, n_members, seed, device, member_offset, psi0, flags, noise, spinup)
        settings.start(self, s)


    def _start(self, cols, forcing, n_members, seed, device, member_offset, psi0, flags, noise, spinup):
        if noise not in ("philox", "numpy") or spinup not in ("shared", "member"):
            raise ValueError(f" {self.__class__.__name__}: unknown noise / spinup mode ({noise}, {spinup}).")
        self.cols, self.forcing = cols, forcing
        self.n_members = int(n_members)
        self.member_offset = int(member_offset)
        self.seed = int(seed)
        self.device = device
        self.noise = noise
        self.spinup_iters = None
        if noise == "numpy":
            self._init_numpy(psi0, flags, spinup)
            return
        if psi0 is None and spinup == "member":
            self.stepper = EnsembleStepper(cols, forcing, self.n_members, device=device, flags=flags)
            self.stepper.set_noise_philox(self.seed, self.member_offset)
            self.psi0, self.spinup_iters = spinup_members_on_gpu(self.stepper, cols, forcing)
            # the x0.8 damping a spin-up retry applied belongs to the spin-up vector, not to the run's base vector
            self.stepper.set_noise_philox(self.seed, self.member_offset)
            self.next_row, self.kernel_ms, self.launches = 1, 0.0, 0
            return
        if psi0 is None:
            # shared initial condition: spin-up with the noise vector of global member 0, draw 0
            probe = EnsembleStepper(cols, forcing, 1, device=device, flags=flags)
            probe.set_noise_philox(self.seed, 0)
            n_rnd = probe.philox_normals(0, PHILOX_DRAW_SPINUP)     # global member 0's spin-up vector
            probe.close()
            psi0, self.spinup_iters, _ = spinup_on_gpu(cols, forcing, n_rnd, device=device, flags=flags)
        self.psi0 = np.asarray(psi0, dtype=float)
        self.stepper = EnsembleStepper(cols, forcing, self.n_members, device=device, flags=flags)
        self.stepper.set_state(self.psi0)
        self.stepper.set_noise_philox(self.seed, self.member_offset)
        self.next_row = 1
        self.kernel_ms = 0.0
        self.launches = 0

    def _init_numpy(self, psi0, flags, spinup):
        cols, forcing, N, D = self.cols, self.forcing, self.n_members, self.cols.dim_d
        self.gens = member_generators(self.seed, N, self.member_offset)
        self.stepper = EnsembleStepper(cols, forcing, N, device=self.device, flags=flags)
        if psi0 is None:
            first = np.stack([g.standard_normal(D) for g in self.gens])           # draw #0 (simulation.py:426)
            if spinup == "member":
                self.stepper.set_noise_host(first)
                psi0, self.spinup_iters = spinup_members_on_gpu(self.stepper, cols, forcing)
            else:
                if self.member_offset == 0:
                    lead = first[0]
                else:       # every shard spins up with global member 0's first draw
                    lead = member_generators(self.seed, 1, 0)[0].standard_normal(D)
                psi0, self.spinup_iters, _ = spinup_on_gpu(cols, forcing, lead, device=self.device, flags=flags)
        self.psi0 = np.asarray(psi0, dtype=float)
        self.stepper.set_state(self.psi0)
        self.stepper.set_noise_host(np.stack([g.standard_normal(D) for g in self.gens]))   # draw #1 (:561)
        self.next_row, self.kernel_ms, self.launches = 1, 0.0, 0

    def advance(self, n_rows, **kw):
        """Solve the next ``n_rows`` forcing rows for every member."""
        if self.noise == "numpy":
            n_fresh = int(self.forcing.refresh[self.next_row:self.next_row + n_rows].sum())
            fresh = np.empty((n_fresh, self.n_members, self.cols.dim_d))
            for q in range(n_fresh):                 # row order, one vector per member per refresh row (:601)
                for k, g in enumerate(self.gens):
                    fresh[q, k] = g.standard_normal(self.cols.dim_d)
            kw["fresh_noise"] = fresh
        return super().advance(n_rows, **kw)

    def wtd_mean_std(self, moments=None):
        m = self.moments() if moments is None else moments
        return moments_to_mean_std(m, self.cols.dz, self.cols.z[0])

    # -- checkpoint / resume (the single-column analogue in the reference is IC_Filename, simulation.py:358-385) ------
    CHECKPOINT_KEYS = ("psi", "noise_scale", "moments", "next_row", "seed", "member_offset", "n_members", "dim_d",
                       "dim_t", "initial_cond")

    def dump(self, path):
        """Everything a stopped Philox ensemble is defined by, in the results container (HDF5 through libhdf5, ``.npz``
        where no libhdf5 loads): member states, per-member damping of the base noise vector, the moment table, the
        next forcing row and the stream keys, then what every option that is on adds (settings.SETTING_DATASETS, RUN_STATE
        and MEMBER_STATE, the tables of the two registries).  ``restore`` continues bit for bit."""
        if self.noise != "philox":
            raise ValueError(" EnsembleSimulation: dump/restore serves the Philox noise source "
                             "(a NumPy stream's position is not part of the stepper).")
        from pathlib import Path
        from . import hdf5io
        arrays = dict(psi=self.stepper.get_state(), noise_scale=self.stepper.noise_scale(),
                      moments=np.asarray(self.stepper.moments()), next_row=np.array(self.next_row, dtype=np.int64),
                      seed=np.array(self.seed, dtype=np.uint64), member_offset=np.array(self.member_offset, dtype=np.int64),
                      n_members=np.array(self.n_members, dtype=np.int64), dim_d=np.array(self.cols.dim_d, dtype=np.int64),
                      dim_t=np.array(self.forcing.dim_t, dtype=np.int64), initial_cond=np.asarray(self.psi0, dtype=float))
        # the options' settings, from which restore builds the run, and their live state; the tables follow, from the registries
        arrays.update(settings.checkpoint_datasets(self, self.stepper))
        # (the members' accumulators of the periods and the uptake are among them: a restore inside a period continues it)
        for key in self.diag_tables_on():
            arrays.update(diag_checkpoint(key, self.stepper.diag_raw(key), self.stepper.diag_counts()))
        for key in self.assim_tables_on():                # the filters' tables: one dataset each, <key>_table
            arrays[key + "_table"] = self.stepper.assim_table(key)
        path = Path(path)
        if hdf5io.available() and path.suffix != ".npz":
            hdf5io.write(path, arrays)
        else:
            path = path.with_suffix(".npz")
            np.savez(path, **arrays)
        return path

    @classmethod
    def restore(cls, path, cols, forcing, device=0, flags=None, enkf_soil_moisture=None, filter_soil_moisture=None):
        """A new ensemble (new handle) continuing the one ``dump`` wrote: same members, same streams, same row.  A run with
        a soil-moisture record needs it again (``enkf_soil_moisture`` or ``filter_soil_moisture``, like the forcing); its
        sensor table is restored."""
        from pathlib import Path
        from . import hdf5io
        path = Path(path)
        data = dict(np.load(path)) if path.suffix == ".npz" else hdf5io.read(path)
        missing = [k for k in cls.CHECKPOINT_KEYS if k not in data]
        if missing:
            raise ValueError(f" EnsembleSimulation: {path} is not an ensemble checkpoint (missing {missing}).")
        n, D, T = int(data["n_members"]), int(data["dim_d"]), int(data["dim_t"])
        if D != cols.dim_d or T != forcing.dim_t:
            raise ValueError(f" EnsembleSimulation: checkpoint of a [{D}]-node column over {T} rows does not fit "
                             f"this run ([{cols.dim_d}], {forcing.dim_t}).")
        psi = np.asarray(data["psi"], dtype=float).reshape(n, D)
        # the settings the constructor takes; which options it then has on says what is installed
        options = settings.checkpoint_keywords(data, path, enkf_soil_moisture=enkf_soil_moisture,
                                               filter_soil_moisture=filter_soil_moisture)
        sim = cls(cols, forcing, n, seed=int(data["seed"]), device=device, member_offset=int(data["member_offset"]),
                  psi0=np.asarray(data["initial_cond"], dtype=float).reshape(-1)[:D], flags=flags, **options)
        settings.install_state(settings.RUN_STATE, sim, data, path)
        sim.stepper.set_state(psi if n > 1 else psi[0])
        for key in sim.assim_tables_on():                 # the tables the constructor turned on, each from <key>_table
            sim.stepper.set_assim_table(key, np.asarray(data[key + "_table"], dtype=np.float64))
        settings.install_state(settings.MEMBER_STATE, sim, data, path)
        sim.stepper.set_moments(np.asarray(data["moments"], dtype=np.int64))
        for key in sim.diag_tables_on():                  # the diagnostics the constructor turned on, in the registry's order
            sim.stepper.set_diag_raw(key, diag_from_checkpoint(key, data))
        sim.next_row = int(data["next_row"])
        return sim


def allreduce_moments(moments, device, force=False):
    """Sum the int64 moment table ([3][T], or [P][3][T] for P parameter points) over all ranks -- the one collective
    of the path (RCCL over xGMI when the backend is nccl).

    Integer sums are exact and order-independent, so the ensemble mean / sigma are bitwise identical at any GPU
    count.  With the nccl backend the table is reduced in device memory (one host->device copy of the table the
    library handed over, ``all_reduce`` on the device tensor, one copy back).  No-op when torch.distributed is not
    initialised or the world has one rank, unless ``force`` asks for the collective anyway (a world-size-1 process
    group exercises the RCCL call path on a single GPU)."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return moments
    if dist.get_world_size() == 1 and not force:
        return moments
    t = torch.from_numpy(np.ascontiguousarray(moments))
    if dist.get_backend() == "nccl":
        t = t.to(device, non_blocking=False)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.cpu().numpy()


def allreduce_stepper_moments(stepper, device, force=False):
    """The run's one collective, on device memory end to end: the stepper's moment table ([3][T] or [P][3][T]) is copied
    device-to-device into a torch tensor (``hc_export_moments``), summed over the ranks with ``all_reduce`` (RCCL when
    the backend is nccl) and only then brought to the host.  Other backends (gloo rehearsals) and single-rank runs go
    through :func:`allreduce_moments` on the host copy."""
    import torch
    import torch.distributed as dist
    active = dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or force)
    if not active or dist.get_backend() != "nccl":
        return allreduce_moments(stepper.moments(), device, force=force)
    shape = (3, stepper.T) if stepper.P == 1 else (stepper.P, 3, stepper.T)
    t = torch.empty(shape, dtype=torch.int64, device=device)
    stepper.export_moments(t.data_ptr())
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.cpu().numpy()


def merge_parameters(params, override):
    """``params`` with the sections of ``override`` ({"Soil_Properties": {...}, ...}) merged in (a deep copy)."""
    import copy
    p = copy.deepcopy(params)
    for section, values in override.items():
        if isinstance(values, dict):
            p.setdefault(section, {}).update(values)
        else:
            p[section] = values
    return p


# What a parameter point may NOT change: the forcing digest (ET series, surface evaporation: simulation.py:273-352) is
# built once from the base parameters and shared by every point of a sweep, and the PREDICT gate is taken on the base.
SWEEP_SHARED_ENVIRONMENTAL = ("Atmospheric_Demand", "Wet_Season_pct", "Evaporation_pct")


def check_sweep_points(params, points):
    """Refuse parameter points that would silently run with the base point's forcing: an override of the
    ``Environmental`` keys the forcing digest reads, of ``Simulation_Flags.PREDICT`` (the repair gate is taken once, on
    the base), of the well or of the data file.  Returns the merged parameter dicts, one per point."""
    merged = [merge_parameters(params, ov) for ov in points]
    for k, mp in enumerate(merged):
        for key in SWEEP_SHARED_ENVIRONMENTAL:
            if mp["Environmental"].get(key) != params["Environmental"].get(key):
                raise ValueError(f" Sweep: point {k} overrides Environmental.{key}; every point of a sweep shares the base "
                                 f"forcing series (simulation.py:273-352) -- run such points as separate ensembles.")
        if bool(mp["Simulation_Flags"].get("PREDICT", False)) != bool(params["Simulation_Flags"].get("PREDICT", False)):
            raise ValueError(f" Sweep: point {k} overrides Simulation_Flags.PREDICT; the flag is taken from the base parameters.")
        for key in ("Well_No", "Site_Information", "Data_Filename"):
            if mp.get(key) != params.get(key):
                raise ValueError(f" Sweep: point {k} overrides {key}; every point shares the well and the forcing file.")
    return merged


class SweepSimulation(_Run):
    """BASELINE config 5: P parameter points x ``n_members`` stochastic members each, ALL in one handle and one
    launch per batch of rows (``hc_add_point``): per-member parameter point -> its own column parameters and slot
    tables in the step kernel, per-point moments.

    Global member ids are point-major over the WHOLE sweep: point k (global index ``first_point + j`` for the j-th
    point of this handle) owns members [k n, (k + 1) n) of the Philox stream, so a point's realisations do not depend
    on which rank or handle runs it.  Every point starts from its OWN spin-up (field capacity, wilting point and the
    equilibrium profile depend on the point: porosity.py:172-181, simulation.py:389-493): the P spin-ups run
    together in one ``hc_spinup`` launch (one member per point, that point's lead member's spin-up vector), and the
    result is broadcast to the point's members."""

    def __init__(self, cols_list, forcing, n_members, seed=0, device=0, first_point=0, flags=None, psi0=None,
                 point_ids=None, **options):
        """``options``: the run's options (settings.OPTIONS and MORE_OPTIONS; :class:`_Run` describes them), normalised and cross-checked
        before any handle exists."""
        self.points = list(cols_list)
        self.P, self.n = len(self.points), int(n_members)
        self._lead = (self.P,)
        s = settings.normalise("SweepSimulation", options, self.points, seed, lead=self._lead)
        self.forcing, self.seed, self.device = forcing, int(seed), device
        # global index of each of this handle's points in the whole sweep: consecutive from `first_point`, or any
        # list (`point_ids`) when points are dealt to ranks round-robin so that every rank gets the same mix of costs
        self.point_ids = (np.arange(self.P, dtype=np.int64) + int(first_point) if point_ids is None
                          else np.asarray(point_ids, dtype=np.int64))
        if self.point_ids.shape != (self.P,) or np.unique(self.point_ids).size != self.P or self.point_ids.min() < 0:
            raise ValueError(" SweepSimulation: point_ids must name each of the handle's points once.")
        self.bases = self.point_ids * self.n
        self.member_offset = int(self.bases[0])
        cols = self.points[0]
        self.cols = cols
        self.spinup_iters = None
        if psi0 is None:
            psi0, self.spinup_iters = self._spinup(flags)
        self.psi0 = np.asarray(psi0, dtype=float).reshape(self.P, cols.dim_d)
        self.stepper = EnsembleStepper(self.points, forcing, self.P * self.n, device=device, flags=flags)
        # a sweep always runs the generic-exponent cell model: a point that happens to sit on the default exponents
        # must not change its bits with the company it is stepped in
        self.stepper.set_generic_exponents(True)
        self.stepper.set_state(self.psi0 if self.P > 1 else self.psi0[0])
        self.stepper.set_noise_philox(self.seed, self.member_offset)
        if self.P > 1:
            self.stepper.set_point_member_bases(self.bases)
        settings.start(self, s)
        self.next_row, self.kernel_ms, self.launches = 1, 0.0, 0

    def _spinup(self, flags):
        cols, forcing, P, D = self.cols, self.forcing, self.P, self.cols.dim_d
        lead = EnsembleStepper(self.points, forcing, P, device=self.device, flags=flags)
        try:
            lead.set_generic_exponents(True)
            lead.set_noise_philox(self.seed, 0)
            noise = np.stack([lead.philox_normals(int(self.bases[j]), PHILOX_DRAW_SPINUP) for j in range(P)])
            start = np.stack([pressure_head(c, c.por_raw)[0] for c in self.points])
            lead.set_state(start if P > 1 else start[0])
            lead.set_noise_host(noise)
            iters, _ = lead.spinup(forcing.zwtd_cm[0], cols.z[0], forcing_row=0, max_iterations=1500)
            return lead.get_state(), iters
        finally:
            lead.close()


def deal_points(n_points, rank, world):
    """Global indices of the parameter points rank `rank` of `world` runs: round-robin."""
    return list(range(int(rank), int(n_points), int(world)))


def parameter_sweep(params, data, well, points, n_members, n_rows, seed=0, device=0, rank=0, world=1,
                    one_launch=True, rows_per_call=48 * 8):
    """BASELINE config 5: a grid of (n, a0, psi_sat, ...) points x ``n_members`` realisations each.

    ``points`` is a list of dicts ``{"Soil_Properties": {...}, "Hydraulic_Conductivity": {...}, ...}`` merged over
    ``params``; every point gets its own tables and its own spin-up.  Whole points are dealt to ranks round-robin
    (:func:`deal_points`: rank r owns points r, r + world, ... -- a grid's cost grows along its slowest axis, so
    contiguous blocks would hand one rank all the expensive points), with no communication; a point's members keep
    their global ids (point k owns members [k n, (k + 1) n) of the Philox stream) whoever runs it.  ``one_launch`` (default)
    steps all of a rank's points in one handle (:class:`SweepSimulation`); ``one_launch=False`` runs them one after
    another, one handle each -- same global member ids, bit-identical results, kept as the cross-check.
    Returns {point index: {"moments", "wtd_mean_cm", "wtd_std_cm", "psi0"}}.
    """
    from .digest import ColumnTables, ForcingDigest
    P = len(points)
    mine = deal_points(P, rank, world)
    if not mine:
        return {}
    merged = check_sweep_points(params, points)
    cols_all = [ColumnTables(merged[k], well) for k in mine]
    forcing = ForcingDigest(params, data, cols_all[0])
    groups = [(mine, cols_all)] if one_launch else [([k], [c]) for k, c in zip(mine, cols_all)]
    out = {}
    for ids, cols_list in groups:
        sim = SweepSimulation(cols_list, forcing, n_members, seed=seed, device=device, point_ids=ids)
        done = 0
        while done < n_rows:
            n = min(rows_per_call, n_rows - done)
            sim.advance(n)
            done += n
        m = sim.moments()
        for j, c in enumerate(cols_list):
            mean_cm, std_cm = moments_to_mean_std(m[j], c.dz, c.z[0])
            out[ids[j]] = {"moments": m[j], "wtd_mean_cm": mean_cm, "wtd_std_cm": std_cm, "psi0": sim.psi0[j],
                              "spinup_iterations": None if sim.spinup_iters is None else int(sim.spinup_iters[j]),
                              "kernel_ms": sim.kernel_ms}
        sim.close()
    return out
