/*
 * hydrocol.h -- C-ABI of libhydrocol.so: MI355X (gfx950) ensemble stepper for the
 * HydroModel 1-D stochastic Richards soil column.
 *
 * The reference (vrettasm/HydroModel) is pure Python and has no FFI; the boundary it
 * exposes for this path is two Python call signatures.  Each entry point below names
 * the reference interface it replaces (paths relative to /root/reference/code):
 *
 *   hc_set_column      <- objects built by Simulation.setupModel (src/simulation.py:100-231):
 *                         Porosity / TreeRoots / VrettasFung|vanGenuchten / SoilProperties ...
 *                         flattened to per-depth tables by hydromodel_amd/digest.py
 *   hc_set_forcing     <- per-row args_i dict (src/simulation.py:591-602): precipitation, atm,
 *                         time(hour), wtd; refresh rule `precip > 0.5 or i % 48 == 0` (:599)
 *   hc_set_state/get   <- y0 / y_i vectors (src/simulation.py:514,609,626)
 *   hc_set_noise_*     <- n_rnd vectors drawn at src/simulation.py:426,561,601
 *   hc_step_rows       <- the row loop body: RichardsPDE.solve(t_span, y0, args_i)
 *                         (src/richards_pde.py:478-537 -> scipy solve_ivp BDF) followed by
 *                         find_wtd(y_i >= psi_sat) (src/simulation.py:609-612)
 *   hc_spinup          <- Simulation.initial_conditions (src/simulation.py:389-493), per member
 *   hc_rhs             <- RichardsPDE.__call__(t, y, args)   (src/richards_pde.py:82-160)
 *   hc_model_nodes     <- h_model(y_i, z, args_i) diagnostics call (src/simulation.py:623;
 *                         src/models/vrettas_fung.py:51 / vanGenuchten.py:23)
 *   hc_get_moments     <- (new) per-row ensemble moments of wtd_est (src/simulation.py:612)
 *   hc_add_point       <- the per-parameter-point objects of Simulation.setupModel (src/simulation.py:146-231:
 *                         SoilProperties / WaterContent / HydraulicConductivity / Porosity -> field capacity,
 *                         wilting point src/porosity.py:172-181, iPsi_50 src/simulation.py:336-339), one set per
 *                         point of a parameter sweep, all points stepped by ONE launch
 *   hc_plugin_eval     <- HydrologicalModel subclasses called directly: VrettasFung.__call__(psi, z, {"n_rnd": ..})
 *                         (src/models/vrettas_fung.py:51-257), vanGenuchten.__call__ (src/models/vanGenuchten.py:23-126)
 *   hc_get/set_noise_scale <- the in-place damping `args["n_rnd"] *= 0.8` of a failed attempt (src/richards_pde.py:522) as
 *                         it accumulates on a member's base vector; with hc_get_state / hc_get_moments the restart state
 *                         of an ensemble (the reference restarts one column from IC_Filename, src/simulation.py:358-385)
 *   hc_set_point_member_bases <- which realisation a member is: the reference seeds one generator per run
 *                         (src/simulation.py:66-70); here member j of sweep point k draws stream base[k] + j
 *   hc_allreduce_moments, hc_get_point_costs <- (new) the ensemble's one collective; per-point cost for scheduling
 *   hc_set_profile_stats, hc_profile_snapshot, hc_get/set/export/reset_profile_stats*, hc_get_profile_overflow
 *                      <- Simulation.run's science output (src/simulation.py:658-671) as ensemble mean / sigma:
 *                         psi_press, theta_vol (and S_eff on the host), transpiration, lateral_flow, abs_error
 *   hc_set_wtd_hist, hc_get_wtd_hist, hc_set_wtd_hist_table, hc_reset_wtd_hist, hc_wtd_distribution
 *                      <- wtd_est / abs_error per row (src/simulation.py:612-615) as the ensemble's distribution:
 *                         per-row histograms of the water-table index, quantiles and the CRPS against the well
 *   hc_set_theta_hist, hc_get_theta_hist, hc_set_theta_hist_table, hc_reset_theta_hist, hc_get_theta_hist_outside,
 *   hc_get_theta_hist_bins
 *                      <- theta_vol (src/simulation.py:623) as the ensemble's distribution: per-node histograms of theta on
 *                         the profile rows, from which the host forms quantile bands of theta(z)
 *   hc_set_layer_storage, hc_get_layer_storage_words, hc_get_layer_storage, hc_set_layer_storage_tables,
 *   hc_export_layer_storage, hc_get_layer_storage_hist, hc_set_layer_storage_hist_table, hc_reset_layer_storage,
 *   hc_get_layer_storage_outside, hc_get_layer_storage_overflow, hc_get_layer_storage_layout
 *                      <- (new) dz * sum of theta_vol (src/simulation.py:623) over a depth layer, per member: the water a
 *                         root zone or the whole column stores, as the ensemble's mean, sigma and histogram on the profile rows
 *   hc_set_theta_cov, hc_get_theta_cov_layout, hc_get_theta_cov_words, hc_get_theta_cov, hc_set_theta_cov_tables,
 *   hc_export_theta_cov, hc_reset_theta_cov, hc_get_theta_cov_outside
 *                      <- (new) theta_vol (src/simulation.py:623) and wtd_est (:612) as the ensemble's second moments: the
 *                         covariance of theta at the selected nodes and the water table on the profile rows
 *   hc_set_period_totals, hc_get_period_totals_words, hc_get_period_totals, hc_set_period_totals_tables,
 *   hc_export_period_totals, hc_get/set/export_period_totals_hist(_table), hc_get/set_period_totals_acc,
 *   hc_reset_period_totals, hc_get_period_totals_outside/overflow/layout
 *                      <- (new) the "cumulative output" transpiration and lateral_flow (src/simulation.py:628-630) summed
 *                         per member over a period of rows, the period's water-table extremes and hydroperiod, as the
 *                         ensemble's mean, sigma and histograms
 *   hc_set_filter, hc_get/set_filter_stats, hc_get/set_filter_base, hc_get_filter_ancestors/weights/draw,
 *   hc_set_filter_soil_moisture, hc_get/set_filter_sm_stats, hc_get_filter_sm_width/member_weights/loglik/sm_theta
 *   hc_set_filter_tempering, hc_get/set_filter_temper_stats, hc_get_filter_temper_trials
 *   hc_set/get_filter_rejuvenation, hc_get/set_filter_rejuvenation_stats, hc_get_filter_rejuvenation_moments,
 *   hc_filter_rejuvenation_normals
 *                      <- (new) the ensemble conditioned on wtd_obs (src/simulation.py:582-612): a bootstrap particle filter,
 *                         and the log marginal likelihood of the well record per parameter point
 *   hc_set_filter_smoother, hc_get_filter_smoother_layout, hc_get_filter_smoother_hist, hc_set_filter_smoother_hist_table,
 *   hc_get/set_filter_smoother_paths, hc_get/set_filter_smoother_ring, hc_filter_smoother_flush, hc_reset_filter_smoother
 *                      <- (new) wtd_est (src/simulation.py:612) of earlier rows given the later record: the filter's
 *                         genealogy as a fixed-lag smoother, the one table that describes the posterior
 *   hc_set_enkf, hc_get/set_enkf_stats, hc_get_enkf_gain/y/eps
 *                      <- (new) the same conditioning by a stochastic ensemble Kalman filter on a continuous water table
 *   hc_set_enkf_soil_moisture, hc_get/set_enkf_sm_stats, hc_get_enkf_sm_width/y/gain/eps
 *                      <- (new) theta_vol (src/simulation.py:623) at sensor depths joins the well in the EnKF's analysis
 *   hc_set/get_enkf_method, hc_get_enkf_sqrt_gain/shift, hc_get_enkf_relaxation
 *                      <- (new) the EnKF's analysis scheme (perturbed observations or square root) and its relaxation to
 *                         prior spread
 *   hc_set/get_enkf_noise_field, hc_get/set_enkf_noise_stats, hc_get_enkf_noise_gain, hc_get_enkf_noise_sqrt_gain/shift,
 *   hc_get/set_enkf_noise_base
 *                      <- (new) args_i["n_rnd"], one base vector of D standard normals per column
 *                         (src/simulation.py:561,592; replaced for one row only on refresh rows, :599-601), is what
 *                         vrettas_fung.py:154-190 turns into K_bkg: a member's conductivity field.  The EnKF's analysis
 *                         updates it together with the member's psi (state augmentation)
 *   hc_set/get_enkf_forcing, hc_get/set_enkf_g_table, hc_get_enkf_g_gain, hc_get_enkf_g_sqrt_gain/shift
 *                      <- (new) the members' forcing-error state g (hc_set_forcing_perturbation) in the EnKF's analysis:
 *                         joint state and forcing-error estimation by state augmentation
 *   hc_set_enkf_window, hc_get/set_enkf_window_stats, hc_get/set_enkf_window_capture, hc_get_enkf_width,
 *   hc_get_enkf_window_width/y/eps/gain
 *                      <- (new) the well's record at rows inside the analysis window joins the analysis (asynchronous EnKF)
 *   hc_set/get_enkf_shard, hc_get_enkf_shard_words, hc_set/get_filter_shard, hc_get_filter_shard_words
 *                      <- (new) one point's members on several handles: the EnKF's analyses and the particle filter's
 *                         resampling are those of the one handle that holds every member
 *
 * Conventions: every function returns 0 on success or a negative hc_status; nothing throws
 * or aborts across the boundary; hc_last_error() gives the thread-local message.  Host
 * pointers are only read/written during the call.  The library owns all device memory.
 * State layout in HBM is member-major: psi[member][depth], fp64.  One handle drives one
 * device; a handle is not thread-safe; distinct handles are independent.
 */
#ifndef HYDROCOL_H
#define HYDROCOL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hc_handle hc_handle;

enum hc_status {
    HC_OK = 0,
    HC_ERR_ARG = -1,       /* bad argument / call order            */
    HC_ERR_DEVICE = -2,    /* HIP runtime error                    */
    HC_ERR_NO_DEVICE = -3, /* no gfx950 device visible             */
    HC_ERR_UNSUPPORTED = -4
};

#define HC_MODEL_VRETTAS_FUNG 0
#define HC_MODEL_VAN_GENUCHTEN 1
#define HC_MAX_DEPTH_NODES 640 /* 64 lanes x 10 cells; columns of 577..640 nodes whose parameter points all keep the root
                                  zone above node 320 run on two cooperating wavefronts per member (64 x 5 cells each),
                                  single points and sweeps alike; HYDROCOL_SPLIT_COLUMN in the environment at hc_create:
                                  0 keeps the one-wave kernels, 1 takes the two-wavefront kernel from 513 nodes on */

/* One soil column geometry + parameter point (static during a run). */
typedef struct {
    int32_t dim_d;        /* D depth nodes (z_grid.size)                              */
    int32_t model;        /* HC_MODEL_*                                               */
    int32_t flag_et;      /* Simulation_Flags.ET                                      */
    int32_t flag_lf;      /* Simulation_Flags.LF  (monitoring mode)                   */
    int32_t flag_hlift;   /* Simulation_Flags.HLIFT                                   */
    int32_t n_root_first; /* root-zone cells of the first-midpoint call (0 or 1)      */
    int32_t n_root_int;   /* root-zone cells of the interior call                     */
    int32_t n_groups;     /* FD-Jacobian column groups                                */
    double theta_res, alpha, n, m, psi_sat, epsilon, lambda_exp, sigma_noise, sat_soil, dz;
    double ipsi50, lai, surface_evap, interception, evap_delta_min;
    /* Repaired PREDICT mode (src/richards_pde.py:312-351) -- an EXTENSION with no reference oracle: the reference
     * raises TypeError at :327-330 (np.linspace with a float count).  Semantics here: low_lim = dim_d - (sat_cells - 1)
     * of each pde_fun call as an integer, no cell drains when it is <= 0; needs the wet-season bit in `daylight`. */
    int32_t flag_predict; /* Simulation_Flags.PREDICT (lateral flow in predictive mode, needs flag_lf)   */
    int32_t sat_cells;    /* ceil(sat_depth / dz), src/simulation.py:128                                  */
} hc_column_params;

/* node_tabs: [3][D] rows = porosity, mean-K, noise coefficient (-1 = no layer) at the nodes
 * mid_tabs : [6][D-1] rows = porosity, field capacity, wilting point, root pdf, mean-K,
 *            noise coefficient at the midpoints
 * groups   : [D] column group of every state entry (scipy group_columns for a tridiagonal) */
int hc_create(int device_ordinal, hc_handle **out);
int hc_destroy(hc_handle *h);
const char *hc_last_error(void);
const char *hc_version(void);   /* "hydrocol <v> (gfx950) kernels <hash>": <hash> identifies the device code (kernel
                                      sources + compile flags + compiler) -- the key of profiles/pmc_constants.json */

int hc_set_column(hc_handle *h, const hc_column_params *p, const double *node_tabs,
                  const double *mid_tabs, const int32_t *groups);
/* Parameter points (BASELINE config 5).  hc_set_column installs point 0 and the geometry (dim_d, groups, dz) and
 * drops any further points; hc_add_point appends one more point with tables of its own (same dim_d, n_groups, dz).
 * With P points the n_members of hc_set_members must be a multiple of P and are point-major: point k owns members
 * [k * n_members / P, (k + 1) * n_members / P).  One hc_step_rows / hc_spinup launch advances every point; each
 * member sees the column parameters and tables of its own point; moments are kept per point.  Adding a point changes
 * the shape of the moment table ([n_points][3][T]): whatever was accumulated before is dropped (the table is re-created,
 * zeroed, by the next call that needs it) -- install all points before the first hc_step_rows. */
int hc_add_point(hc_handle *h, const hc_column_params *p, const double *node_tabs, const double *mid_tabs);
int hc_get_point_count(hc_handle *h); /* >= 1 once hc_set_column has run; negative on error */
/* The cell model comes in two builds: one specialised for the reference's default exponents (vrettas_fung, n = 2,
 * m = 1/2, lambda = 1: every pow() folds into rsqrt / multiplies) and a generic one (powers as exp(y log x)); a handle
 * takes the first only when EVERY point qualifies.  The two agree to ~1e-15 relative per call, not bit for bit.
 * on != 0 pins the generic build, so that a default-exponent point gives the same bits whether it is stepped alone or
 * inside a sweep of other points. */
int hc_set_generic_exponents(hc_handle *h, int32_t on);

/* Forcing struct-of-arrays, n_rows entries each; wtd_obs < 0 marks a row to skip
 * (src/simulation.py:582-588): such a row is not solved and consumes NO noise draw (its refresh flag is ignored,
 * host-noise callers must not supply a vector for it).  The library numbers the draws itself: refresh row k
 * (1-based, skipped rows not counted) uses draw k; 0 = base vector.
 * daylight: bit 0 = daylight (6 <= hour <= 17, src/richards_pde.py:230); bit 1 = wet season, month in
 * {10,11,12,1,2,3} (src/richards_pde.py:315) -- read only in PREDICT mode. */
int hc_set_forcing(hc_handle *h, int64_t n_rows, const double *precip, const double *atm,
                   const uint8_t *daylight, const int32_t *wtd_obs, const uint8_t *refresh);

/* One row of the forcing replaced in place (row < n_rows of hc_set_forcing; its refresh flag is cleared): what the
 * row-by-row caller of src/simulation.py:590-609 knows only when it reaches the row -- args_i["wtd"], ["atm"],
 * ["time"], ["precipitation"] -- handed over just before `pde_model.solve(t_span, y0, args_i)` (hydromodel_amd/pde.py). */
int hc_set_forcing_row(hc_handle *h, int64_t row, double precip, double atm, uint8_t daylight, int32_t wtd_obs);

int hc_set_members(hc_handle *h, int64_t n_members);
/* psi: [n_members][D] (broadcast 0), [D] copied to every member (1), or [n_points][D] copied to the members of
 * each parameter point (2) */
int hc_set_state(hc_handle *h, const double *psi, int broadcast);
int hc_get_state(hc_handle *h, double *psi, int64_t first_member, int64_t count);

/* Noise source A (parity): host-supplied base vectors [n_members][D]; refresh-row vectors are
 * passed to hc_step_rows.  Mutated in place by the x0.8 retry rule (src/richards_pde.py:522). */
int hc_set_noise_host(hc_handle *h, const double *base);
int hc_get_noise_base(hc_handle *h, double *base, int64_t first_member, int64_t count);
/* Noise source B (throughput): counter-based Philox4x32-10 + Box-Muller generated in-kernel;
 * stream = (seed, member_offset + member, draw index, depth).  The retry damping is kept as a
 * per-member scale factor. */
int hc_set_noise_philox(hc_handle *h, uint64_t seed, int64_t member_offset);
/* draw indices: 0 = base vector, k >= 1 = k-th refresh row, HC_PHILOX_DRAW_SPINUP = the vector spin-up solves use
 * (the reference draws spin-up, base, refresh... in that order: src/simulation.py:426,561,601) */
#define HC_PHILOX_DRAW_SPINUP 0xFFFFFFFFll
/* What the Philox source yields for (member, draw): out[D] (test hook). */
int hc_philox_normals(hc_handle *h, int64_t member, int64_t draw, double *out);

/* Correlated noise fields: a vertical correlation of the Philox source's vectors.
 * For a member and a draw, xi [D] is what hc_philox_normals returns.  Two coefficient vectors a [D] and b [D] per
 * parameter point define the field z [D], in fp64 with contraction off (one product, one product, one sum):
 *     z_0 = xi_0
 *     z_i = xi_i                               where a_i == 0  (a break: the recursion restarts; a copy, no arithmetic)
 *     z_i = (a_i * z_{i-1}) + (b_i * xi_i)     otherwise
 * sequentially down the column, so the bits are defined by the tables alone (stepper.noise_correlate restates it in
 * NumPy).  With a_i = rho = exp(-dz / l) and b_i = sqrt(1 - rho rho) this is the exact Cholesky factor of the exponential
 * covariance exp(-|z_i - z_j| / l): every node's variance is 1, so sigma_noise and the noise coefficients keep their
 * meaning; a break makes the two sides independent (a layer interface).
 *   The base vector is z of draw 0 times the member's damping scale (one rounding, as the filter's fill), a refresh row's
 *   vector is z of that row's draw index, spin-up vectors stay white.  The handle fills these vectors itself
 *   (noise_field_fill_kernel: Philox, recursion and store in one pass) and runs the step kernel's caller-noise path, as
 *   with the particle filter in a Philox run: the x0.8 damping mutates the base vector in place; the particle filter
 *   copies it with psi; the EnKF's noise field analyses it like any other.  A launch stages at most 4 GiB of refresh
 *   vectors.  Not modelled: correlation in time between a refresh vector and the base, a correlated rejuvenation jitter,
 *   correlated spin-up vectors, other covariances, host-noise runs (such a caller shapes its own vectors).
 * hc_set_noise_correlation: tables [n_points][D]; a == NULL turns it off (the in-kernel source again; the damping the
 *   base vectors took meanwhile is not carried into the scales; under a filter or the noise field their base stays and
 *   the refresh vectors are white again).  Needs a Philox run (hc_set_noise_philox first, and the
 *   column, forcing, members and state in place).  HC_ERR_ARG for host noise, a non-finite entry, a_i outside [0, 1),
 *   b_i <= 0, a_0 != 0, |a_i^2 + b_i^2 - 1| > 1e-12 where a_i != 0, b_i != 1 where a_i == 0, or the particle filter or the
 *   EnKF's noise field already on (their base vectors carry history: set the correlation first); a refused call leaves
 *   the correlation off.  On success base
 *   [N][D] is allocated and filled with the correlated draw 0 times the current scales; hc_set_filter and
 *   hc_set_enkf_noise_field called afterwards keep that base instead of refilling it.  While it is on, hc_spinup,
 *   spin-up solves of hc_step_rows and hc_set_noise_scale are refused: set the correlation after the spin-up.  Turned off
 *   by whatever resets the noise source: hc_set_noise_philox, hc_set_noise_host, hc_set_members, hc_set_column /
 *   hc_add_point, hc_set_point_member_bases.  With nothing set, nothing is launched or allocated.
 * hc_get_noise_correlation: on, and the tables when on (a, b may be NULL).
 * hc_noise_field_normals: what the source now yields for (member, draw), unscaled (test hook; member is the stream's
 *   key as in hc_philox_normals, and with several points the table is that of the point whose keys hold it).  With the
 *   correlation off it is hc_philox_normals.
 * hc_get/set_noise_field_base: the base vectors [N][D] (a checkpoint) while a correlation is on in a Philox run; with a
 *   filter or the noise field on their own accessors read and write the same vectors. */
int hc_set_noise_correlation(hc_handle *h, const double *a, const double *b);
int hc_get_noise_correlation(hc_handle *h, int32_t *on, double *a, double *b);
int hc_noise_field_normals(hc_handle *h, int64_t member, int64_t draw, double *out);
int hc_get_noise_field_base(hc_handle *h, double *base, int64_t first_member, int64_t count);
int hc_set_noise_field_base(hc_handle *h, const double *base);

/* Perturbed forcing: a multiplicative log-normal error per member on the two forcing streams, s = 0 precipitation and
 * s = 1 atmospheric demand, with memory in time.
 *   The day of forcing row i is k = i / 48 (integer division: the model's own daily clock, the one the noise refresh
 *   runs on).  xi_{m,k,s} is the standard normal of ONE Philox4x32-10 block keyed by `seed` at the counter
 *   (word_s, k, gid_lo, gid_hi), word_0 = HC_FORCING_WORD_PRECIP, word_1 = HC_FORCING_WORD_DEMAND, taken from the cosine
 *   branch of the Box-Muller step as the EnKF's draws are.  (First counter words in use: the noise streams depth / 2
 *   < 2^31, the rejuvenation jitter 0x80000000 | depth / 2, the EnKF 0xFFFFFFF0 + i and 0xFFFFFFFE, the particle filter
 *   0xFFFFFFFF: the streams never meet.)  gid is the member's global id, the one its noise stream is keyed by:
 *   member_offset + m, or with several points point_base[k] + j.  A host-noise run has no such stream: its ids are
 *   0 + m unless hc_set_forcing_member_offset gives the first member's id (the shards of one host-noise ensemble).
 *   In fp64 with contraction off, one product, one product, one sum, in this order:
 *       g_{m,0,s} = xi_{m,0,s}
 *       g_{m,k,s} = (phi * g_{m,k-1,s}) + (c * xi_{m,k,s})          an AR(1) of unit variance
 *       f_{m,k,s} = exp((sigma_s * g_{m,k,s}) - h_s)                 a log-normal of mean one; exactly 1.0 where sigma_s == 0
 *   with phi = exp(-1 / tau) and c = sqrt(1 - phi phi) formed by the caller (tau = 0: phi = 0, c = 1, g = xi) and
 *   h_s = sigma_s sigma_s / 2 formed on the host (stepper.forcing_recursion_of restates g in NumPy, bit for bit given xi).
 *   On a solved row i of member m that is no spin-up solve the step kernel integrates with precip_i * f_{m,k,0} and
 *   atm_i * f_{m,k,1}, one IEEE product each, and nothing else changes: the refresh rule (precip > 0.5) and the draw
 *   indices, surface_evap, daylight / wet, wtd_obs, spin-up solves, hc_rhs, hc_rhs_ex and the Python RHS stay with the
 *   record.  A member is therefore, bit for bit, a run on its own scaled record with the ensemble's refresh flags.
 *   Before each launch the handle fills the factors of the days the launch touches (forcing_factor_fill_kernel: Philox,
 *   recursion, exp and a coalesced store in one pass) and advances the carried state g [2][N] and the day it stands at
 *   (into a second buffer that replaces the first once the step launch is issued: a launch that fails before that leaves
 *   the state where it stood, and the same rows can be stepped again);
 *   a launch that starts inside that day reuses its g, so nothing depends on where launch boundaries fall.  Rows must
 *   not go back behind the day the state stands at (HC_ERR_ARG; hc_set_forcing_state or a new
 *   hc_set_forcing_perturbation rewinds).  After a particle filter's resampling g travels with the member (a latent state
 *   of its trajectory; the refresh draws stay with the slot); the EnKF leaves g alone unless hc_set_enkf_forcing has it
 *   analysed with the member's state (below: the analysed g is what the rest of the day and, through the recursion, every
 *   later day integrate with).  While it is on, the step kernel
 *   is the build that carries the predictive lateral-flow branch (a monitoring-mode point keeps its semantics through
 *   flag_predict, as in a mixed sweep); with nothing set nothing is launched or allocated and the build is the one it was.
 *   Not modelled: g in a sharded EnKF analysis (refused) or in a smoother, a per-member refresh rule, additive or gamma
 *   errors, correlation between the two streams, the sharded particle filter (refused).
 * hc_set_forcing_perturbation: needs the column, forcing, members and state in place.  HC_ERR_ARG for a non-finite value,
 *   sigma outside [0, 1], phi outside [0, 1), c <= 0, |phi^2 + c^2 - 1| > 1e-12, or a sharded particle filter.  Both sigma = 0
 *   is allowed: the factors are 1.0 and the wider build runs.  The state starts empty (day -1).  Turned off by
 *   hc_set_forcing, hc_set_members, hc_set_column / hc_add_point, hc_set_point_member_bases and hc_clear_forcing_perturbation.
 * hc_set_forcing_member_offset: the global id of the handle's first member for this feature alone, in place of the noise
 *   source's (no other stream reads it).  Needs the feature on, one parameter point, and no row stepped yet (HC_ERR_ARG);
 *   a new hc_set_forcing_perturbation forgets it.
 * hc_get_forcing_perturbation: on, and the parameters when on (each pointer may be NULL).
 * hc_get/set_forcing_state: g [2][N] and the day it stands at (-1: no row stepped yet, g is not read): a checkpoint.
 * hc_forcing_normals: the raw xi of the stream key `member` (a global id), out[n_days][2] (test hook).
 * hc_forcing_factors: f of the handle's slots first_member ... + count over the days first_day ... + n_days by the
 *   stateless recursion from day 0 on the same device code, out[n_days][2][count]; what the step kernel applies to slots
 *   that neither a resampling nor an analysis (hc_set_enkf_forcing) has touched. */
#define HC_FORCING_WORD_PRECIP 0xFFFFFFE0u
#define HC_FORCING_WORD_DEMAND 0xFFFFFFE1u
#define HC_FORCING_DAY_ROWS 48
int hc_set_forcing_perturbation(hc_handle *h, double sigma_precip, double sigma_demand, double phi, double c, uint64_t seed);
int hc_clear_forcing_perturbation(hc_handle *h);
int hc_set_forcing_member_offset(hc_handle *h, int64_t member_offset);
int hc_get_forcing_perturbation(hc_handle *h, int32_t *on, double *sigma_precip, double *sigma_demand, double *phi, double *c,
                                uint64_t *seed);
int hc_get_forcing_state(hc_handle *h, double *g, int64_t *day);
int hc_set_forcing_state(hc_handle *h, const double *g, int64_t day);
int hc_forcing_normals(hc_handle *h, int64_t member, int64_t first_day, int64_t n_days, double *out);
int hc_forcing_factors(hc_handle *h, int64_t first_member, int64_t count, int64_t first_day, int64_t n_days, double *out);

typedef struct {
    int64_t row_begin;      /* first row to solve (row i integrates t in [i-1, i]); >= 1      */
    int64_t n_rows;
    int32_t spinup;         /* 1: SPINUP semantics (src/simulation.py:398): row_begin is used as
                               the forcing row for every solve, t_span = (0,1), noise never refreshed */
    int32_t accumulate_moments; /* add (count, sum idx, sum idx^2) of wtd_est per row          */
    const double *fresh_noise;  /* host-noise mode: [n_refresh_rows_in_range][n_members][D]    */
    int32_t *wtd_out;       /* nullable: [n_rows][n_members] wtd_est index per row             */
    int32_t *stats_out;     /* nullable: [n_rows][n_members][6] nfev,njev,nlu,nsteps,attempts, then
                               (refresh flag) | (failed attempts of the row << 8): each failed attempt scaled the
                               row's noise vector by 0.8 (src/richards_pde.py:522)                      */
    double *psi_rows_out;   /* nullable: [n_rows][n_members][D] state after every row          */
    double *diag_out;       /* nullable: [n_rows][n_members][2] = transpiration, lateral_flow as
                               pde_model.arg_out holds them after the row's solve
                               (src/richards_pde.py:380-391, src/simulation.py:629-630)        */
    double kernel_ms;       /* out: device time of the launch(es), HIP events on the stream    */
    int64_t launches;       /* out */
} hc_step_args;

int hc_step_rows(hc_handle *h, hc_step_args *a);

/* Simulation.initial_conditions (src/simulation.py:389-493) for every member in ONE launch: each member
 * repeats the solve of `forcing_row` over t in (0, 1) with SPINUP semantics and its own fixed noise vector,
 * starting from the state set by hc_set_state, until its own stop rule holds (src/simulation.py:468:
 * |zwtd_cm - z[wtd_est]| <= 2 dz and mean((y_j - y_{j-1})^2) <= 0.01) or max_iterations solves are done.
 * The members' states are left in place (hc_get_state). */
typedef struct {
    int64_t forcing_row;      /* 0 in the reference                                                */
    int32_t max_iterations;   /* burn_in = 1500 in the reference (src/simulation.py:420)           */
    double zwtd_cm;           /* first water-table observation, cm                                 */
    double z0_cm;             /* depth of node 0: z[i] = z0_cm + i * dz                            */
    int32_t *iterations_out;  /* [n_members] solves used; negative = stopped by max_iterations     */
    double kernel_ms;         /* out */
} hc_spinup_args;
int hc_spinup(hc_handle *h, hc_spinup_args *a);
int hc_synchronize(hc_handle *h);
/* event counters since hc_create: [0] FD-Jacobian passes that took num_jac's "difference too small ->
 * retry with a 10x step" branch, [1] failed BDF attempts (each scales the noise by 0.8), [2] attempts abandoned
 * by the kernel's iteration budget (default 20 000 trips of the phase loop, ~14x the costliest regular attempt seen;
 * a semantic deviation -- SciPy's BDF has no such cap -- handled like a solve that gave up, DESIGN.md "Iteration
 * budget"; with HYDROCOL_STRICT_GUARD=1 in the environment hc_step_rows / hc_spinup fail instead), [3] where the
 * last of those happened: global member id << 24 | forcing row.
 * Test hooks read from the environment at hc_create: HYDROCOL_DEBUG_MAX_ITER (same as hc_set_iteration_budget),
 * HYDROCOL_DEBUG_JAC_REJECT (raises num_jac's retry threshold), HYDROCOL_ROWS_PER_LAUNCH, HYDROCOL_CHUNK_MEMBERS
 * (members per scheduling chunk when several parameter points share a launch), HYDROCOL_COV_CHUNK_MEMBERS (members per
 * chunk of the theta covariance's staging, hc_set_theta_cov), HYDROCOL_DEBUG_CUS (a persistent grid of fewer workgroups
 * than the device has compute units: measurements only). */
int hc_get_counters(hc_handle *h, uint64_t *out4);
/* Rows one kernel launch of hc_step_rows covers; hc_step_rows splits longer requests.  Default (and rows = 0): with the
 * in-kernel noise 48 = one simulated day for ensembles of >= 1 048 576 members, proportionally more for smaller ones
 * (48 x 1 048 576 / members, at most a year; round 5: 65 536 before -- 4 096 members +5 %, 16 384 +2 %, 65 536 +3 %); with
 * the caller's noise (every refreshed row of a launch stages members x D doubles) 48 x 65 536 / members.
 * A member's rows of a launch are solved back to back by one wavefront with psi resident in LDS, and a launch ends when
 * its slowest wavefront does.  Large ensembles (>> 1 024 wavefronts' worth of members) balance within a day; a SMALL
 * ensemble (a few members per wavefront, e.g. 4 096) loses ~15 % to that tail per launch and is better served by long
 * launches (a year: the members' total costs are nearly equal).  Per-row device buffers grow with it
 * (2 B x rows x members for the water-table indices). Results do not depend on it. */
int hc_set_rows_per_launch(hc_handle *h, int32_t rows);
/* Budget of one BDF attempt in trips of the kernel's phase loop (>= 1). */
int hc_set_iteration_budget(hc_handle *h, int32_t phase_steps);
/* The integrator is SciPy's (third-party to the reference; /root/reference/requirements.txt:4 pins scipy==1.5.2, the pinning
 * vectors were made with 1.15.3).  On this path the two differ in ONE place: common.py select_initial_step clamps h0 and
 * the step it returns to the integration interval since scipy 1.9.  Default (0): the >= 1.9 form; on != 0: the 1.5.2 form
 * (also HYDROCOL_SCIPY_152=1 in the environment at hc_create).  How often the clamps bind and what that moves:
 * profiles/r05_scipy152_clamp.txt. */
int hc_set_scipy_152(hc_handle *h, int32_t on);

/* moments: [n_points][3][n_forcing_rows] int64 = count, sum(idx), sum(idx^2) of wtd_est over the members of each
 * parameter point ([3][n_forcing_rows] for the usual single point); not available for spin-up solves */
int hc_get_moments(hc_handle *h, int64_t *moments);
/* The same table copied device-to-device into caller-owned memory on the handle's device (n_points * 3 * n_rows
 * int64): the buffer a collective (RCCL all-reduce over the ranks' tables) works on, without a host round trip.
 * Complete when the call returns. */
int hc_export_moments(hc_handle *h, void *device_dst);
int hc_set_moments(hc_handle *h, const int64_t *moments);
int hc_reset_moments(hc_handle *h);

/* Ensemble profile statistics: what Simulation.run returns for one column (src/simulation.py:658-671) as the mean and
 * population sigma over the members of each parameter point, reduced on the device.
 *   profile rows r % stride == 0 (r < n_forcing_rows): psi_press = the state after the row's solve (psi[i], :615) and
 *     theta_vol = theta of that state at the nodes (h_model, :620; bit for bit hc_model_nodes' out[0]); row 0 is the state
 *     before any solve (psi[0], theta_vol[0]) and comes from hc_profile_snapshot on the current states;
 *   every solved row: transpiration, lateral_flow (pde_model.arg_out after the row's solve, :629-630; the values
 *     hc_step_args.diag_out returns) and sum |obs_idx - wtd_idx| (abs_error = dz * that sum / count, :612).
 * Skipped rows (wtd_obs < 0) count no members; spin-up solves accumulate nothing.
 * Integer sums only: x is quantised to q = rint(x * 2^s), s = HC_PROF_SCALE_* below, |q| <= HC_PROF_Q_MAX (a value outside is
 * clamped and counted in the overflow slot); each member adds q to word 0 and the four 20-bit limbs of q^2 (< 2^80),
 * (q^2 >> 20k) & (2^20 - 1), to words 1 + k.  Five int64 words per (row, node, quantity): sums over ranks / handles are
 * plain int64 sums (exact, order-independent); the host forms n sum q^2 - (sum q)^2 exactly before any rounding.
 * Table (int64, n_prow = (n_forcing_rows - 1) / stride + 1, P points, T forcing rows, D nodes), in this order:
 *   prof [P][n_prow][D][2][5]   quantity 0 = psi_press, 1 = theta_vol
 *   pcnt [P][n_prow]            members counted in each profile row
 *   flux [P][T][2][5]           quantity 0 = transpiration, 1 = lateral_flow
 *   fcnt [P][T]                 members counted in each solved row
 *   aerr [P][T]                 sum |obs_idx - wtd_idx|
 *   ovf  [1]                    values clamped by the quantisation (summed like the rest)
 * hc_step_rows with statistics on stages the two fluxes of every row ([rows][N][2] doubles, at most 1 GiB) on the device.
 * When the stride is at least the number of rows whose states fit in about 4 GiB ([rows][N][D] doubles), a launch ends on
 * each profile row and that row is reduced from the members' current states; shorter strides stage the states of every
 * row of a launch (as psi_rows_out does) and the launches are shortened to fit.  The step kernels are the same either way
 * and results do not depend on launch length.
 * hc_set_profile_stats: stride 0 = off (default); otherwise (re)creates the table zeroed.  Like the moment table it is
 * re-created, zeroed, when the points, the forcing rows or the depth change.  get / set / export take the table's size in
 * words (hc_get_profile_stats_words) and fail on any other. */
#define HC_PROF_WORDS 5
#define HC_PROF_SCALE_PSI 16        /* psi [cm]: 2^-16 cm steps, |psi| < 2^24 cm                                   */
#define HC_PROF_SCALE_THETA 40      /* theta in [0, 1]: 2^-40 steps                                                */
#define HC_PROF_SCALE_FLUX 32       /* transpiration, lateral flow [cm per row]: 2^-32 steps, |x| < 2^8             */
#define HC_PROF_Q_MAX ((1LL << 40) - 1)
int hc_set_profile_stats(hc_handle *h, int32_t stride);
int hc_get_profile_stats_words(hc_handle *h, int64_t *n_words);
/* accumulates every member's current state as profile row `row` (row % stride == 0), counting all members */
int hc_profile_snapshot(hc_handle *h, int64_t row);
int hc_get_profile_stats(hc_handle *h, int64_t *table, int64_t n_words);
int hc_set_profile_stats_tables(hc_handle *h, const int64_t *table, int64_t n_words);   /* checkpoint / resume */
/* device-to-device into caller-owned memory on the handle's device (the buffer of a collective); complete on return */
int hc_export_profile_stats(hc_handle *h, void *device_dst, int64_t n_words);
int hc_reset_profile_stats(hc_handle *h);
int hc_get_profile_overflow(hc_handle *h, uint64_t *count);   /* the ovf slot */

/* Ensemble water-table distribution: the reference's wtd_est = find_wtd(...) and abs_error = |zWtd_cm - z[wtd_est]| of one
 * column (src/simulation.py:612-615) over the members of each parameter point, as exact integer histograms.
 *   histogram rows r % stride == 0 (r < n_forcing_rows), n_hrow = (n_forcing_rows - 1) / stride + 1, slot j <-> row j stride
 *   (the profile rows of hc_set_profile_stats).  Row 0 is the initial state: no water table is computed for it, its
 *   histogram stays empty.  Skipped rows (wtd_obs < 0) count no members; spin-up solves accumulate nothing.
 *   hist [P][n_hrow][D] int32: hist[p][j][b] = members of point p whose water-table index after row j stride's solve is b
 *   (the index moments_kernel sums, hc_step_args.wtd_out).  Integer adds only: the table does not depend on launch length,
 *   member split, point order or the number of handles / ranks summed.
 * hc_set_wtd_hist: stride 0 = off (default); otherwise (re)creates the table zeroed.  Like the moment table it is re-created,
 * zeroed, when the points, the forcing rows or the depth change.  HC_ERR_ARG for a table of more than HC_WTD_HIST_MAX_ENTRIES
 * entries or a point of more than 2^31 - 1 members (a count must fit its int32 bin).  get / set take the table's size in
 * entries (P n_hrow D) and fail on any other.  The step kernels are the same with the table on or off.
 *
 * hc_wtd_distribution: the summary of n_rows histograms of D bins (hist [n_rows][D], e.g. a [P][n_hrow][D] table summed over
 * ranks, flattened) against obs_idx [n_rows], on `device`, for the caller's table (no handle: the points of a sweep
 * assembled over ranks belong to no single handle).  Per row, with c_b the cumulative count and n = c_{D-1}:
 *   count[r] = n;
 *   quantile_idx[r][l] = the smallest b with c_b >= k, k = max(1, ceil(n levels[l])) in fp64: numpy.quantile(idx, q,
 *     method="inverted_cdf") of the members' indices; -1 when n = 0;
 *   crps_cm[r] = dz S / n^2, S = sum_{b=0}^{D-2} (c_b - n [b >= obs_idx[r]])^2: the CRPS of the ensemble's empirical CDF on the
 *     grid against the observation, integral (F(x) - 1{x >= z_obs})^2 dx; for n = 1 exactly the reference's abs_error.  S is
 *     an exact 128-bit integer; S / n^2 is formed in double-double and rounded once (within 1 ulp of dz S / n^2).  NaN when
 *     n = 0 or obs_idx[r] is outside [0, D).
 * Levels in [0, 1], at most HC_WTD_MAX_LEVELS of them; n_rows D <= HC_WTD_HIST_MAX_ENTRIES.  Host pointers in and out;
 * complete on return. */
#define HC_WTD_MAX_LEVELS 16
#define HC_WTD_HIST_MAX_ENTRIES (1LL << 30)      /* 4 GiB of int32 bins */
int hc_set_wtd_hist(hc_handle *h, int32_t stride);
int hc_get_wtd_hist(hc_handle *h, int32_t *table, int64_t n_entries);
int hc_set_wtd_hist_table(hc_handle *h, const int32_t *table, int64_t n_entries);   /* checkpoint / resume, rank sums */
int hc_reset_wtd_hist(hc_handle *h);
int hc_wtd_distribution(int device, const int32_t *hist, const int32_t *obs_idx, int64_t n_rows, int32_t D,
                        const double *levels, int32_t n_levels, double dz, int64_t *count, int32_t *quantile_idx,
                        double *crps_cm);

/* Ensemble soil-moisture distribution: theta_vol of the profile rows (hc_set_profile_stats, which must be on) as exact
 * integer histograms per node.  theta above the water table is a saturating function of psi and the members pile up at the
 * porosity below it, so a mean +- sigma band can leave [theta_res, porosity]; the histogram makes no such assumption.
 *   rows: the profile rows, at the profile stride (slot j <-> row j stride, n_prow slots); row 0 is counted by
 *   hc_profile_snapshot, the others by hc_step_rows from the states the profile statistics read.  Skipped rows (wtd_obs < 0)
 *   count no members; spin-up solves accumulate nothing.
 *   bins: B = 32, 64 or 128.  theta is the cell model's theta_vol of the member's psi at the node, with no noise term: the
 *   value the profile statistics quantise and hc_model_nodes returns, bit for bit.  A member adds one to bin
 *   b = floor(theta B) of its node (theta B is exact in fp64: the bin depends on theta's bits alone); theta == 1.0 goes to
 *   bin B - 1; a theta that is NaN, below 0 or above 1 goes to no bin and adds one to the `outside` count.
 *   table (int32): hist [P][n_prow][D][B], then the outside count as one uint64 in two more entries (low word first):
 *   P n_prow D B + 2 entries.  Integer adds only: the table does not depend on launch length, member split, point order or
 *   the number of handles / ranks summed.
 * hc_set_theta_hist: n_bins 0 = off (default); 32, 64 or 128 (re)creates the table zeroed.  HC_ERR_ARG (and off) when the
 * profile statistics are off, for any other bin count, for a table of more than HC_WTD_HIST_MAX_ENTRIES bins or a point of
 * more than 2^31 - 1 members.  hc_set_profile_stats turns it off: it re-creates what the histogram is keyed to.  Like the
 * profile table it is re-created, zeroed, when the points, the forcing rows or the depth change.  get / set take the
 * table's size in entries and fail on any other.  The step kernels are the same with the table on or off, and with it off
 * nothing is launched for it. */
int hc_set_theta_hist(hc_handle *h, int32_t n_bins);
int hc_get_theta_hist(hc_handle *h, int32_t *table, int64_t n_entries);
int hc_set_theta_hist_table(hc_handle *h, const int32_t *table, int64_t n_entries);   /* checkpoint / resume, rank sums */
int hc_reset_theta_hist(hc_handle *h);
int hc_get_theta_hist_outside(hc_handle *h, uint64_t *count);
int hc_get_theta_hist_bins(hc_handle *h, int32_t *n_bins);   /* 0: off */

/* Ensemble soil-water storage by depth layer: how much water [cm] each member holds between two depths, on the profile rows
 * (hc_set_profile_stats, which must be on), as exact integer moments and histograms over the members.  The nodes of a
 * column covary (one wetting front moves them together), so neither the per-node sigma nor the per-node histograms give a
 * layer's spread: the sum over depth is taken per member, before anything is reduced over the members.
 *   layers: L <= HC_STORAGE_MAX_LAYERS node ranges [i0_l, i1_l), 0 <= i0 < i1 <= D; layers may overlap or nest.
 *   rows: the profile rows, at the profile stride (slot j <-> row j stride, n_prow slots); row 0 is counted by
 *   hc_profile_snapshot, the others by hc_step_rows from the states the profile statistics read.  Skipped rows (wtd_obs < 0)
 *   count no members; spin-up solves accumulate nothing.
 *   per member m and layer l: T = sum_{i0 <= i < i1} theta_{m,i}, theta the cell model's theta_vol of the member's psi at the
 *   node with no noise term (the value the profile statistics quantise and hc_model_nodes returns, bit for bit);
 *   S = dz * T, the storage [cm of water]; u = T / (double)(i1 - i0), the layer's mean theta.  fp64, nothing contracted.
 *   The sum's order is fixed by (i0, i1) alone -- not by D, the launch length or the wave that got the member:
 *     x_j, j = 0..63, starts at 0.0 and adds theta_i of the layer's nodes with i mod 64 == j in ascending i;
 *     then x_j += x_{j+32} (j < 32), x_j += x_{j+16} (j < 16), ..., x_0 += x_1; T = x_0.
 *   moments (int64 table), in this order:
 *     stor [P][n_prow][L][5]   q = rint(S * 2^HC_PROF_SCALE_STORAGE), |q| <= HC_PROF_Q_MAX: word 0 sum q, words 1..4 the
 *                              20-bit limbs of sum q^2, as the profile statistics
 *     scnt [P][n_prow]         members counted in each row
 *     ovf  [1]                 values clamped by the quantisation or NaN
 *     P n_prow (5 L + 1) + 1 words.  |S| < 2^12 cm fits: a layer of (i1 - i0) dz >= 4096 cm is refused, so only a NaN (or a
 *     theta outside [0, 1]) can overflow.
 *   histogram (int32 table; n_bins = 0: none): hist [P][n_prow][L][B], B a power of two in 32 .. 1024, then the outside
 *     count as one uint64 in two more entries (low word first).  A member adds one to bin floor(u B) of its layer (u B is
 *     exact in fp64); u == 1.0 goes to bin B - 1; a u that is NaN, below 0 or above 1 goes to no bin and adds one to `outside`.
 *   Integer adds only across members: both tables are the same bits at any launch length, member split, point order and
 *   number of handles / ranks summed.
 * hc_set_layer_storage: n_layers 0 = off (default); otherwise (re)creates both tables zeroed.  `ranges` is [L][2] =
 * (i0, i1).  HC_ERR_ARG (and off) when the profile statistics are off, for more than HC_STORAGE_MAX_LAYERS layers, an empty
 * or out-of-column range, a layer of 4096 cm or more, any other bin count or a point of more than 2^31 - 1 members.
 * hc_set_profile_stats turns it off.  Like the profile table both tables are re-created, zeroed, when the points, the
 * forcing rows or the depth change (and refused then, if a range no longer fits the column).  get / set / export take the
 * table's size in words (hc_get_layer_storage_words) or entries (P n_prow L B + 2) and fail on any other; the histogram
 * calls fail when there is none.  hc_reset_layer_storage zeroes both.  hc_get_layer_storage_layout returns L, B and the
 * ranges ([HC_STORAGE_MAX_LAYERS][2], the first L filled).  The step kernels are the same with the tables on or off, and
 * with them off nothing is launched for them. */
#define HC_STORAGE_MAX_LAYERS 8
#define HC_PROF_SCALE_STORAGE 28    /* storage [cm]: 2^-28 cm steps, |S| < 2^12 cm                                  */
#define HC_STORAGE_MAX_CM 4096.0
int hc_set_layer_storage(hc_handle *h, int32_t n_layers, const int32_t *ranges, int32_t n_bins);
int hc_get_layer_storage_words(hc_handle *h, int64_t *n_words);
int hc_get_layer_storage(hc_handle *h, int64_t *table, int64_t n_words);
int hc_set_layer_storage_tables(hc_handle *h, const int64_t *table, int64_t n_words);   /* checkpoint / resume, rank sums */
int hc_export_layer_storage(hc_handle *h, void *device_dst, int64_t n_words);           /* as hc_export_profile_stats */
int hc_get_layer_storage_hist(hc_handle *h, int32_t *table, int64_t n_entries);
int hc_set_layer_storage_hist_table(hc_handle *h, const int32_t *table, int64_t n_entries);
int hc_reset_layer_storage(hc_handle *h);
int hc_get_layer_storage_outside(hc_handle *h, uint64_t *count);    /* 0 without a histogram */
int hc_get_layer_storage_overflow(hc_handle *h, uint64_t *count);   /* the ovf slot */
int hc_get_layer_storage_layout(hc_handle *h, int32_t *n_layers, int32_t *n_bins, int32_t *ranges);

/* Ensemble conductivity profiles: the mean and spread over the members of ln K_hrc and ln K_bkg at every node, and of the
 * effective vertical conductivity of depth layers, on the profile rows (hc_set_profile_stats, which must be on), as exact
 * integer moments.  K is the one quantity the model's noise enters, log-normal by construction and many decades wide down
 * an unsaturated column: the statistics are taken on ln K (exp of the mean is the geometric mean).
 *   rows: the profile rows, at the profile stride (slot j <-> row j stride, n_prow slots); row 0 is counted by
 *   hc_profile_snapshot, the others by hc_step_rows from the states the profile statistics read, before the row's
 *   assimilation (the forecast, as every table).  Skipped rows (wtd_obs < 0) count no members; spin-up solves accumulate nothing.
 *   noise: nu, the row's noise vector as its solve left it --
 *     a row that does not refresh the noise (and row 0): the member's base vector as it stands after the row, every
 *       earlier x0.8 in it;
 *     a refresh row: the row's own vector (draw index draw_idx[row], or the caller's / staged fresh vector), multiplied by
 *       0.8 once per failed attempt of that row, successive IEEE products.
 *     Vectors in memory (hc_set_noise_host; a Philox run whose handle fills caller noise: particle filter, the EnKF's
 *     noise field, a noise correlation): base_noise after the launch, or the launch's last staged fresh vector.  In-kernel
 *     Philox: philox_normal(seed, gid, 0, i) * nscale[m], one product, for the base; philox_normal(seed, gid,
 *     draw_idx[row], i) for a refresh row; gid as the step kernel keys it (member_offset + m, or the point's base + j).
 *     So that the base and the scale are the row's own, a launch ends on every profile row while the table is on, staged
 *     rows included, and the launch stages the per-row stats (the failed attempts of its last row).  No state depends on
 *     where a launch ends; the step kernels are the same.
 *   per member m and node i: (K_hrc, K_bkg) = the cell model at (psi_{m,i}, rnd = nu_i), the values hc_model_nodes returns
 *   on the same inputs, bit for bit; q = rint(log(K) * 2^HC_PROF_SCALE_LNK), |q| <= HC_PROF_Q_MAX (|ln K| < 2^10 covers
 *   every finite positive double).  A K that is not finite or not > 0 (K_hrc is exactly 0 where theta is clamped to
 *   theta_res) adds to no sum: every (node, quantity) has its own count.
 *   per member and layer l (node range [i0, i1), n = i1 - i0; at most HC_STORAGE_MAX_LAYERS, which may overlap):
 *   K_eff = (double)n / R, R = sum_{i0 <= i < i1} 1 / K_hrc,i -- the harmonic mean, which governs flow across layers --
 *   in the layer storage's order: x_j, j = 0..63, starts at 0.0 and adds 1 / K_hrc,i of the layer's nodes with i mod 64 == j
 *   in ascending i; then x_j += x_{j+32} (j < 32), ..., x_0 += x_1; R = x_0.  fp64, nothing contracted.  q =
 *   rint(log(K_eff) * 2^HC_PROF_SCALE_LNK); a member whose K_eff is not finite and > 0 is left out of that layer.  The sum
 *   over depth comes before the one over members: the nodes of one member covary.
 *   table (int64), in this order:
 *     kmom       [P][n_prow][D][2][5]  0 = K_hrc, 1 = K_bkg: word 0 sum q, words 1..4 the 20-bit limbs of sum q^2
 *     kcnt       [P][n_prow][D][2]     members added
 *     kmom_layer [P][n_prow][L][5]     ln K_eff, as kmom
 *     kcnt_layer [P][n_prow][L]        members added
 *     ovf        [1]                   values clamped by the quantisation
 *     P n_prow (12 D + 6 L) + 1 words.  Integer adds only across members: the same bits at any launch length, member split,
 *     point order and number of handles / ranks summed.
 * hc_set_conductivity_stats: n_layers -1 = off (default; hc_clear_conductivity_stats does the same), 0 = the node
 * statistics alone, otherwise with `ranges` [L][2] = (i0, i1); (re)creates the table zeroed.  HC_ERR_ARG (and off) when the
 * profile statistics are off, for more than HC_STORAGE_MAX_LAYERS layers, an empty or out-of-column range or a layer of
 * HC_STORAGE_MAX_CM or more.  hc_set_profile_stats turns it off.  Like the profile table it is re-created, zeroed, when the
 * points, the forcing rows or the depth change.  get / set / export take the table's size in words
 * (hc_get_conductivity_stats_words) and fail on any other.  hc_get_conductivity_stats_layout returns on / off, L and the
 * ranges ([HC_STORAGE_MAX_LAYERS][2], the first L filled).  With the table off nothing is launched or staged for it and no
 * launch is cut.
 * hc_conductivity_eval (test hook): out [4][N][D] = K_hrc, K_bkg, ln K_hrc, ln K_bkg of the members' current states with
 * the noise of forcing row `row` by the rule above and no failed attempt, from the same device code.  A refresh row of
 * vectors in memory reads the vector the last launch staged last. */
#define HC_PROF_SCALE_LNK 30        /* ln K: 2^-30 steps, |ln K| < 2^10                                             */
int hc_set_conductivity_stats(hc_handle *h, int32_t n_layers, const int32_t *ranges);
int hc_clear_conductivity_stats(hc_handle *h);
int hc_get_conductivity_stats_words(hc_handle *h, int64_t *n_words);
int hc_get_conductivity_stats(hc_handle *h, int64_t *table, int64_t n_words);
int hc_set_conductivity_stats_tables(hc_handle *h, const int64_t *table, int64_t n_words);   /* checkpoint / resume, rank sums */
int hc_export_conductivity_stats(hc_handle *h, void *device_dst, int64_t n_words);           /* as hc_export_profile_stats */
int hc_reset_conductivity_stats(hc_handle *h);
int hc_get_conductivity_stats_layout(hc_handle *h, int32_t *on, int32_t *n_layers, int32_t *ranges);
int hc_get_conductivity_stats_overflow(hc_handle *h, uint64_t *count);   /* the ovf slot */
int hc_conductivity_eval(hc_handle *h, int64_t row, double *out);

/* Ensemble covariance of theta(z) and the water table: the second moments of the members' theta_vol at the selected nodes
 * and of their water-table index, on the profile rows (hc_set_profile_stats, which must be on), in exact integers.  Every
 * other table is a marginal; this one says how the nodes of a column move together: the ensemble's vertical correlation,
 * the spread of the storage of any layer chosen after the run, cov(theta_i, wtd) for placing a sensor.
 *   nodes: with a node stride s >= 1 the selected nodes are i_k = k s, k = 0 .. n - 1, n = ceil(D / s); E = n + 1 columns,
 *   column n is the water table.
 *   rows: the profile rows, at the profile stride (slot j <-> row j stride, n_prow slots); row 0 is counted by
 *   hc_profile_snapshot, the others by hc_step_rows from the states the profile statistics read.  Skipped rows (wtd_obs < 0)
 *   count no members; spin-up solves accumulate nothing.
 *   per member: q_k = rint(theta_{i_k} 2^20) for k < n, theta the cell model's theta_vol of the member's psi at the node
 *   with no noise term (the value the profile statistics quantise and hc_model_nodes returns, bit for bit; theta 2^20 is
 *   exact, so the rounding is rint's alone; 0 <= q_k <= 2^20).  q_n = b, the find_wtd index of the staged state over all D
 *   nodes: one below the deepest node with !(psi >= psi_sat), clamped to D - 1, and 0 when there is none.
 *   A member is counted iff every selected theta satisfies 0 <= theta <= 1 (false for a NaN); a member that is not counted
 *   adds nothing to any word and one to `outside`.
 *   table (int64): per point and profile row W = 1 + E + E (E + 1) / 2 words,
 *     count            members counted
 *     S1 [E]           sum q_a
 *     S2 [E (E + 1) / 2]  sum q_a q_b for a <= b, packed by rows: entry (a, b) at a E - a (a - 1) / 2 + (b - a)
 *   as [P][n_prow][W], then the one `outside` word: P n_prow W + 1 words.  A product is at most 2^40 (below 2^41); a point holds at most
 *   2^22 members (HC_THETA_COV_MAX_MEMBERS), so S2 <= 2^62 fits an int64.  Integer adds only: the table is the same bits at
 *   any launch length, member split, chunk length, point order and number of handles / ranks summed.
 * hc_set_theta_cov: node_stride 0 = off (default); otherwise (re)creates the table zeroed.  HC_ERR_ARG (and off) when the
 * profile statistics are off, for a stride below 1 or above D, for a point of more than HC_THETA_COV_MAX_MEMBERS members
 * and for a table of more than HC_THETA_COV_MAX_WORDS words (take a larger node stride or a larger profile stride).
 * hc_set_profile_stats turns it off.  Like the profile table it is re-created, zeroed, when the points, the forcing rows
 * or the depth change.  get / set / export take the table's size in words (hc_get_theta_cov_words) and fail on any other.
 * The members' quantised rows are staged in device memory allocated on first use, at most 1 GiB: a larger ensemble runs
 * in chunks of members (test hook: HYDROCOL_COV_CHUNK_MEMBERS in the environment at hc_create forces the chunk length).
 * The step kernels are the same with the table on or off, and with it off nothing is launched or allocated for it. */
#define HC_THETA_COV_SCALE 20                       /* theta: 2^-20 steps */
#define HC_THETA_COV_MAX_MEMBERS (1LL << 22)        /* per point: 2^22 products of at most 2^40 keep S2 <= 2^62 */
#define HC_THETA_COV_MAX_WORDS (1LL << 30)          /* 8 GiB of int64 words */
int hc_set_theta_cov(hc_handle *h, int32_t node_stride);
int hc_get_theta_cov_layout(hc_handle *h, int32_t *node_stride, int32_t *n_nodes, int64_t *words_per_row);   /* 0, 0, 0: off */
int hc_get_theta_cov_words(hc_handle *h, int64_t *n_words);
int hc_get_theta_cov(hc_handle *h, int64_t *table, int64_t n_words);
int hc_set_theta_cov_tables(hc_handle *h, const int64_t *table, int64_t n_words);   /* checkpoint / resume, rank sums */
int hc_export_theta_cov(hc_handle *h, void *device_dst, int64_t n_words);           /* as hc_export_profile_stats */
int hc_reset_theta_cov(hc_handle *h);
int hc_get_theta_cov_outside(hc_handle *h, uint64_t *count);

/* Period totals per member: what each member's transpiration and lateral flow sum to over a period of forcing rows (a
 * month, a season, a year), how shallow and how deep its water table got in the period and on how many rows it stood at or
 * above a depth (the hydroperiod), as exact integer moments and histograms over the members.  The rows of one member are
 * correlated in time (one wetting front, one water table), so neither the per-row sigmas nor the per-row histograms give
 * a period's spread: the rows are aggregated per member first, and only then is anything reduced over the members.
 *   periods: n_period <= HC_PERIOD_MAX_PERIODS inclusive end rows e_0 < e_1 < ..., 1 <= e_p < n_rows.  Period p covers the
 *   forcing rows (e_{p-1}, e_p], period 0 starts at row 1, each holds at most HC_PERIOD_MAX_ROWS rows; rows after the last
 *   end belong to no period.  A skipped row (wtd_obs < 0) adds nothing but still closes a period when it is an end row.
 *   Spin-up solves accumulate nothing.  hc_step_rows ends a launch on every end row (states do not depend on it).
 *   accumulators (int64 [K][N], K = 4 + n_thresholds <= 8, member m of plane k at k N + m), from the diag and the
 *   water-table index the row's launch stored for member m:
 *     0  transpiration   sum over the period's solved rows of q = rint(diag[.,0] * 2^HC_PROF_SCALE_FLUX), |q| <=
 *                        HC_PROF_Q_MAX (the profile statistics' rule; a clamped or NaN value adds one to ovf)
 *     1  lateral_flow    the same of diag[.,1]
 *     2  wtd_shallowest  the smallest water-table index of the period's solved rows (65535: none yet)
 *     3  wtd_deepest     the largest (0: none yet)
 *     4 + j              the solved rows with water-table index <= threshold_nodes[j]
 *   At the end of a period, from the members that had a solved row in it (wtd_shallowest != 65535), per point:
 *   moments (int64 table), in this order:
 *     pmom [P][n_period][K][5]  word 0 the sum of v, words 1..4 the 20-bit limbs of the sum of v^2, as the profile
 *                               statistics; v = A >> 12 = floor(A / 4096) for the two flux totals (units of 2^-20 cm,
 *                               clamped to |v| <= HC_PROF_Q_MAX and counted in ovf), v = A for the indices and counts
 *     pcnt [P][n_period]        the members counted (0 for a period with no solved row)
 *     ovf  [1]
 *     P n_period (5 K + 1) + 1 words.
 *   histograms (int32 table; n_bins = 0: none), in this order:
 *     phist_flux [P][n_period][2][B]  B a power of two in 32 .. 1024 over [0, 2^e_q) cm, e_q = flux_max_log2[q] in
 *                                     -8 .. 12: bin (v B) >> (20 + e_q) for 0 <= v < 2^(20 + e_q), any other v adds one
 *                                     to `outside`
 *     phist_wtd  [P][n_period][2][D]  the shallowest and the deepest index of each member
 *     then `outside` as one uint64 in two more entries (low word first): P n_period 2 (B + D) + 2 entries.
 *   The threshold counts have moments only.  After the reduction the members' accumulators are reset (0, 0, 65535, 0,
 *   0 ...).  On an assimilation row the reduction runs before the resampling or the analysis: the tables describe the
 *   forecast.  The particle filter's resampling copies an ancestor's accumulators with its state (acc_out[k][m] =
 *   acc_in[k][anc[m]]: the filter's path estimate); EnKF members persist.  Integer adds only: the tables are the same
 *   bits at any launch length, member split, point order and number of handles / ranks summed.
 * hc_set_period_totals: n_periods 0 = off (default); otherwise (re)creates the tables zeroed and the accumulators reset.
 * HC_ERR_ARG (and off) for ends that do not ascend or lie outside [1, n_rows), more than HC_PERIOD_MAX_PERIODS periods or
 * HC_PERIOD_MAX_ROWS rows in one, more than HC_PERIOD_MAX_THRESHOLDS thresholds, a threshold node outside the column, any
 * other bin count or exponent, and while a sharded particle filter is set (hc_set_filter_shard, which in turn refuses
 * while period totals are set: the routed columns do not carry the accumulators).  The tables are re-created, zeroed,
 * when the points, the forcing rows or the depth change, the accumulators when the member count does.  get / set /
 * export take the size in words (hc_get_period_totals_words; K N for the accumulators) or entries and fail on any other;
 * the histogram calls fail when there is none.  hc_reset_period_totals zeroes the tables and resets the accumulators.
 * hc_get_period_totals_layout returns the counts, the threshold nodes ([HC_PERIOD_MAX_THRESHOLDS]), the exponents ([2])
 * and, if end_rows is not NULL, the first n_end_rows end rows.  The step kernels are the same with the tables on or off
 * (a launch stores diag as it does for the profile statistics), and with them off nothing is launched or allocated. */
#define HC_PERIOD_MAX_PERIODS 4096
#define HC_PERIOD_MAX_ROWS (1 << 20)
#define HC_PERIOD_MAX_THRESHOLDS 4
int hc_set_period_totals(hc_handle *h, int32_t n_periods, const int64_t *end_rows, int32_t n_thresholds,
                         const int32_t *threshold_nodes, int32_t n_bins, const int32_t *flux_max_log2);
int hc_get_period_totals_words(hc_handle *h, int64_t *n_words);
int hc_get_period_totals(hc_handle *h, int64_t *table, int64_t n_words);
int hc_set_period_totals_tables(hc_handle *h, const int64_t *table, int64_t n_words);   /* checkpoint / resume, rank sums */
int hc_export_period_totals(hc_handle *h, void *device_dst, int64_t n_words);           /* as hc_export_profile_stats */
int hc_get_period_totals_hist(hc_handle *h, int32_t *table, int64_t n_entries);
int hc_set_period_totals_hist_table(hc_handle *h, const int32_t *table, int64_t n_entries);
int hc_export_period_totals_hist(hc_handle *h, void *device_dst, int64_t n_entries);
int hc_get_period_totals_acc(hc_handle *h, int64_t *acc, int64_t n_words);              /* [K][N], for checkpoints */
int hc_set_period_totals_acc(hc_handle *h, const int64_t *acc, int64_t n_words);
int hc_reset_period_totals(hc_handle *h);
int hc_get_period_totals_outside(hc_handle *h, uint64_t *count);    /* 0 without histograms */
int hc_get_period_totals_overflow(hc_handle *h, uint64_t *count);   /* the ovf slot */
int hc_get_period_totals_layout(hc_handle *h, int32_t *n_periods, int32_t *n_thresholds, int32_t *n_bins,
                                int32_t *threshold_nodes, int32_t *flux_max_log2, int64_t *end_rows, int64_t n_end_rows);

/* Root-water uptake by depth: from which layer the trees take their water in each period of hc_set_period_totals, per
 * member first (the rate is zero at night: a sampled row says nothing), then as exact integer moments, share histograms
 * and a depth profile over the members.  The sink depends on theta at the midpoints, the root and porosity tables and the
 * row's atm / daylight alone, so it is evaluated after the fact from the end state of every solved daylight row: a
 * launch stages its rows' end states (as a short profile stride does, within the same ~4 GiB) and a kernel behind it reads
 * them.  The step kernels are the same with the feature on or off.
 *   quantity, for a member's psi [D] after the solve of forcing row r (normal mode, flag_et on, daylight), M = D - 1:
 *     y_i = 0.5 (psi_i + psi_{i+1}), theta_i = the cell model's theta at y_i with the midpoint porosity (no noise term),
 *     u_i >= 0 the uptake the reference's RHS applies at that state (its sink is -u_i): cells 1 .. n_root_int from the
 *     interior call, normalised together; cell 0 from the first-midpoint call, normalised on its own, when n_root_first
 *     = 1; zero elsewhere, on a night row, with flag_et off.  With R = cells 1 .. n = n_root_int, in fp64 without
 *     contraction, every division a division:
 *       water_k = dz S(theta_i - wlt_i); water_k <= 0: all zero.  Otherwise
 *       c_i = C(theta)_i, total = dz C(theta)_n' (0 -> 1), a1_i = max(theta_i invd1_i, (dz c_i) / total),
 *       a2_i = theta_i > fc_i; g = 0.1 when a2_i holds on all of R, else 1; rho_i = a2_i ? |a1_i g| : 0,
 *       tot = dz S(rho) (0 -> 1), x_i = (rho_i / tot) root_i, tot_x = dz S(x);
 *       tot_x > 1: x_i = x_i / tot_x, tot_x = dz S(x);  tot_x > 0: u_i = (min(atm, water_k) / tot_x) x_i, else zero.
 *     The first-midpoint call is the same with R = {0} (one cell: no sums, c_0 = theta_0, g = 0.1).
 *     invd1 = 1 / (por - wlt) (0 -> 1) is formed once on the host.
 *   order of the sums (fixed by n_root_int alone; cell i sits in round i / 64 at lane i % 64, cells outside R add 0.0):
 *     S(v): lane j's partial p_j = the values of its cells by ascending round, from 0.0; then for s = 32, 16 .. 1:
 *       p_j += p_{j+s} (j < s); S = p_0.
 *     C(v): per round the inclusive scan over the lanes by doubling offsets -- for o = 1, 2 .. 32: t_j += t_{j-o}
 *       (j >= o), all lanes at once -- and c_i = carry + t_j, where carry = the sum, by ascending round from 0.0, of the
 *       earlier rounds' t_63.  C(v)_n' = the carry after the last round that holds a cell of R.
 *   layers: L <= HC_UPTAKE_MAX_LAYERS ranges [lo_l, hi_l) of midpoint cells, 0 <= lo < hi <= M; they may overlap or lie
 *     below the roots.  U_0 = dz S'(u over every cell), U_l = dz S'(u over the layer's cells), S' = S over the cells
 *     0 .. n_root_int (cell 0 included).
 *   accumulators (int64 [L + 1][N], member m of plane l at l N + m): the sum over the period's solved daylight rows of
 *     q = rint(U_l 2^HC_PROF_SCALE_FLUX), |q| <= HC_PROF_Q_MAX (a clamped or NaN value adds one to ovf).
 *   depth profile: q_i = rint(u_i 2^HC_UPTAKE_SCALE_PROFILE) of every member and solved daylight row of period p, clamped
 *     to HC_PROF_Q_MAX (counted in ovf; so is a negative q_i, which adds nothing), added as two 20-bit limbs
 *     q_i & (2^20 - 1) and q_i >> 20 to uprof [P][n_period][M][2]: 2^22 members x 2^20 rows x 2^20 stays below 2^62.
 *   At the end of a period, before the period totals' own reduction and from the members it counts (those with a solved
 *   row in the period), per point, v_l = A_l >> 12 = floor(A_l / 4096) (units of 2^-20 cm, clamped to |v| <=
 *   HC_PROF_Q_MAX and counted in ovf):
 *   tables (int64), in this order:
 *     umom  [P][n_period][L + 1][5]  word 0 the sum of v_l, words 1..4 the 20-bit limbs of the sum of v_l^2
 *     ucnt  [P][n_period]            the members counted
 *     uprof [P][n_period][M][2]
 *     ovf   [1]
 *     P n_period (5 (L + 1) + 1 + 2 M) + 1 words.
 *   histogram (int32; n_bins = 0: none): [P][n_period][L][B], B a power of two in 32 .. 1024: a counted member adds one
 *     per layer to bin min(B - 1, (v_l B) / v_0) -- the layer's share of its total, by integer division -- and a member
 *     with v_0 <= 0 adds one to `outside` instead, one uint64 in two more entries (low word first): P n_period L B + 2.
 *   After the reduction the accumulators are reset to 0.  On an assimilation row the reduction runs before the resampling
 *   or the analysis; the particle filter's resampling copies an ancestor's accumulators with its state, EnKF members
 *   persist.  Integer adds only beyond the member: the tables are the same bits at any launch length, member split, point
 *   order and number of handles summed.
 * hc_set_root_uptake: n_layers 0 = off (default); otherwise (re)creates the tables zeroed and the accumulators reset.
 * HC_ERR_ARG (and off) while the period totals are off, for more than HC_UPTAKE_MAX_LAYERS layers, an empty or
 * out-of-column range, any other bin count, and while a sharded particle filter is set (hc_set_filter_shard, which in
 * turn refuses while this is set).  hc_set_period_totals with other end rows, hc_set_members and hc_set_column turn it
 * off; hc_set_period_totals with the same end rows re-creates it zeroed.  get / set / export take the size in words
 * (hc_get_root_uptake_words; (L + 1) N for the accumulators) or entries and fail on any other; the histogram calls fail
 * when there is none.  hc_get_root_uptake_layout fills cell_lo / cell_hi ([HC_UPTAKE_MAX_LAYERS]).  With the feature off
 * nothing is launched, staged or allocated for it and no launch is cut.
 * hc_root_uptake_eval (test hook): theta_mid and u, [N][M] each, of the members' CURRENT states on forcing row `row`
 * (its atm and daylight; a night row gives u = 0), computed by the same device code; needs no hc_set_root_uptake. */
#define HC_UPTAKE_MAX_LAYERS 8
#define HC_UPTAKE_SCALE_PROFILE 44    /* u [1 / row]: 2^-44 steps, u < 2^-4 */
int hc_set_root_uptake(hc_handle *h, int32_t n_layers, const int32_t *cell_lo, const int32_t *cell_hi, int32_t n_bins);
int hc_get_root_uptake_words(hc_handle *h, int64_t *n_words);
int hc_get_root_uptake(hc_handle *h, int64_t *table, int64_t n_words);
int hc_set_root_uptake_tables(hc_handle *h, const int64_t *table, int64_t n_words);    /* checkpoint / resume, rank sums */
int hc_export_root_uptake(hc_handle *h, void *device_dst, int64_t n_words);            /* as hc_export_profile_stats */
int hc_get_root_uptake_hist(hc_handle *h, int32_t *table, int64_t n_entries);
int hc_set_root_uptake_hist_table(hc_handle *h, const int32_t *table, int64_t n_entries);
int hc_export_root_uptake_hist(hc_handle *h, void *device_dst, int64_t n_entries);
int hc_get_root_uptake_acc(hc_handle *h, int64_t *acc, int64_t n_words);               /* [L + 1][N], for checkpoints */
int hc_set_root_uptake_acc(hc_handle *h, const int64_t *acc, int64_t n_words);
int hc_reset_root_uptake(hc_handle *h);
int hc_get_root_uptake_outside(hc_handle *h, uint64_t *count);     /* 0 without a histogram */
int hc_get_root_uptake_overflow(hc_handle *h, uint64_t *count);    /* the ovf slot */
int hc_get_root_uptake_layout(hc_handle *h, int32_t *n_layers, int32_t *n_bins, int32_t *cell_lo, int32_t *cell_hi);
int hc_root_uptake_eval(hc_handle *h, int64_t row, double *theta_mid, double *u);

/* Particle filter on the well's water table (bootstrap filter, systematic resampling in exact integers).
 *   Assimilation rows: r >= 1, r % stride == 0 and wtd_obs[r] >= 0 (wtd_obs as it stands when hc_step_rows reaches the row:
 *   hc_set_forcing_row before the row's step sets or removes its observation).  Slot j <-> row j stride,
 *   n_arow = (n_forcing_rows - 1) / stride + 1; slot 0 stays empty.  A launch ends on every assimilation row (results do not
 *   depend on launch length); spin-up solves are never filtered.
 *   Order at an assimilation row: the row is solved; every table on the handle (moments, profile statistics, histograms)
 *   accumulates it -- they describe the FORECAST ensemble; then the filter resamples.  After the call hc_get_state returns
 *   the ANALYSIS; psi_rows_out and wtd_out hold the forecast of the row.
 *   Weights, per parameter point p (members [p N_p, (p + 1) N_p)), o = wtd_obs[r], b = a member's water-table index
 *   (the index hc_step_args.wtd_out returns), n_b = members of p in bin b, all in fp64 without contraction:
 *     t_b = dz * (double)(b - o) / sigma_cm;  l_b = -0.5 * (t_b * t_b);  s = max l_b over the bins with n_b > 0;
 *     q_b = floor(2^31 * exp(l_b - s)) for n_b > 0, q_b = 0 for an empty bin: q = 2^31 at the nearest occupied bin, and a
 *     bin more than ~6.5 sigma further from the well than that gets q = 0 (truncation: such members leave no offspring).
 *   Resampling, member order within the point: C_m = exclusive prefix sum of q_m = q_{b_m} (int64), Q = sum q_m;
 *   x = one 64-bit Philox4x32-10 value (the first two output words, word 1 high) under the key filter seed, counter
 *   (0xFFFFFFFF, row, key_lo, key_hi) with key = the point's first global member id (hc_set_point_member_bases; one point:
 *   member_offset) -- a noise counter's first word is a depth index / 2, so the two never meet; r = floor(x Q / 2^64).
 *   Slot k takes the member m with C_m <= floor((k Q + r) / N_p) < C_m + q_m: member m fills
 *   k in [ceil((C_m N_p - r) / Q), ceil(((C_m + q_m) N_p - r) / Q)) (128-bit intermediates; the ranges partition [0, N_p)).
 *   All integers: the ancestry depends on no reduction order, launch length, point order or rank count.  With equal weights
 *   (sigma_cm = 1e30) it is the identity.
 *   A member's Markov state is (psi, base noise vector): slot k takes both from its ancestor.  Refresh vectors stay keyed by
 *   the slot's own stream.  Host noise: h->base is gathered with psi; the caller keeps drawing slot k's refresh vectors
 *   from slot k's generator.  Philox noise: with the filter on the step kernel runs its caller-noise path; the library
 *   fills the base vectors once, in hc_set_filter, as z * scale (z = the kernel's draw-0 normal of the slot, scale =
 *   hc_set_noise_scale's value, one rounding), and each launch's refresh vectors from the slot's stream and the row's draw
 *   index (a launch stages at most ~4 GiB of them).  The x0.8 retry damping then follows the host-noise semantics
 *   (applied to the base vector in place, src/richards_pde.py:522), which are the reference's.
 *   Diagnostics, float64 [P][n_arow][4] per point and slot: count = sum_b n_b; ESS = (sum n_b q_b)^2 / sum n_b q_b^2 (exact
 *   128-bit sums, the quotient from a double-double correction, within 2 ulp of the exact ratio); the log-likelihood increment
 *   s + log(W / count) - log(sigma_cm) - 0.5 * log(2 pi), W = sum_b n_b exp(l_b - s) summed in increasing b (log cm^-1: the
 *   Gaussian density of the observed depth given the member's, averaged over the members); survivors = members with at
 *   least one offspring.  Slots without an assimilation hold count = 0 and NaN.  A point's log marginal likelihood is the
 *   sum of its increments in row order (on the host).
 * hc_set_filter: stride 0 = off; otherwise (re)creates the table, and in a Philox run fills the base vectors.  Needs column,
 *   forcing, members and noise source; sigma_cm finite and > 0; at most 2^31 - 1 members per point, 2^32 - 1 rows.
 *   A later hc_set_column / hc_add_point / hc_set_point_member_bases, hc_set_members, hc_set_noise_host or
 *   hc_set_noise_philox turns the filter off; hc_set_forcing re-creates the table (count 0, NaN) when the row count changes.
 *   With the filter on in a Philox run, hc_spinup / spin-up rows and hc_set_noise_scale are refused (the base vectors carry
 *   the damping: set scales and do spin-ups before hc_set_filter) and hc_get_noise_scale no longer follows the run.
 * hc_get/set_filter_stats: the table (P n_arow 4 entries; checkpoints, the assembly of a sweep over ranks).
 * hc_get/set_filter_base: the device base vectors [n_members][D] of a filtered Philox run (resume).
 * Test hooks of the last assimilation: ancestors [n_members] int64 (handle-local member index of each slot's ancestor;
 *   hc_set_filter_shard: the global one), weights [P][D] int64 (q_b), draw [P] int64 (r). */
int hc_set_filter(hc_handle *h, int32_t stride, double sigma_cm, uint64_t seed);
int hc_get_filter_stats(hc_handle *h, double *table, int64_t n_entries);
int hc_set_filter_stats(hc_handle *h, const double *table, int64_t n_entries);
int hc_get_filter_base(hc_handle *h, double *base, int64_t first_member, int64_t count);
int hc_set_filter_base(hc_handle *h, const double *base);
int hc_get_filter_ancestors(hc_handle *h, int64_t *ancestors);
int hc_get_filter_weights(hc_handle *h, int64_t *q);
int hc_get_filter_draw(hc_handle *h, int64_t *r);

/* Tempered weights: hold the effective sample size of every resampling above a floor (Poterjoy's beta-regularisation of
 * the localised particle filter, 2016 / 2019; equivalently the observation error inflated by 1 / sqrt(beta), per row and
 * point).  On an assimilation row the weight kernels above (or the sensor rows' below) run first and are untouched: count
 * n, s, l_b per occupied bin (l_m per counted member on a sensor row), q at beta = 1, and entries 0-2 of the filter's
 * table -- count, ESS and increment stay those of the stated observation error, so the log-likelihood stays comparable
 * between tempered and untempered runs.  Entry 3 (survivors) counts the resampling that actually happened.  Then, per
 * parameter point, in exact integers but for the exp of a weight:
 *   T = min(n, max(1, (int64) ceil(ess_floor * (double) n)));
 *   for k in 0 ... 1024, beta_k = k / 1024 (exact): q(k) = floor(2^31 * exp(beta_k * (l - s))) for a counted member or an
 *   occupied bin -- l - s and the product each rounded once, no contraction -- and 0 otherwise; q(1024) are the bits above;
 *   Q_k = sum q(k), S_k = sum q(k)^2 over the members (a bin counts n_b times): Q_k exact in 64 bits, S_k in 128;
 *   ok(k) <=> Q_k * Q_k >= T * S_k, both sides exact in 128 bits (Q_k < 2^62, T < 2^31, S_k < 2^93); ok(0) always holds.
 *   Trial 0 is k = 1024: if ok, beta = 1 and nothing is rewritten -- the weights, {Q, r}, the ancestry and everything
 *   downstream are the untempered run's bits.  Otherwise lo = 0, hi = 1024 and, while hi - lo > 1: mid = (lo + hi) >> 1;
 *   ok(mid) ? lo = mid : hi = mid -- ten more trials (512, ...) -- and k = lo.  k is DEFINED as the outcome of this
 *   procedure (the floors make ESS(beta) not strictly monotone).
 *   k < 1024: the point's weights become q(k) (the bin table q_b, or q_m of a sensor row) and its draw
 *   {Q_k, floor(x * Q_k / 2^64)} with the same Philox value x (same counter: no new randomness); the prefix scan, the slot
 *   fill, the survivors, the gather, the sharded routing, the period accumulators' gather and the sensors' posterior moments
 *   run on these values as they run without tempering.  k = 0: the observation is ignored on that row.  exp(l_m - s) of a
 *   sensor row (hc_get_filter_loglik's neighbour column, the source of W) is not rewritten.
 *   A row with n = 0 is not tempered.  k depends on no launch length, member split, point order or rank count.
 *   The table, float64 [P][n_arow][4] per point and slot: beta = k / 1024; the ESS at beta = Q_k^2 / S_k (the quotient of
 *   the filter's table; at beta = 1 that table's ESS to the bit); T; the trials evaluated (1 or 11).  Slots without an
 *   assimilation and rows that were not tempered hold NaN.
 * hc_set_filter_tempering: ess_floor = 0 turns tempering off (the default: nothing is launched or allocated); otherwise
 *   finite with 0 < ess_floor < 1 (HC_ERR_ARG else) and the particle filter on (hc_set_filter first).  Whatever turns the
 *   filter off removes it, hc_set_filter included.  Valid with a soil-moisture record, a sweep, either noise source, period
 *   totals and hc_set_filter_shard (every handle runs the same kernels on the same gathered indices and finds the same k).
 * hc_get/set_filter_temper_stats: the table (P n_arow 4 entries; checkpoints, the assembly of a sweep over ranks).
 * Test hook of the last assimilation: hc_get_filter_temper_trials, int64 [P][11][4] = {k, Q_k, S_k low word, S_k high
 *   word} in trial order, unused rows k = -1 (a row that was not tempered: all of them).  hc_get_filter_weights,
 *   hc_get_filter_member_weights and hc_get_filter_draw return what the resampling used. */
int hc_set_filter_tempering(hc_handle *h, double ess_floor);
int hc_get_filter_temper_stats(hc_handle *h, double *table, int64_t n_entries);
int hc_set_filter_temper_stats(hc_handle *h, const double *table, int64_t n_entries);
int hc_get_filter_temper_trials(hc_handle *h, int64_t *trials);

/* Rejuvenated base vectors: the kernel-shrinkage move of Liu & West (2001) on the members' base noise vectors.  A member's
 * base vector is its static log-conductivity field (src/simulation.py:598-602 uses it on every row that is neither wet
 * nor a multiple of 48), and resampling a static quantity only loses values: after a non-trivial resampling several slots
 * of a point share one vector and nothing in the dynamics separates them again.  With a discount delta,
 *   a = (3 delta - 1) / (2 delta),  h = sqrt(1 - a a)   (host, fp64, every operation rounded once),
 * an assimilation row ends -- after the gather, the buffer swap, the period accumulators' gather and the sensors' posterior
 * moments -- with, per parameter point p of N_p members:
 *   Trigger: the point is rejuvenated iff 0 < survivors < N_p (entry 3 of the filter's table, read on the device: no host
 *   synchronisation).  Systematic resampling is monotone, so survivors = N_p is the identity ancestry: flat weights and
 *   the neutral filter leave every vector to the bit.
 *   Moments of the resampled vectors x [N_p][D], node by node, by the EnKF's spread passes (differences from the point's
 *   first member, tiles of 256 members in member order, the tile partials strided over 1024 threads and a fixed tree):
 *   mean_d = x_0d + S1_d / N_p, S1_d = sum_k (x_kd - x_0d);  s_d = sqrt(S2_d / (N_p - 1)), S2_d = sum_k ((x_kd - x_0d) -
 *   S1_d / N_p)^2  (N_p = 1: 0).
 *   Update, no contraction:  z'_kd = (mean_d + a (z_kd - mean_d)) + (h s_d) eps_kd,  eps a standard normal of
 *   Philox4x32-10 under the filter's seed at counter (0x80000000 | (d >> 1), row, gid_lo, gid_hi), gid the slot's global
 *   member id (point base + j, or member offset + m: the id of the EnKF's draws), Box-Muller as the noise's normals: the
 *   cosine for even d, the sine for odd d, both from one block.  A noise counter's first word is below 2^31, the filter's
 *   draw and the EnKF's are >= 0xFFFFFFF0: the streams never meet, even under equal seeds.
 *   Vote: the new vector is stored only if every entry is finite; otherwise the member keeps its vector and is counted.
 *   psi and the refresh rows' one-row vectors are not touched.  The ensemble's mean and variance per node are, in
 *   expectation, what the resampling left (a^2 + h^2 = 1), and no two members share a field.  With a single survivor
 *   s_d = 0 and nothing can be restored: hold the ESS up as well (hc_set_filter_tempering).
 *   The table, float64 [P][n_arow][4] per point and slot: applied (1 / 0); members refused; sqrt(sum_d s_d^2 / D) of the
 *   resampled vectors; the same of the vectors the move left (two more spread passes).  The last two are summed by one
 *   thread, nodes ascending, and NaN when not applied; slots without an assimilation hold NaN.
 * hc_set_filter_rejuvenation: discount = 0 turns it off (the default: nothing is launched or allocated); otherwise finite
 *   with 0.5 <= discount < 1 (HC_ERR_ARG else), the particle filter on (hc_set_filter first) and not sharded:
 *   hc_set_filter_shard gathers water-table indices only, the moments would need an exchange of their own, and each of the
 *   two refuses while the other is set.  Whatever turns the filter off removes it, hc_set_filter included.  Valid with a
 *   soil-moisture record, tempering, a window, period totals, a sweep and either noise source.
 * hc_get_filter_rejuvenation: discount and a (0, 0: off).
 * hc_get/set_filter_rejuvenation_stats: the table (P n_arow 4 entries; checkpoints, the assembly of a sweep over ranks).
 * Test hooks: hc_get_filter_rejuvenation_moments, the last assimilation's float64 [P][3][D] = mean_d, s_d of the resampled
 *   vectors and s_d of the vectors the move left (computed whether or not the point was rejuvenated);
 *   hc_filter_rejuvenation_normals, stateless: eps of the handle's slots first_member ... first_member + count - 1 at
 *   forcing row `row`, out [count][D] (the filter on; the draws themselves are never stored). */
int hc_set_filter_rejuvenation(hc_handle *h, double discount);
int hc_get_filter_rejuvenation(hc_handle *h, double *discount, double *shrinkage);
int hc_get_filter_rejuvenation_stats(hc_handle *h, double *table, int64_t n_entries);
int hc_set_filter_rejuvenation_stats(hc_handle *h, const double *table, int64_t n_entries);
int hc_get_filter_rejuvenation_moments(hc_handle *h, double *moments);
int hc_filter_rejuvenation_normals(hc_handle *h, int64_t row, int64_t first_member, int64_t count, double *out);

/* Soil-moisture sensors in the particle filter: a record of volumetric water content at up to 8 depth nodes joins the well
 * in the weights, which then belong to a member and not to a bin.  values [n_forcing_rows][n_sensors], NaN = no observation
 * on that row; sigma [n_sensors] (m^3/m^3) finite and > 0; nodes in [0, D).
 *   Assimilation rows do not change: r >= 1, r % stride == 0 and wtd_obs[r] >= 0.  A row on which no sensor has a value runs
 *   the bin path of hc_set_filter untouched: an all-NaN record gives the well-only run to the bit (states, table, hooks).
 *   A row with m_s >= 1 sensor values, per parameter point p (N_p members, member order), fp64 without contraction:
 *     theta_m,i = the reference's theta_vol of member m's forecast psi at the node of present sensor i (the cell model of
 *     hc_model_nodes, to its bits; theta has no noise term);
 *     t_w = dz * (double)(b_m - o) / sigma_cm;  a = t_w * t_w;  for each present sensor in record order:
 *     u = (theta_m,i - theta_obs,i) / sigma_i;  a += u * u;  then l_m = -0.5 * a;
 *     a member with b_m >= D or a non-finite l_m is not counted and gets q_m = 0; s = max l_m over the counted members;
 *     e_m = exp(l_m - s);  q_m = floor(2^31 * e_m): 2^31 at the likeliest member.
 *   Resampling: C_m, Q, the draw r (the same Philox counter) and the slot ranges as for hc_set_filter, on q_m as it stands:
 *   the ancestry is an integer function of q_m, and q_m of nothing but the member's own column and the point's s (a maximum:
 *   no order).
 *   Sums over a point's members, the one order of every floating-point sum on this path (fixed by N_p alone, no
 *   floating-point atomics): tiles of 1024 consecutive members; within a tile, 256 threads take 4 consecutive members each,
 *   summed in member order from 0.0; the 256 thread sums are combined in a tree of halving strides (x_i += x_{i + 128}, then
 *   x_i += x_{i + 64}, ... x_0 += x_1); the tile sums are added in ascending tile order from 0.0.  Members past N_p add 0.0.
 *   The filter's table on such a row: count = the counted members; ESS = Q^2 / sum q_m^2 (exact sums, as for hc_set_filter);
 *   the increment, in this order,
 *     s + log(W / count) - log(sigma_cm) - log(sigma_i) for each present sensor in record order
 *       - 0.5 * (double)(1 + m_s) * log(2 pi),   W = sum e_m over the counted members (the order above; others add 0.0):
 *   the joint Gaussian density of the observed vector given the member's, averaged over the members, in
 *   log cm^-1 (m^3/m^3)^-m_s; survivors as before.  The table is the same bits at any launch length and point order.
 *   Sensor diagnostics, float64 [P][n_arow][n_sensors][6]: observed (0/1), observation, forecast mean of theta (sum / N_p),
 *   forecast std of theta (two passes: squared deviations from that mean, / (N_p - 1), 0 for N_p = 1), posterior mean and std
 *   of theta over the resampled slots, theta_{anc[k]} (theta is a function of the copied column), every sum in the order
 *   above.  A sensor without a value on a sensor row: observed = 0, the rest NaN; a slot without a sensor row: all NaN.
 * hc_set_filter_soil_moisture: n_sensors = 0 removes the record; otherwise (re)creates the sensor table (NaN).  Needs the
 *   particle filter on (hc_set_filter first); HC_ERR_ARG while the EnKF is on, for more than 8 sensors, a node outside the
 *   column, a sigma that is not finite and > 0, a value outside [0, 1].  Whatever turns the filter off removes the record
 *   (hc_set_filter included).  hc_step_rows refuses while the record's row count differs from the forcing's.
 *   With a record set hc_set_filter_shard is refused, and with sharding set so is the record (HC_ERR_ARG either way): the
 *   sharded filter gathers water-table indices only.  A sweep dealt by whole points runs on any number of handles.
 * hc_get/set_filter_sm_stats: the sensor table (P n_arow n_sensors 6 entries; checkpoints, the assembly of a sweep over ranks).
 * Test hooks of the last assimilation, with a record set: hc_get_filter_sm_width (m_s; 0: it took the bin path),
 *   hc_get_filter_member_weights (q_m [n_members] int64; after a bin-path row q_{b_m}); after a sensor row also
 *   hc_get_filter_loglik (l_m [n_members]) and hc_get_filter_sm_theta ([n_members][m_s]), and hc_get_filter_weights (the
 *   bin table) is zero. */
int hc_set_filter_soil_moisture(hc_handle *h, int32_t n_sensors, const int32_t *nodes, const double *values,
                                const double *sigma);
int hc_get_filter_sm_stats(hc_handle *h, double *table, int64_t n_entries);
int hc_set_filter_sm_stats(hc_handle *h, const double *table, int64_t n_entries);
int hc_get_filter_sm_width(hc_handle *h, int32_t *width);
int hc_get_filter_member_weights(hc_handle *h, int64_t *q);
int hc_get_filter_loglik(hc_handle *h, double *l);
int hc_get_filter_sm_theta(hc_handle *h, double *theta);

/* The well's record inside the window, particle filter (sequential importance sampling with delayed resampling): nothing
 * is resampled between two assimilation rows, so slot k is one trajectory over the whole window, and its importance weight
 * at the assimilation row is the product of the likelihoods of every observation that trajectory passed.  At chosen rows
 * before an assimilation row each member's water-table index is recorded when the row is solved, and at the assimilation
 * those indices join the member's weight as further well-type terms.  The mean of the products is still the unbiased
 * estimate of the window's marginal likelihood.  No state is stored, no row is solved twice, the step kernels are not
 * involved.  The counterpart of hc_set_enkf_window, with its rules.
 *   offsets [n_offsets] (<= 8, and n_offsets + n_sensors <= 8): rows before the assimilation row, integers in [1, stride),
 *   distinct; kept in ascending order.  For assimilation row r and offset o the lagged row r_j = r - o takes part when
 *   r_j >= 1, wtd_obs[r_j] >= 0 and r is an assimilation row, all as wtd_obs stands; otherwise it is absent on that
 *   assimilation, like a sensor without a value.
 *   Capture: a launch ends on every lagged row that takes part; then b_m(r_j) of every member -- the index wtd_out returns
 *   for that row -- goes into a device buffer [n_offsets][n_members] with rows [n_offsets] beside it (-1: none), which the
 *   assimilation empties.  A lagged row solved before hc_set_filter_window, or by another handle, is absent unless
 *   hc_set_filter_window_capture brought it.
 *   Weights at r with m_w >= 1 present lagged rows: the row takes the per-member path of hc_set_filter_soil_moisture, also
 *   when no sensor has a value (m_s = 0); fp64 without contraction:
 *     t_w = dz * (double)(b_m - o) / sigma_cm;  a = t_w * t_w;  the present sensors' u * u in record order, as there;
 *     then for each present lagged row by ascending offset:
 *     t_j = dz * (double)(b_m(r_j) - wtd_obs[r_j]) / sigma_cm;  a += t_j * t_j;  then l_m = -0.5 * a;
 *     a member whose index on r or on any present lagged row is >= D, or whose l_m is not finite, is not counted and gets
 *     q_m = 0.  s, e_m, q_m, the exact integer sums and the ESS, the draw (the same Philox counter), the scan, the fill and
 *     the gather, tempering (on l_m - s), the period accumulators' gather and the sensors' posterior moments run unchanged
 *     on that l_m.  R stays diagonal: correlated errors of the well's record are not modelled.
 *   The increment, in this order: s + log(W / count) - log(sigma_cm), - log(sigma_i) for each present sensor in record
 *     order, - log(sigma_cm) once for each present lagged row by ascending offset,
 *     - 0.5 * (double)(1 + m_s + m_w) * log(2 pi): the joint log-density of everything the window's trajectories passed
 *     (log cm^-(1 + m_w) (m^3/m^3)^-m_s).
 *   A row on which no lagged row takes part runs exactly the path it runs without a window: the bin path, or the sensor
 *   path.  The same bits at any launch length, point order or dealing of a sweep's points to handles or ranks.
 *   Window diagnostics, float64 [P][n_arow][n_offsets][4]: observed (0/1), observation dz * wtd_obs[r_j], forecast mean
 *   (sum / N_p) and std (two passes, / (N_p - 1), 0 for N_p = 1) of dz * (double)b_m(r_j) over the point's N_p members,
 *   every sum in the tile order of the sensor rows (cm from the top node; the host adds z[0] to the observation and the
 *   mean).  An offset absent on a row that has lagged rows: observed = 0, the rest NaN; a slot without any lagged row: NaN.
 * hc_set_filter_window: n_offsets = 0 turns it off: every bit, launch and allocation is then that of hc_set_filter.  Needs
 *   the particle filter on (hc_set_filter first); HC_ERR_ARG for an offset outside [1, stride), a repeated one, too many
 *   (hc_set_filter_soil_moisture refuses likewise when the sensors come second), while the EnKF is on, and while
 *   hc_set_filter_shard is set -- which is refused in turn while a window is set: the sharded filter gathers the indices
 *   of the assimilation row only.  Whatever turns the filter off removes the window (hc_set_filter included).
 *   (Re)creates the table (NaN) and empties the buffer.
 * hc_get/set_filter_window_stats: the table (P n_arow n_offsets 4 entries; checkpoints, the assembly of a sweep over ranks).
 * hc_get/set_filter_window_capture: b int32 [n_offsets][n_members] and rows [n_offsets], the lagged row each offset holds
 *   for the coming assimilation (-1: none; its indices read 0): what a checkpoint between a capture and its assimilation
 *   must carry.  Indices lie in [0, 65535] (HC_ERR_ARG else).
 * Test hooks of the last assimilation: hc_get_filter_window_width (m_w and, slots != NULL, the offsets' indices of the
 *   lagged columns in column order); hc_get_filter_loglik and hc_get_filter_member_weights keep returning l_m and q_m,
 *   also with a window and no soil-moisture record. */
int hc_set_filter_window(hc_handle *h, int32_t n_offsets, const int32_t *offsets);
int hc_get_filter_window_stats(hc_handle *h, double *table, int64_t n_entries);
int hc_set_filter_window_stats(hc_handle *h, const double *table, int64_t n_entries);
int hc_get_filter_window_capture(hc_handle *h, int32_t *b, int64_t *rows);
int hc_set_filter_window_capture(hc_handle *h, const int32_t *b, const int64_t *rows);
int hc_get_filter_window_width(hc_handle *h, int32_t *width, int32_t *slots);

/* Fixed-lag smoother of the water table by ancestry (Kitagawa 1996): the filter's own genealogy.  Every slot carries the
 * water-table indices of the member it descends from on the last K + 1 record rows; after a resampling the slots' values
 * for a record row K record rows back are a sample of p(water table there | the observations up to the present row).
 * This is the one table that describes the posterior: every other table of an assimilated run describes the forecast.
 * No state is stored, no row is solved twice, nothing is assumed Gaussian, the step kernels are not involved; the
 * quantity carried is the integer index wtd_out returns, so the tables are exact integers with the same bits at any
 * launch length, point order or dealing of a sweep's points to handles or ranks.
 *   Record rows: r >= 1 with r % stride == 0; n_srow = (n_forcing_rows - 1) / stride + 1, slot j <-> row j stride, slot 0
 *   stays empty.  lag = K record rows, 0 <= K <= HC_SMOOTHER_MAX_LAG.  The stride is independent of the filter's.
 *   The ring, per handle, K + 1 planes: ring_w uint16 [K + 1][N] (water-table indices), ring_id uint32 [K + 1][N] (the
 *   member's index within its point when the plane was recorded) and ring_row int64 [K + 1] (the forcing row a plane
 *   holds; -1: none).
 *   After each launch of hc_step_rows (launches end on assimilation rows and nothing is resampled inside one, so this is
 *   the same as processing the rows one by one), after every forecast table has accumulated and after the launch's
 *   assimilation, over the launch's record rows R in ascending order, j = R / stride:
 *     1. store: plane j mod (K + 1) takes b_m(R), the index wtd_out returns, and id = m - p N_p; its row becomes R.  If
 *        wtd_obs[R] < 0 the row is skipped: the plane's row becomes -1 instead.
 *     2. gather, if R is the launch's last row and the filter resampled on it: every plane with row >= 0, of both rings,
 *        goes through the row's ancestor table (slot m takes the values of anc[m]).  An assimilation row that is not a
 *        record row runs this step alone.
 *     3. emit plane (j - K) mod (K + 1), if j - K >= 1 and its row >= 0: shist[p][j - K][b] += the members of p whose
 *        plane value is b (a value >= D goes to no bin); spaths[p][j - K] = (distinct ids among the point's slots, R);
 *        then the plane's row becomes -1.
 *   K = 0 gives the analysis distribution of the row itself; K > 0 the distribution of row R - K stride conditioned on
 *   the observations up to R.  With flat weights the table equals hc_set_wtd_hist's on those rows and every path count
 *   is N_p.
 *   Path degeneracy: far enough back every slot descends from one member.  spaths reports it, as the number of distinct
 *   paths behind a row's histogram; towards 1 the histogram is one trajectory, not a distribution (take a shorter lag, or
 *   hold the ESS up with hc_set_filter_tempering).
 *   Tables: shist int32 [P][n_srow][D], at most HC_WTD_HIST_MAX_ENTRIES entries; spaths int64 [P][n_srow][2], (0, -1)
 *   until emitted.  Both are re-created and the ring emptied when the points, the forcing row count or the depth change.
 * hc_set_filter_smoother: stride 0 turns it off: nothing is then launched or allocated, and every bit is that of
 *   hc_set_filter alone.  Needs the particle filter on (hc_set_filter first); HC_ERR_ARG for a lag outside
 *   [0, HC_SMOOTHER_MAX_LAG], stride < 0, a table above the cap, while the EnKF is on and while hc_set_filter_shard is
 *   set -- which is refused in turn while the smoother is set: the exchanged columns do not carry the ring.  Whatever
 *   turns the filter off removes the smoother (hc_set_filter included).
 * hc_get_filter_smoother_layout: stride, lag, n_srow (zeros: off).
 * hc_get_filter_smoother_hist / hc_set_filter_smoother_hist_table, hc_get/set_filter_smoother_paths: the tables (P n_srow D
 *   and P n_srow 2 entries; checkpoints, the assembly of a sweep over ranks).
 * hc_get/set_filter_smoother_ring: w int32 [K + 1][N], id int64 [K + 1][N], rows [K + 1] and the last row stepped (what a
 *   flush conditions on; -1: none): what a checkpoint between a store and its emission must carry.  A plane without a row
 *   reads 0.  Indices lie in [0, 65535], ids in [0, N_p), a row is -1 or the record row of its plane (HC_ERR_ARG else).
 * hc_filter_smoother_flush: emits every pending plane, in ascending row order, each with the conditioning row it reached
 *   -- the last row stepped -- and empties it, so that further stepping counts nothing twice: spaths[..][1] - row is the
 *   lag a slot really got.
 * hc_reset_filter_smoother: the tables as created, the ring empty. */
#define HC_SMOOTHER_MAX_LAG 64
int hc_set_filter_smoother(hc_handle *h, int32_t stride, int32_t lag);
int hc_get_filter_smoother_layout(hc_handle *h, int32_t *stride, int32_t *lag, int64_t *n_srow);
int hc_get_filter_smoother_hist(hc_handle *h, int32_t *table, int64_t n_entries);
int hc_set_filter_smoother_hist_table(hc_handle *h, const int32_t *table, int64_t n_entries);
int hc_get_filter_smoother_paths(hc_handle *h, int64_t *table, int64_t n_entries);
int hc_set_filter_smoother_paths(hc_handle *h, const int64_t *table, int64_t n_entries);
int hc_get_filter_smoother_ring(hc_handle *h, int32_t *w, int64_t *id, int64_t *rows, int64_t *last_row);
int hc_set_filter_smoother_ring(hc_handle *h, const int32_t *w, const int64_t *id, const int64_t *rows, int64_t last_row);
int hc_filter_smoother_flush(hc_handle *h);
int hc_reset_filter_smoother(hc_handle *h);

/* Ensemble Kalman filter on the well's water table (stochastic EnKF: perturbed observations, Evensen 1994 / Burgers et al.
 * 1998).  It moves every member's psi by the sample covariance between psi and the observed quantity; noise is untouched.
 *   Analysis rows, launches and order: as for hc_set_filter -- r >= 1, r % stride == 0 and wtd_obs[r] >= 0 (as it stands
 *   when hc_step_rows reaches the row); slot j <-> row j stride, n_arow = (n_forcing_rows - 1) / stride + 1, slot 0 stays
 *   empty; a launch ends on every analysis row; spin-up solves are never analysed.  The row is solved, every table
 *   accumulates it (the FORECAST), then the analysis updates psi: psi_rows_out and wtd_out hold the forecast of the row,
 *   hc_get_state returns the ANALYSIS.
 *   Depths: z_i = i dz, measured from the top node (the C-ABI has no z[0]; only the two means of the diagnostics depend on
 *   it, and the host adds the well's z[0] to them).
 *   Observation operator, per member (a continuous water table): b = the member's find_wtd index (the index wtd_out returns);
 *     y = z[b-1] + dz * (psi_sat - psi[b-1]) / (psi[b] - psi[b-1])   if b >= 1 and psi[b-1] < psi_sat <= psi[b],
 *     y = z[b]                                                        otherwise,
 *   psi_sat of the member's point.  So y lies in (z[b-1], z[b]] and varies below one cell, where the reference's z[wtd_est]
 *   (src/simulation.py:612-615) is discrete: a deliberate deviation, the filter needs the spread the index cannot give.
 *   Perturbed observations: o = wtd_obs[r]; member k sees o_k = z[o] + sigma_cm eps_k, eps_k one standard normal of
 *   Philox4x32-10 under the EnKF seed at counter (0xFFFFFFFE, r, key_lo, key_hi), key = the member's GLOBAL id
 *   (member_offset + m; a sweep: the point's base + j), the first two output words (word 1 high) through the Box-Muller step
 *   of the noise (its cosine branch).  A noise counter's first word is a depth index / 2 and the particle filter's is
 *   0xFFFFFFFF: the three never meet.  eps_k depends on no launch length, member split or point order.
 *   Per point p (N_p members), fp64 without contraction:
 *     ybar, psibar_d = the member means; v = sum (y_k - ybar)^2 / (N_p - 1); c_d = sum (psi_dk - psibar_d)(y_k - ybar) / (N_p - 1)
 *     (two passes: means, then anomalies; N_p = 1: v = c = 0);
 *     rho_d = GC(|z_d - ybar| / L), the Gaspari-Cohn fifth-order taper with support 2 L (L = localisation_cm; L = 0: rho = 1);
 *     K_d = rho_d c_d / (v + sigma_cm^2);  psi_dk <- psi_dk + K_d (o_k - y_k) on all D nodes.
 *   A member whose updated column has a non-finite entry keeps its forecast and is counted as rejected.  Base noise
 *   vectors, noise scales and draw counters are not touched (no caller-noise path: Philox runs keep their in-kernel noise).
 *   Reproducibility: every sum over a point's members runs in an order fixed by N_p alone (tiles of 256 members in member
 *   order, then the tile partials by 1024 threads in tile-strided order and a fixed tree, for the columns and y alike), no
 *   floating-point atomics: the analysis is the same to the bit at any launch length, point order, dealing of a sweep's
 *   points to handles or ranks, and from run to run.
 *   Diagnostics, float64 [P][n_arow][8] per point and slot: count = N_p; prior mean ybar (cm from z[0]); prior std sqrt(v)
 *   (cm); innovation z[o] - ybar (cm); log-likelihood increment -0.5 log(2 pi (v + sigma^2)) - 0.5 (z[o] - ybar)^2 /
 *   (v + sigma^2) (log cm^-1, the particle filter's unit); posterior mean and std of y (the same operator and sums on the
 *   analysis states); rejected members.  Slots without an analysis hold count = 0 and NaN.  A point's log marginal
 *   likelihood is the sum of its increments in row order (on the host).
 * hc_set_enkf: stride 0 = off; otherwise (re)creates the table.  Needs column, forcing, members and noise source;
 *   sigma_cm finite and > 0; localisation_cm finite and >= 0; at most 2^32 - 1 rows.  HC_ERR_ARG while the particle filter
 *   is on (and hc_set_filter with a stride > 0 while the EnKF is on).  A later hc_set_column / hc_add_point /
 *   hc_set_point_member_bases, hc_set_members, hc_set_noise_host or hc_set_noise_philox turns it off; hc_set_forcing
 *   re-creates the table (count 0, NaN) when the row count changes.
 * hc_get/set_enkf_stats: the table (P n_arow 8 entries; checkpoints, the assembly of a sweep over ranks).
 * Test hooks of the last analysis: gain [P][D] (K_d), y [n_members] (the forecast y_k), eps [n_members]. */
int hc_set_enkf(hc_handle *h, int32_t stride, double sigma_cm, double localisation_cm, uint64_t seed);
int hc_get_enkf_stats(hc_handle *h, double *table, int64_t n_entries);
int hc_set_enkf_stats(hc_handle *h, const double *table, int64_t n_entries);
int hc_get_enkf_gain(hc_handle *h, double *gain);
int hc_get_enkf_y(hc_handle *h, double *y);
int hc_get_enkf_eps(hc_handle *h, double *eps);

/* Soil-moisture sensors in the EnKF analysis: a record of volumetric water content at n_sensors (<= 8) nodes joins the
 * well on the analysis rows of hc_set_enkf (the rows themselves do not change: r >= 1, r % stride == 0, wtd_obs[r] >= 0).
 *   values [n_forcing_rows][n_sensors] (m^3/m^3, in [0, 1]; NaN = no observation), nodes [n_sensors] in [0, D), sigma
 *   [n_sensors] the sensors' error standard deviations (finite, > 0).
 *   A row with no sensor value runs the m' = 1 case, the analysis of hc_set_enkf (an all-NaN record: the well-only run to
 *   the bit).  A row with m_s >= 1 sensor values runs one batch update per point of m' = 1 + m_s observations, in a fixed
 *   order: the well, then the present sensors in record order.
 *   Observations per member: Y_k = (y_k, theta_k[j_1], ...): y_k the water table of hc_set_enkf; theta_k[j] the cell model
 *   at node j on the forecast psi (the bits of hc_model_nodes' theta; theta has no noise term).
 *   Perturbed observations: o_k = (z[o] + sigma_cm eps_k, theta_obs,i + sigma_i eps_k,i); eps_k as for hc_set_enkf (counter
 *   (0xFFFFFFFE, r, key)); sensor i of the RECORD draws at counter (0xFFFFFFF0 + i, r, key_lo, key_hi) under the EnKF seed
 *   and the member's global id, through the same Box-Muller step, whether it is present on the row or not.  Noise
 *   counters (first word a depth index / 2), the particle filter's (0xFFFFFFFF) and these never meet.
 *   Per point p (N_p members), fp64 without contraction, two passes (means, then anomalies), /(N_p - 1) (N_p = 1: 0):
 *     Ybar, C_YY (m' x m'), C_psiY (D x m');
 *     taper (L = localisation_cm > 0; L = 0: rho = 1): rho_{d,i} = GC(|z_d - zeta_i| / L), rho_{i,i'} = GC(|zeta_i - zeta_i'|
 *     / L), zeta = ybar for the well and z[j_i] for a sensor;
 *     K = (rho o C_psiY)(rho o C_YY + R)^-1, R = diag(sigma_cm^2, sigma_i^2): a Cholesky factor of the m' x m' matrix in a
 *     fixed order (one thread per point), then per node a forward and a backward substitution; a pivot that is not finite
 *     and > 0 gives a NaN gain (every member then keeps its forecast and counts as rejected);
 *     psi_k <- psi_k + K (o_k - Y_k), the m' terms summed in i order; a member whose updated column has a non-finite entry
 *     keeps its forecast and is counted as rejected.
 *   Reproducibility: every member sum runs in tiles of 256 members in member order, then the tile partials by 1024 threads
 *   in tile-strided order and a fixed tree (the rule of hc_set_enkf, for every column), no floating-point atomics: the same
 *   bits at any launch length, point order, dealing of a sweep's points to handles or ranks.
 *   The EnKF's table on such a row: entries 0-3 and 5-7 keep their meaning (the well's y; the posterior from the analysis
 *   states); entry 4 is the JOINT Gaussian log-density of the observed vector under N(Ybar, C_YY + R), untapered, in
 *   log cm^-1 (m^3/m^3)^-m_s.
 *   Sensor diagnostics, float64 [P][n_arow][n_sensors][6]: observed (0/1), observation, prior mean and std of theta, posterior
 *   mean and std of theta (the analysis states, rejected members at their forecast).  A sensor without a value on an analysed
 *   row: observed = 0, the rest NaN; every entry of a slot without a joint analysis (none, or no sensor value on the row): NaN.
 * hc_set_enkf_soil_moisture: n_sensors = 0 removes the record; otherwise (re)creates the table (NaN).  Needs the EnKF on
 *   (hc_set_enkf first); HC_ERR_ARG while the particle filter is on.  Turned off by whatever turns the EnKF off (hc_set_enkf
 *   included).  hc_step_rows refuses while the record's row count differs from the forcing's.
 * hc_get/set_enkf_sm_stats: the sensor table (P n_arow n_sensors 6 entries; checkpoints, the assembly of a sweep over ranks).
 * Test hooks of the last analysis, when it had sensor values: hc_get_enkf_sm_width (m', 0: the last analysis had none),
 *   y [n_members][m'] (Y_k), gain [P][D][m'] (K), eps [n_members][n_sensors] (every sensor of the record).  On such a row
 *   hc_get_enkf_y / eps hold the well's y_k and eps_k, hc_get_enkf_gain the well's column of K. */
int hc_set_enkf_soil_moisture(hc_handle *h, int32_t n_sensors, const int32_t *nodes, const double *values,
                              const double *sigma);
int hc_get_enkf_sm_stats(hc_handle *h, double *table, int64_t n_entries);
int hc_set_enkf_sm_stats(hc_handle *h, const double *table, int64_t n_entries);
int hc_get_enkf_sm_width(hc_handle *h, int32_t *width);
int hc_get_enkf_sm_y(hc_handle *h, double *y);
int hc_get_enkf_sm_gain(hc_handle *h, double *gain);
int hc_get_enkf_sm_eps(hc_handle *h, double *eps);

/* The EnKF's analysis scheme and its relaxation to prior spread, for every analysis row of hc_set_enkf (well alone or
 * with sensors, m' = 1 + m_s).  Notation per point as above: N_p members, Ybar, the tapered cross-covariance row c_d =
 * (rho o C_psiY)_d, S = rho o C_YY + R = L L^T (the Cholesky factor of the gain), K_d = c_d S^-1, o = (z[o], theta_obs,i)
 * the UNPERTURBED observations, R^1/2 = diag(sigma_cm, sigma_i).
 *   method 0, stochastic: the perturbed-observation update of hc_set_enkf / hc_set_enkf_soil_moisture.
 *   method 1, square root (Whitaker & Hamill 2002, eq. 10, with the Cholesky factor as the square root of S): the mean
 *   moves by the Kalman gain, the anomalies by a reduced gain, nothing is drawn:
 *     dbar_d  = sum_i K_di (o_i - Ybar_i)                       (i in order)
 *     Kr_d    = c_d L^-T (L + R^1/2)^-1                         (the forward substitution of K_d, then a backward
 *                                                                substitution with the lower-triangular L + R^1/2)
 *     psi_dk <- psi_dk + dbar_d + sum_i Kr_di (Ybar_i - Y_ki)   (i in order)
 *   For m' = 1: Kr = K / (1 + sqrt(sigma^2 / s)).  No Philox counter is consumed: the analysis does not depend on the
 *   EnKF seed.  A failed factorisation gives NaN (K, Kr, dbar) and every member is rejected, as for method 0; the vote
 *   on a member's column (a non-finite entry: the forecast stays, counted as rejected) is the same.  The
 *   log-likelihood, the prior diagnostics and the rejection rule describe the forecast and do not change.
 *   relaxation = alpha in [0, 1] (RTPS, Whitaker & Hamill 2012), either method: after the update, per point and node d,
 *   over the columns the members kept,
 *     sigma_b_d, sigma_a_d = the sample std (N_p - 1) of psi_d before / after the update (two passes each: mean, then
 *                            squared anomalies; N_p = 1: 0; after the update the columns are summed relative to the
 *                            point's first member, so that a node on which every member agrees -- a saturated tail --
 *                            has sigma_a = 0 exactly and is left alone),
 *     f_d = 1 + alpha (sigma_b_d - sigma_a_d) / sigma_a_d   (f_d = 1 where sigma_a_d is 0 or not finite, where N_p = 1,
 *                                                            and for a point whose factorisation failed),
 *     psi_dk <- psibar_d + f_d (psi_dk - psibar_d), psibar_d the mean after the update; a node with f_d = 1 keeps its
 *     bits; a member whose relaxed column has a non-finite entry keeps its unrelaxed analysis (it is not counted as
 *     rejected).
 *   so that the node's std becomes (1 - alpha) sigma_a + alpha sigma_b.  The posterior entries of both tables (the
 *   EnKF's 5-7, the sensors' posterior mean and std) then describe the RELAXED ensemble.  Every sum follows the tile rule
 *   of hc_set_enkf (tiles of 256 members in member order, 1024 threads in tile-strided order, a fixed tree, no
 *   floating-point atomics, contraction off): the same bits at any launch length, point order or member split.
 *   With (0, 0), the state after hc_set_enkf, an analysis is that of hc_set_enkf to the bit and launches nothing more.
 * hc_set_enkf_method: needs the EnKF on (hc_set_enkf first); HC_ERR_ARG for another method, or a relaxation outside
 *   [0, 1] or not finite.  Reset to (0, 0) by whatever turns the EnKF off or re-creates it (hc_set_enkf included), like
 *   the sensor record.  hc_get_enkf_method: the two settings ((0, 0) while the EnKF is off).
 * Test hooks of the last analysis: hc_get_enkf_sqrt_gain [P][D][m'] (Kr) and hc_get_enkf_sqrt_shift [P][D] (dbar),
 *   HC_ERR_ARG unless it was a square-root analysis; hc_get_enkf_relaxation: sigma_b, sigma_a and f, [P][D] each,
 *   HC_ERR_ARG unless it relaxed.  hc_get_enkf_gain / hc_get_enkf_sm_gain keep returning K.  After a square-root
 *   analysis hc_get_enkf_eps / hc_get_enkf_sm_eps fail (HC_ERR_ARG), like a call before any analysis. */
int hc_set_enkf_method(hc_handle *h, int32_t method, double relaxation);
int hc_get_enkf_method(hc_handle *h, int32_t *method, double *relaxation);
int hc_get_enkf_sqrt_gain(hc_handle *h, double *gain);
int hc_get_enkf_sqrt_shift(hc_handle *h, double *shift);
int hc_get_enkf_relaxation(hc_handle *h, double *sigma_b, double *sigma_a, double *factor);

/* The noise field in the analysis (joint state-parameter estimation by state augmentation; Chen & Zhang 2006, Hendricks
 * Franssen & Kinzelbach 2008).  A member's base noise vector z [D] -- args_i["n_rnd"] of src/simulation.py:561,592, which
 * vrettas_fung.py:154,172,190 turns into K_bkg on every row but the refresh rows (src/simulation.py:599-601 replace it for
 * that one row) -- is the member's conductivity field.  With on = 1 every analysis updates it with the member's psi, from
 * the same observations, draws and m' x m' factor:
 *     zbar_d, c_d,i = sum_k (z_dk - zbar_d)(Y_ki - Ybar_i)          (the tile rule of hc_set_enkf over (z, Y))
 *     K^z_d = (rho_d o c_d / (N_p - 1)) S^-1                         (rho_d: node d at depth d dz, localisation_cm of
 *                                                                     hc_set_enkf; S = rho o C_YY + R and its factor are
 *                                                                     the state's to the bit)
 *     z_dk <- z_dk + sum_i K^z_d,i delta_ki, i in order              (delta: the member's innovations of its psi update;
 *                                                                     square root: the reduced gain, Ybar_i - Y_ki, and
 *                                                                     the shift sum_i K^z_d,i (o_i - Ybar_i))
 *   after the state's update (Y is still the forecast's).  A member whose psi analysis was rejected keeps its z to the
 *   bit and is not counted here; a member whose updated z would hold a non-finite entry keeps its old z, is counted in
 *   noise_rejected, and its psi update stands.  Then the anomalies of z are relaxed to prior spread with `relaxation` by
 *   the rule of hc_set_enkf_method (its sigma_a = 0 rule included; the members of either kind above are left alone); parameters regain no spread from the dynamics, so
 *   relaxation = 0 lets the field collapse over a long run.  All D entries are updated (a node that belongs to no layer
 *   never reads its z); the refresh rows' vectors are one-row draws and are not estimated.  Nothing is drawn, no step
 *   kernel is involved, and with on = 0 nothing is launched or allocated.
 *   Table (hc_get/set_enkf_noise_stats), float64 [P][n_arow][4 D + 1], NaN until the row is analysed: per node the prior
 *   mean and std of z_d, the mean and std after the relaxation ([4][D]), then noise_rejected.
 *   Noise source: with host noise the vectors are the caller's (hc_set_noise_host) updated in place, and
 *   hc_get_noise_base returns the analysed ones.  In a Philox run the step kernel keys its base vector by slot, so -- as
 *   with the particle filter -- the handle fills base and refresh vectors from philox_normal itself and runs the
 *   caller-noise path: hc_spinup and spin-up solves of hc_step_rows, and hc_set_noise_scale, are refused while it is on
 *   (set it after the spin-up; the base vectors carry the x0.8 damping), and hc_get/set_enkf_noise_base read and write
 *   the vectors [N][D] (a checkpoint; HC_ERR_ARG outside a Philox run with the field on).
 * hc_set_enkf_noise_field: needs the EnKF on; HC_ERR_ARG for on outside {0, 1}, a relaxation outside [0, 1] or not finite,
 *   or a sharded analysis (hc_set_enkf_shard refuses it in turn: the exchanged partials cover psi only).  Turned off by
 *   whatever turns the EnKF off or re-creates it.  hc_get_enkf_noise_field: (0, 0) while it is off.
 * Test hooks of the last analysis, [P][m'][D]: hc_get_enkf_noise_gain (K^z), hc_get_enkf_noise_sqrt_gain (the reduced
 *   gain) and hc_get_enkf_noise_sqrt_shift [P][D], the latter two HC_ERR_ARG unless it was a square-root analysis. */
int hc_set_enkf_noise_field(hc_handle *h, int32_t on, double relaxation);
int hc_get_enkf_noise_field(hc_handle *h, int32_t *on, double *relaxation);
int hc_get_enkf_noise_stats(hc_handle *h, double *table, int64_t n_entries);
int hc_set_enkf_noise_stats(hc_handle *h, const double *table, int64_t n_entries);
int hc_get_enkf_noise_gain(hc_handle *h, double *gain);
int hc_get_enkf_noise_sqrt_gain(hc_handle *h, double *gain);
int hc_get_enkf_noise_sqrt_shift(hc_handle *h, double *shift);
int hc_get_enkf_noise_base(hc_handle *h, double *base, int64_t first_member, int64_t count);
int hc_set_enkf_noise_base(hc_handle *h, const double *base);

/* The members' forcing state in the analysis (joint state and forcing-error estimation by state augmentation).  With
 * hc_set_forcing_perturbation every member carries g_{m,s} (s = 0 precipitation, 1 demand), an AR(1) over days whose
 * log-normal scales its record.  With on = 1 every analysis row r updates g of the day k = r / 48 the row lies in, after
 * psi (and after the noise field's vectors), from the same forecast Y [N][m'], observation errors, draws and factor:
 *     gbar_s, c_s,i = sum_k (g_ks - gbar_s)(Y_ki - Ybar_i)           (the tile rule of hc_set_enkf over (g, Y))
 *     K^g_s = (c_s / (N_p - 1)) S^-1                                  (NO taper on C_gY: g has no depth; S = rho o C_YY + R
 *                                                                      and its factor are the state's to the bit)
 *     g_ks <- g_ks + sum_i K^g_s,i delta_ki, i in order               (delta: the member's innovations of its psi update;
 *                                                                      square root: the reduced gain, Ybar_i - Y_ki, and
 *                                                                      the shift sum_i K^g_s,i (o_i - Ybar_i))
 *   A member whose psi analysis was rejected keeps its g to the bit; a member whose updated (g_0, g_1) would hold a
 *   non-finite entry keeps its old g and is counted as refused.  A stream with sigma_s = 0 is not written: its g keeps
 *   every bit (its factor is 1.0 regardless) and its table columns repeat the prior.  Then the anomalies are relaxed to
 *   prior spread with `relaxation`, by the noise field's rules.  Unlike the noise field g regains spread from its own
 *   recursion, so relaxation = 0 is a sound choice.  The analysed g is written into the carried state: the next launch
 *   starts inside day k from it, and g_{k+1} = (phi g_k) + (c xi_{k+1}) carries the update to every later day.  With a
 *   stride that is a multiple of 48 the analysis row is the first row of its day, so the covariance of g_k with y comes
 *   through phi from the day before (phi = 0: from that one row alone).  The work is done by the analysis's own kernels on
 *   the member-major copy x [N][2] of g (a pass with D = 2): sums over tiles of 256 members reduced in the fixed order, so
 *   the analysed g has the same bits at any launch length and point order.  No step kernel is involved; with on = 0
 *   nothing is launched or allocated.
 *   Table (hc_get/set_enkf_g_table), float64 [P][n_arow][9], NaN until the row is analysed: per stream s columns
 *   4 s + (prior mean, prior std, mean and std after the relaxation), then in column 8 the refused members.
 * hc_set_enkf_forcing: needs hc_set_enkf and hc_set_forcing_perturbation first; HC_ERR_ARG for on outside {0, 1}, a
 *   relaxation outside [0, 1] or not finite, the EnKF off, the perturbation off, or a sharded analysis (hc_set_enkf_shard
 *   refuses it in turn: the exchanged partials cover psi only).  Turned off by whatever turns the EnKF or the perturbation
 *   off or sets either again.  hc_get_enkf_forcing: (0, 0) while it is off.
 * Test hooks of the last analysis: hc_get_enkf_g_gain (K^g [P][m'][2]), hc_get_enkf_g_sqrt_gain (the reduced
 *   gain, [P][m'][2]) and hc_get_enkf_g_sqrt_shift [P][2], the latter two HC_ERR_ARG unless it was a square-root
 *   analysis, all three unless an analysis has run since hc_set_enkf_forcing.  g itself: hc_get_forcing_state. */
int hc_set_enkf_forcing(hc_handle *h, int32_t on, double relaxation);
int hc_get_enkf_forcing(hc_handle *h, int32_t *on, double *relaxation);
int hc_get_enkf_g_table(hc_handle *h, double *table, int64_t n_entries);
int hc_set_enkf_g_table(hc_handle *h, const double *table, int64_t n_entries);
int hc_get_enkf_g_gain(hc_handle *h, double *gain);
int hc_get_enkf_g_sqrt_gain(hc_handle *h, double *gain);
int hc_get_enkf_g_sqrt_shift(hc_handle *h, double *shift);

/* The well's record inside the window (asynchronous EnKF, Sakov, Evensen & Bertino 2010): at chosen rows before an
 * analysis row each member's y is recorded when the row is solved, and at the analysis those values join the batch as
 * further columns of Y, so that the members' present states are updated with the covariance between psi now and y then.
 * No state is stored, no row is solved twice, the step kernels are not involved.
 *   offsets [n_offsets] (<= 8, and n_offsets + n_sensors <= 8 so that m' <= 9): rows before the analysis row, integers in
 *   [1, stride), distinct; kept in ascending order.  For analysis row r and offset o the lagged row r_j = r - o takes
 *   part when r_j >= 1 and wtd_obs[r_j] >= 0 (the row was solved and has an observation); otherwise it is absent on that
 *   analysis, like a sensor without a value.
 *   Capture: a launch ends on every lagged row that takes part (and whose analysis row is one, as wtd_obs stands); then
 *   y_k of every member -- the operator and the bits of hc_set_enkf, hc_get_enkf_y on that row -- goes into a device
 *   buffer [n_offsets][n_members], which the analysis empties.  A lagged row solved before hc_set_enkf_window, or by
 *   another handle, is absent unless hc_set_enkf_window_capture brought it.
 *   Analysis at r: Y_k = (y_k, theta_k[j_1], ..., y_k(r_j1), ...), m' = 1 + m_s + m_w columns: the well at r, the present
 *   sensors in record order, the present lagged rows by ascending offset.  A lagged column is a well-type observation:
 *   o = z[wtd_obs[r_j]], error sigma_cm (R stays diagonal: correlated errors of the well's record are not modelled),
 *   zeta = z[wtd_obs[r_j]] -- its own observed depth -- in the taper of hc_set_enkf_soil_moisture, and in the stochastic
 *   scheme eps_k at counter (0xFFFFFFFE, r_j, key_lo, key_hi): the draw the well would have had on row r_j, which is never
 *   an analysis row (o < stride), so no draw is used twice.  The square-root scheme draws nothing.  Gain, reduced gain,
 *   update, the vote on a member's column, relaxation and the posterior diagnostics run as on any m'-wide row; the
 *   EnKF's entry 4 is the joint log-density of everything assimilated on the row (log cm^-(1 + m_w) (m^3/m^3)^-m_s).
 *   Moments, profiles and histograms keep describing the forecast.  The same bits at any launch length, point order or
 *   dealing of a sweep's points to handles or ranks.
 *   Window diagnostics, float64 [P][n_arow][n_offsets][4]: observed (0/1), observation z[wtd_obs[r_j]], prior mean and std
 *   of the recorded y (cm from the top node; the host adds z[0] to the first two).  An offset absent on an analysis with
 *   lagged rows: observed = 0, the rest NaN; every entry of a slot whose analysis had no lagged row: NaN.
 * hc_set_enkf_window: n_offsets = 0 turns it off: analyses, launches and tables are then those of hc_set_enkf to the bit.
 *   Needs the EnKF on (hc_set_enkf first); HC_ERR_ARG for an offset outside [1, stride), a repeated one, or too many
 *   (hc_set_enkf_soil_moisture refuses likewise when the sensors come second).  Turned off by whatever turns the EnKF off
 *   (hc_set_enkf included).  (Re)creates the table (NaN) and empties the buffer.
 * hc_get/set_enkf_window_stats: the table (P n_arow n_offsets 4 entries; checkpoints, the assembly of a sweep over ranks).
 * hc_get/set_enkf_window_capture: y [n_offsets][n_members] and rows [n_offsets], the lagged row each offset holds for the
 *   coming analysis (-1: none; its y reads 0): what a checkpoint between a capture and its analysis must carry.
 * Test hooks of the last analysis: hc_get_enkf_width (m', 0: none yet); hc_get_enkf_window_width (m_w and, slots != NULL,
 *   the offsets' indices of the lagged columns in column order); when m_w > 0: y [n_members][m_w], eps [n_members][m_w]
 *   (HC_ERR_ARG after a square-root analysis); hc_get_enkf_window_gain: K [P][D][m'], every column, on any analysed row.
 *   hc_get_enkf_y / eps / gain and the hc_get_enkf_sm_* hooks keep returning the well's and the sensors' columns. */
int hc_set_enkf_window(hc_handle *h, int32_t n_offsets, const int32_t *offsets);
int hc_get_enkf_window_stats(hc_handle *h, double *table, int64_t n_entries);
int hc_set_enkf_window_stats(hc_handle *h, const double *table, int64_t n_entries);
int hc_get_enkf_window_capture(hc_handle *h, double *y, int64_t *rows);
int hc_set_enkf_window_capture(hc_handle *h, const double *y, const int64_t *rows);
int hc_get_enkf_width(hc_handle *h, int32_t *width);
int hc_get_enkf_window_width(hc_handle *h, int32_t *width, int32_t *slots);
int hc_get_enkf_window_y(hc_handle *h, double *y);
int hc_get_enkf_window_eps(hc_handle *h, double *eps);
int hc_get_enkf_window_gain(hc_handle *h, double *gain);

/* One point's members on several handles (a single-point ensemble over several GPUs): the handle holds members
 * [first_global, first_global + n_members) of a point with n_global members, and its analyses are those of the one handle
 * that holds them all, to the bit.  Every sum over the members is formed as partials of tiles of 256 consecutive members
 * in member order and reduced in an order fixed by the tile count alone; a shard that starts on a tile boundary forms
 * exactly the partials the whole ensemble would have formed for its tiles, so the shards only have to gather them.
 *   Before each of the analysis's reductions -- the prior sums, the prior products, the squared prior anomalies, the
 *   analysis columns' sums and their squared anomalies (relaxation only), the posterior sums and products -- the handle
 *   writes its tiles' partials at their place in the global layout [n_tiles_global][columns] of the pass inside
 *   device_buf, drains its stream and calls fn(ctx, pass, n_words, first_word, count_words): `pass` points into device_buf
 *   at the pass's layout of n_words doubles, of which [first_word, first_word + count_words) are this handle's.  On
 *   return (0 = ok) every other handle's words must be in place and visible on the device: a gather (copy), never
 *   arithmetic.  The reduction then runs over all n_tiles_global tiles on every handle alike, so sums, gains and every
 *   diagnostics table (EnKF, sensors, window) are identical on all of them.  Every mean and variance divides by n_global
 *   or n_global - 1.  The relaxation's spread is summed relative to the point's first member: the handle with
 *   first_global = 0 contributes that member's analysis column (one more call of fn: n_words = D, its count_words = D,
 *   everyone else's 0).  All handles of a point must analyse the same rows with the same settings, or the calls do not
 *   pair up.  A non-zero return of fn fails hc_step_rows with HC_ERR_DEVICE (the states are then unusable).
 *   The draws of the stochastic scheme are keyed by first_global + m; with hc_set_noise_philox its member_offset must
 *   equal first_global (HC_ERR_ARG), so that the model noise is the whole ensemble's too.  The window's capture stays
 *   per handle (only the handle's own members' y).  The test hooks return the handle's own members for y / eps and the
 *   same gains on every handle; the count entry of the EnKF's table is n_global.
 * hc_get_enkf_shard_words: what device_buf must hold for n_global members, in doubles: the global tile count times the
 *   widest pass as the sensors and the window stand (the prior products [D + m'][m'] plus the squared anomalies [D] that
 *   travel with them under relaxation, or the posterior's), and at least D.  Set the sensors and the window first: an
 *   analysis that finds the buffer too small fails with HC_ERR_ARG.
 * hc_set_enkf_shard: device_buf is caller-owned memory on the handle's device (the idiom of hc_export_moments), alive
 *   while the shard is set.  Needs the EnKF on; HC_ERR_ARG for more than one point on the handle, first_global % 256 != 0,
 *   n_members % 256 != 0 on a shard that is not the last (first_global + n_members < n_global), first_global + n_members >
 *   n_global, n_words < hc_get_enkf_shard_words, a NULL buffer or callback.  n_global = 0 turns sharding off; so does
 *   whatever turns the EnKF off.  With sharding off nothing changes: no launch, no synchronisation, the same kernels.
 *   n_global = n_members with first_global = 0 and a callback that does nothing gives the unsharded bits.
 * hc_get_enkf_shard: n_global (0: off) and first_global. */
typedef int (*hc_enkf_exchange_fn)(void *ctx, void *device_buf, int64_t n_words, int64_t first_word, int64_t count_words);
int hc_get_enkf_shard_words(hc_handle *h, int64_t n_global, int64_t *n_words);
int hc_set_enkf_shard(hc_handle *h, int64_t n_global, int64_t first_global, void *device_buf, int64_t n_words,
                      hc_enkf_exchange_fn fn, void *ctx);
int hc_get_enkf_shard(hc_handle *h, int64_t *n_global, int64_t *first_global);

/* One point's members on several handles, particle filter: the handle is shard `index` of n_shards and holds members
 * [b_index, b_index+1) of a point with n_global = b_S members, bounds b_0 = 0 < b_1 < ... < b_S (any bounds: no alignment,
 * a shard of one member is legal).  The handles' assimilations together are the assimilation of the one handle that
 * holds every member, to the bit: states, base noise vectors, the diagnostics table, weights, draw and ancestry.
 * Everything the ancestry depends on is an integer function of the members' water-table indices on the row, and
 * systematic resampling is monotone -- the ancestor of slot k is non-decreasing in k -- so a shard's slots need an
 * ordered run of ancestors, and two shards' runs share at most one member.
 *   Order at an assimilation row, after the row is solved and the tables have accumulated the forecast:
 *   1. the handle writes its members' water-table indices as 8-byte integers at words [b_index, b_index+1) of device_buf,
 *      drains its stream and calls gather(ctx, device_buf, n_global, b_index, n_members); on return (0 = ok) every other
 *      handle's words must be in place and visible on the device (a copy);
 *   2. the kernels of hc_set_filter run over the gathered vector with N_p = n_global; the draw's key is the point's first
 *      global member id (hc_set_noise_philox: member_offset - b_index = 0; host noise: member_offset as it stands).  Every
 *      handle obtains the same q_b, Q, r, diagnostics row (count = n_global) and ancestor table anc[n_global];
 *   3. from anc and the bounds alone the handle derives, per other shard s, the members it receives from s -- the distinct
 *      ancestors of its own slots that lie in [b_s, b_s+1), ascending -- and the members it sends to s -- the distinct
 *      ancestors of s's slots that lie in its own range, ascending; both ends derive the same lists, none travels.  It
 *      packs, per destination in shard order and per listed member, psi[D] then the base noise vector [D] (2 D words)
 *      into the send region, drains its stream and calls route(ctx, send, send_words, recv, recv_words): send_words[s] /
 *      recv_words[s] = the 8-byte words for / from shard s (0 for s = index), the blocks contiguous in shard order from
 *      `send` / `recv` (both inside device_buf).  On return (0 = ok) the block of every source must be in the receive
 *      region and visible on the device (a copy: the words are bit patterns);
 *   4. slot k takes psi and base from the handle's own member anc[k] - b_index, or from the receive region.
 *   Both callbacks are called once per assimilation on every handle, also when nothing is routed (equal weights, Q = 0:
 *   the ancestry is the identity), so the handles' calls pair up.  All handles of a point must assimilate the same rows
 *   with the same settings.  A non-zero return of either callback fails hc_step_rows with HC_ERR_DEVICE (the states are
 *   then unusable).  No floating-point arithmetic on this path.  A soil-moisture record (hc_set_filter_soil_moisture) and sharding
 *   exclude each other: only water-table indices are gathered; a sweep's points are dealt whole.
 * hc_get_filter_shard_words: what device_buf must hold, in 8-byte words: the index vector n_global, the send region
 *   (n_members + n_shards - 1) 2 D and the receive region n_members 2 D (monotonicity bounds both).
 * hc_set_filter_shard: device_buf is caller-owned memory on the handle's device, alive while the shard is set.  Needs the
 *   particle filter on; HC_ERR_ARG for more than one point on the handle, bounds that do not start at 0 or do not increase
 *   strictly, index outside [0, n_shards), n_members != b_index+1 - b_index, n_global > 2^31 - 1, in a Philox run
 *   member_offset != b_index (the model noise and the base vectors must be the whole ensemble's), a NULL buffer or
 *   callback, n_words < hc_get_filter_shard_words.  A refused call leaves sharding off.  n_shards = 0 turns sharding off;
 *   so does whatever turns the filter off, hc_set_filter itself included.  With sharding off nothing changes: the same
 *   kernels and launches, no synchronisation.  n_shards = 1 with callbacks that do nothing gives the unsharded bits.
 * hc_get_filter_shard: n_shards (0: off), index and n_global.
 * While sharded, hc_get_filter_ancestors returns the GLOBAL member id of the ancestor of each of the handle's own slots
 *   ([n_members]); weights and draw are the same on every handle. */
typedef int (*hc_filter_route_fn)(void *ctx, void *send, const int64_t *send_words, void *recv, const int64_t *recv_words);
int hc_get_filter_shard_words(hc_handle *h, int32_t n_shards, const int64_t *bounds, int32_t index, int64_t *n_words);
int hc_set_filter_shard(hc_handle *h, int32_t n_shards, const int64_t *bounds, int32_t index, void *device_buf,
                        int64_t n_words, hc_enkf_exchange_fn gather, hc_filter_route_fn route, void *ctx);
int hc_get_filter_shard(hc_handle *h, int32_t *n_shards, int32_t *index, int64_t *n_global);

/* The path's one collective inside the library, for a single process that drives several devices with
 * one handle each: every handle's moment table is replaced by the sum over all n handles (ncclAllReduce, ncclInt64,
 * ncclSum over RCCL / xGMI, in place on device memory, on the handles' own streams).  Integer sums: the result does not
 * depend on the number of devices.  RCCL is bound at run time (dlopen); HC_ERR_UNSUPPORTED when it is not loadable.
 * One process per GPU (torch.distributed) callers use hc_export_moments + their own all-reduce instead. */
int hc_allreduce_moments(hc_handle **handles, int n);

/* Bit-exact resume of a Philox ensemble (the reference's single-column analogue is IC_Filename,
 * src/simulation.py:358-385): besides the state (hc_get_state / hc_set_state), the moment table (hc_get_moments /
 * hc_set_moments) and the next row, a stopped ensemble is defined by the damping every member's base noise vector has
 * collected from failed attempts, scale[member] = 0.8^k (src/richards_pde.py:522 applied to the base vector).
 * hc_set_noise_scale must follow hc_set_noise_philox (which resets the scales to 1); values must lie in (0, 1]. */
int hc_get_noise_scale(hc_handle *h, double *scale, int64_t first_member, int64_t count);
int hc_set_noise_scale(hc_handle *h, const double *scale, int64_t first_member, int64_t count);

/* Several parameter points in one handle: base[k] = global id of point k's first member, i.e. the Philox stream of
 * member j of point k is keyed by base[k] + j.  Default (and base = NULL): member_offset + k * members_per_point, the
 * points of this handle are consecutive points of the sweep.  A rank that is dealt non-consecutive points (round-robin
 * by cost) sets the bases so that a point's realisations do not depend on who runs it. */
int hc_set_point_member_bases(hc_handle *h, const int64_t *base);
/* cost[n_points]: RHS evaluations spent on each point's members by hc_step_rows since the points were installed (zeros
 * for a single point).  The library walks the points costliest-first from the second launch on (the order changes
 * no result; HYDROCOL_POINT_ORDER=fixed in the environment at hc_create keeps point order). */
int hc_get_point_costs(hc_handle *h, uint64_t *cost);

/* Test hooks -------------------------------------------------------------------------- */
/* dydt for every member's current state on forcing row `row` (noise = base vectors).
 * aux (nullable): [n_members][3*(D-1)+1] = c | s | f at the midpoints, then pL.
 * diag (nullable): [n_members][2] = transpiration, lateral flow of this one evaluation -- the two integrals a stepped row
 * reports for its last evaluation (hc_step_args.diag_out); asking for them changes no other output.
 *
 * The device function behind all of it, rhs_eval, exists in two instantiations.  The plain one (ONE_BALLOT = false) is what
 * the step kernels of one wave per SIMD run: 2, 3, 8, 9, 10 cells per lane, generic exponents from 7 cells.  The step
 * kernels of the two-waves-per-SIMD layout (two_of in csrc/hc_step.h: default exponents at 4 ... 7 cells per lane, generic
 * exponents at 4 ... 6, the split column) run the other one (ONE_BALLOT = true): the same values by a shorter
 * instruction sequence, every shortcut of which claims equal bits.  `variant` selects what is evaluated:
 *   HC_RHS_HOOK         the plain instantiation.  A split column is evaluated by its two-wavefront kernel when aux is
 *                       NULL and by the one-wave kernel of its depth when aux is requested.
 *   HC_RHS_AS_STEPPED   what the handle's step kernel runs: its instantiation on its wave layout (a split column on two
 *                       wavefronts, with or without aux).  Where two_of is false this is HC_RHS_HOOK's kernel.
 *   HC_RHS_HOOK_LAYOUT  the plain instantiation on the step kernel's wave layout: HC_RHS_HOOK except that a split column
 *                       stays on two wavefronts when aux is requested (the partner of HC_RHS_AS_STEPPED in a bit-for-bit
 *                       comparison of aux there).
 * hc_rhs(h, row, spinup, dydt, aux) is hc_rhs_ex(h, row, spinup, HC_RHS_HOOK, dydt, aux, NULL). */
enum { HC_RHS_HOOK = 0, HC_RHS_AS_STEPPED = 1, HC_RHS_HOOK_LAYOUT = 2 };
int hc_rhs(hc_handle *h, int64_t row, int32_t spinup, double *dydt, double *aux);
int hc_rhs_ex(hc_handle *h, int64_t row, int32_t spinup, int32_t variant, double *dydt, double *aux, double *diag);
/* plugin call on the nodes for every member's current state: out [4][n_members][D]
 * = theta, K, C, K_bkg; qinf [n_members] (nullable) */
int hc_model_nodes(hc_handle *h, double *out, double *qinf);

/* Stateless plugin call (needs a device, no handle): psi [n_cells][n_cols] depth-major as the reference's
 * [dim_d x dim_m]; por / meank / noisec / n_rnd [n_cells] = porosity, layer-mean K (0 -> 1e-7, src/utilities.py:50),
 * noise coefficient (0.05 / 0.10 / 1.0, -1 = cell in no layer) and N(0,1) value of every cell.
 * out [4][n_cells][n_cols] = theta, K, C, K_bkg; qinf [n_cols] = q_inf_max from row 0 (src/models/vrettas_fung.py:254).
 * Only model, theta_res, alpha, n, m, psi_sat, epsilon, lambda_exp, sigma_noise, sat_soil and dz of `p` are read. */
int hc_plugin_eval(int device_ordinal, const hc_column_params *p, int64_t n_cells, int64_t n_cols,
                   const double *psi, const double *por, const double *meank, const double *noisec,
                   const double *n_rnd, double *out, double *qinf);

#ifdef __cplusplus
}
#endif
#endif
