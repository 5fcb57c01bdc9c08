"""Command line of the reference (``/root/reference/code/berkeley_hydro_main.py``), GPU-backed.

    python3 berkeley_hydro_main.py --params P.json [--data D.csv] [--seed S] [--device K] [--gpus N]

Same 12 required JSON keys (:40-43), same header-less 4-column CSV (:115-116), same messages and
exit codes (any error -> message + exit status 1, :138-142).  Additions (the reference tolerates
unknown keys, only membership of the 12 is checked):

* ``--seed`` / JSON ``"Seed"``: seeds ``Simulation(name, seed)``; the reference's CLI cannot be seeded.
* JSON ``"Ensemble": {"Members": N, "Seed": s, "Days": d, "Noise": "philox"|"numpy", "Spinup": "shared"|"member"}``:
  run N stochastic members (in-kernel Philox noise, or the reference's NumPy streams with member 0 on
  ``SeedSequence(seed)`` and member k on ``spawn_key=(k,)``; one shared spin-up or one per member) and write the
  per-row water-table mean / sigma to ``<Output_Name>_ensemble.h5``.
* ``"Ensemble": {..., "Points": [{"Soil_Properties": {"n": 1.7, "a0": 0.012}}, {...}, ...]}``: a parameter sweep
  (BASELINE config 5) -- every entry is merged over the file's own sections to give one parameter point; all points run
  with ``Members`` realisations each in ONE launch per batch of rows, each from its own spin-up, and the output holds
  ``moments [P][3][T]``, ``wtd_mean_cm`` / ``wtd_std_cm [P][T]`` and ``initial_cond [P][D]``.
* ``--gpus N`` / ``"Ensemble": {"GPUs": N}``: one process per GPU (``multigpu.py``).  The command starts its N ranks itself
  (children of ``torch.distributed.run`` on 127.0.0.1) before it touches a GPU; ensemble members shard by contiguous
  blocks, sweep points are dealt round-robin, nothing is exchanged while stepping, ONE all-reduce ends the run (the int64
  moment table over RCCL; for a sweep also the per-point initial conditions) and rank 0 writes
  ``<Output_Name>_ensemble.h5`` once -- the reference's single ``sim.run(); sim.saveResults()``
  (``berkeley_hydro_main.py:128-137``), bit-identical at any N.
* ``"Ensemble": {..., "Profiles": 48}``: ensemble profile statistics reduced on the GPU -- every 48th forcing row (1 = every
  row, as the reference stores them) the mean / sigma over the members of ``theta_vol``, ``psi_press`` and ``S_eff``
  ``[T_out][D]``, and for every solved row those of ``transpiration`` / ``lateral_flow`` and ``abs_error_mean`` ``[T]``
  (simulation.py:658-671; ``<key>_mean`` / ``<key>_std``, with ``profile_rows`` and ``profile_count``), added to
  ``<Output_Name>_ensemble.h5`` (a sweep: a leading ``[P]`` axis).  The integer tables are all-reduced with the moments.
* ``"Ensemble": {..., "Profiles": 48, "Profile_Distribution": {"Bins": 128, "Quantiles": [0.05, 0.5, 0.95]}}``: the members'
  ``theta_vol`` counted per node on the GPU on the profile rows (include/hydrocol.h hc_set_theta_hist) -- an exact integer
  histogram over ``Bins`` (32, 64 or 128; default 128) equal bins of [0, 1], summed over the ranks like the moments -- and
  from it the quantile bands of theta(z): per level, row and node the centre of the first bin whose cumulative count
  reaches the level's rank (``Quantiles``, required: as ``Distribution.Quantiles``, at most 16, the same rank rule).  Needs
  ``"Profiles"`` >= 1.  Added to ``<Output_Name>_ensemble.h5``: ``theta_hist`` ``[T_out][D][B]`` int32,
  ``theta_hist_rows``, ``theta_hist_count``, ``theta_hist_bins``, ``theta_hist_outside`` (values that were NaN or outside
  [0, 1]: none in a sound run), ``theta_quantile_levels`` and ``theta_quantile`` ``[T_out][L][D]`` (a sweep: a leading
  ``[P]`` axis), and the run ends with the line `` [Ensemble xN] theta bands: L levels on R rows, B bins``.
* ``"Ensemble": {..., "Profiles": 48, "Storage": {"Layers_cm": [[0, 100], [100, 300]], "Bins": 128, "Quantiles": [0.05,
  0.5, 0.95]}}``: the water each depth layer stores, in cm, reduced per member on the GPU on the profile rows
  (include/hydrocol.h hc_set_layer_storage): S = dz sum theta_vol over the nodes with top <= z < bottom (at most 8 layers,
  which may overlap; each must hold a node), then the ensemble's mean and sigma from exact integer sums -- the nodes of a
  column covary, so neither follows from the per-node profile statistics.  ``Bins`` (optional: a power of two in 32 .. 1024)
  adds the histogram of each layer's mean theta and, with ``Quantiles`` (optional, default 0.05, 0.25, 0.5, 0.75, 0.95;
  at most 16, the rank rule of ``Distribution.Quantiles``), the quantile bands in cm; ``Quantiles`` without ``Bins`` is
  refused.  Needs ``"Profiles"`` >= 1.  The tables are summed over the ranks like the moments.  Added to
  ``<Output_Name>_ensemble.h5``: ``storage_layers_cm``, ``storage_nodes`` ``[L][2]``, ``storage_rows``, ``storage_count``,
  ``storage_mean_cm``, ``storage_std_cm`` ``[T_out][L]``, ``storage_overflow`` (values the quantisation clamped or that
  were NaN: none in a sound run) and, with ``Bins``, ``storage_hist`` ``[T_out][L][B]`` int32,
  ``storage_hist_bins``, ``storage_hist_outside``, ``storage_quantile_levels`` and ``storage_quantile_cm``
  ``[T_out][Lv][L]`` (a sweep: a leading ``[P]`` axis on the per-row datasets), and the run ends with the line
  `` [Ensemble xN] storage: L layers on R rows``.
* ``"Ensemble": {..., "Profiles": 48, "Conductivity": true}`` or ``"Conductivity": {"Layers_cm": [[0, 100], [100, 300]]}``:
  the two conductivities the reference reports per saved row (``K_hrc``, ``K_bkg``, simulation.py:661-665), over the
  members, reduced on the GPU on the profile rows (include/hydrocol.h hc_set_conductivity_stats).  Every member's K at
  every node is the cell model's with the noise vector its row was solved with; the statistics are taken on ln K -- K is
  log-normal by construction and spans decades down an unsaturated column -- from exact integer sums: mean and sigma of
  ln K and the geometric mean K = exp(mean), in cm per row.  A K that is not finite and > 0 (K_hrc is exactly 0 where theta
  sits at theta_res) is left out, which the per-node counts show.  ``Layers_cm`` (optional; at most 8 layers, which may
  overlap; each must hold a node and less than 4096 cm) adds each layer's effective vertical conductivity
  K_eff = n / sum 1 / K_hrc, reduced per member before the members are.  Needs ``"Profiles"`` >= 1; ``false`` is the same as
  no key.  While it is on a launch ends on every profile row; the members' states do not depend on it.  The table is
  summed over the ranks like the profile statistics; with a filter or an EnKF it describes the forecast.  Added to
  ``<Output_Name>_ensemble.h5``: ``conductivity_rows``, ``conductivity_count`` ``[T_out][D][2]``, ``lnK_hrc_mean``,
  ``lnK_hrc_std``, ``K_hrc_geomean``, ``lnK_bkg_mean``, ``lnK_bkg_std``, ``K_bkg_geomean`` ``[T_out][D]``,
  ``conductivity_overflow`` and, with layers, ``K_eff_layers_cm``, ``K_eff_nodes`` ``[L][2]``, ``K_eff_count``,
  ``lnK_eff_mean``, ``lnK_eff_std``, ``K_eff_geomean`` ``[T_out][L]`` (a sweep: a leading ``[P]`` axis on the per-row
  datasets), and the run ends with the line `` [Ensemble xN] conductivity: D nodes and L layers on R rows``.
* ``"Ensemble": {..., "Profiles": 48, "Covariance": {"Node_Stride": 4, "Sensor_Sigma": 0.02}}``: how the nodes of a
  column and the water table move together, from exact integer second moments accumulated on the GPU on the profile rows
  (include/hydrocol.h hc_set_theta_cov): theta_vol at every ``Node_Stride``-th node (default 1) quantised to 2^-20 and the
  members' water-table index, their sums and sums of products over the members -- every other table is a marginal.  From
  them the covariance of theta(z), its covariance and correlation with the water table and, with ``Sensor_Sigma``
  (optional: a probe's error in m3/m3, > 0), the fraction of the water table's variance one probe at each node would
  remove in a linear update, cov(theta_i, wtd)^2 / ((var theta_i + sigma^2) var wtd).  Needs ``"Profiles"`` >= 1; a
  ``theta_cov`` dataset above 2 GiB is refused (take a larger node stride or a larger profile stride).  The table is summed
  over the ranks like the profile statistics; with a filter or an EnKF it describes the forecast.  Added to
  ``<Output_Name>_ensemble.h5``: ``theta_cov_node_stride``, ``theta_cov_nodes``, ``theta_cov_depth_cm`` ``[n]``,
  ``theta_cov_rows``, ``theta_cov_count``, ``theta_cov_outside`` (members with a theta that was NaN or outside [0, 1]: none
  in a sound run), ``theta_cov`` ``[T_out][n][n]``, ``wtd_theta_cov_cm`` ``[T_out][n]``, ``wtd_var_cm2`` ``[T_out]``,
  ``theta_wtd_corr`` ``[T_out][n]`` and, with ``Sensor_Sigma``, ``theta_sensor_sigma`` and ``theta_sensor_gain``
  ``[T_out][n]`` (a sweep: a leading ``[P]`` axis on the per-row datasets), and the run ends with the line
  `` [Ensemble xN] covariance: n nodes on R rows``.
* ``"Ensemble": {..., "Periods": {"Rows": 1440, "Shallower_than_cm": [100, 200], "Bins": 128, "Transpiration_max_cm": 16,
  "Lateral_flow_max_cm": 4, "Quantiles": [0.05, 0.5, 0.95]}}``: period totals per member, reduced on the GPU at the end of
  every period (include/hydrocol.h hc_set_period_totals): each member's transpiration and lateral flow summed over the
  period's solved rows, its shallowest and deepest water table and the rows on which the water table stood at or above
  each depth of ``Shallower_than_cm`` (optional, at most 4, mapped to the first node at or below the depth), then the
  ensemble's mean and sigma from exact integer sums -- a member's rows are correlated in time, so none of these follows
  from the per-row tables.  Exactly one of ``Rows`` (a period every so many rows, 1 .. 2^20) and ``Calendar``
  (``"month"`` or ``"year"``: a period ends on the last row of each calendar month or year of the record's Datenum).
  ``Bins`` (optional: a power of two in 32 .. 1024) adds histograms of the flux totals over [0, max) cm
  (``Transpiration_max_cm``, default 16, and ``Lateral_flow_max_cm``, default 4: powers of two in 2^-8 .. 2^12) and of both
  extremes over the depth grid and, with ``Quantiles`` (optional, default 0.05, 0.25, 0.5, 0.75, 0.95; at most 16, the
  rank rule of ``Distribution.Quantiles``), their quantiles; the three keys need ``Bins``.  Periods that end after the
  run's last row are dropped.  Needs no ``"Profiles"``.  Refused with ``"Filter": {"Sharded": true}`` on a single-point
  run (the routed columns do not carry the members' accumulators).  The tables are summed over the ranks like the
  moments.  Added to ``<Output_Name>_ensemble.h5``: ``period_end_rows``, ``period_solved_rows``, ``period_count``,
  ``period_{transpiration,lateral_flow,wtd_shallowest,wtd_deepest}_{mean,std}_cm`` ``[n_period]``,
  ``period_thresholds_cm``, ``period_threshold_nodes``, ``period_below_rows_{mean,std}`` and
  ``period_below_fraction_mean`` ``[n_period][n_thresholds]``, ``period_overflow`` and, with ``Bins``,
  ``period_hist_flux`` ``[n_period][2][B]`` and ``period_hist_wtd`` ``[n_period][2][D]`` int32, ``period_hist_outside``,
  ``period_quantile_levels`` and ``period_{transpiration,lateral_flow,wtd_shallowest,wtd_deepest}_quantile_cm``
  ``[n_period][Lv]`` (a sweep: a leading ``[P]`` axis on the per-period statistics), and the run ends with the line
  `` [Ensemble xN] periods: R periods, K quantities``.
* ``"Periods": {..., "Uptake": {"Layers_cm": [[0, 100], [100, 300], [300, 1500]], "Bins": 128, "Quantiles": [0.05, 0.5,
  0.95]}}``: root-water uptake by depth over the same periods (include/hydrocol.h hc_set_root_uptake): each member's uptake
  of every solved daylight row, evaluated on the GPU from the row's end state, totalled over the period for the whole
  column and for 1 to 8 depth layers (a midpoint belongs to a layer when top <= z + dz / 2 < bottom), reduced over the
  members at the period's end, and the period's uptake at every midpoint.  ``Bins`` (optional) adds histograms of each
  layer's share of a member's total and ``Quantiles`` (default 0.05, 0.5, 0.95; needs ``Bins``) their quantiles.  Refused
  before any GPU call: a non-object, an unknown key, more than 8 layers, a layer that holds no root cell, ``Quantiles``
  without ``Bins``, ``Simulation_Flags.ET`` off.  Added to the file: ``uptake_layers_cm``, ``uptake_cells``,
  ``uptake_depth_cm`` ``[D-1]``, ``uptake_count``, ``uptake_total_{mean,std}_cm`` ``[n_period]``,
  ``uptake_layer_{mean,std}_cm`` and ``uptake_share_of_mean`` ``[n_period][L]``, ``uptake_profile`` ``[n_period][D-1]``,
  ``uptake_depth_quantile_cm`` ``[n_period][2]``, ``uptake_overflow`` and, with ``Bins``, ``uptake_share_hist``
  ``[n_period][L][B]`` int32, ``uptake_hist_outside``, ``uptake_quantile_levels`` and ``uptake_share_quantile``
  ``[n_period][Lv][L]`` (a sweep: a leading ``[P]`` axis), and the run ends with the line
  `` [Ensemble xN] uptake: L layers over R periods, median depth ... cm``.
* ``"Ensemble": {..., "Distribution": {"Stride": 48, "Quantiles": [0.05, 0.5, 0.95]}}``: the members' water-table index
  counted per row on the GPU -- every 48th forcing row (default 48; 0 = off) a histogram over the depth grid, summed over
  the ranks like the moments -- and from it the quantile depths (NumPy's ``method="inverted_cdf"``; default levels 0.05,
  0.25, 0.5, 0.75, 0.95, at most 16) and the CRPS against the well, the ensemble form of the reference's ``abs_error``
  (simulation.py:612-615: for one member the CRPS is ``abs_error``).  Added to ``<Output_Name>_ensemble.h5``:
  ``wtd_hist`` ``[T_out][D]``, ``wtd_hist_rows``, ``wtd_hist_count``, ``wtd_quantile_levels``, ``wtd_quantile_cm``
  ``[T_out][L]``, ``wtd_crps_cm`` ``[T_out]`` and ``wtd_crps_mean_cm`` (a sweep: a leading ``[P]`` axis), and the run
  ends with the line `` [Ensemble xN] CRPS = ... cm over R rows``, as the reference ends with its MAE.
* ``"Ensemble": {..., "Filter": {"Stride": 48, "Sigma_cm": 10.0, "Seed": s}}``: a bootstrap particle filter on the well
  (include/hydrocol.h hc_set_filter) -- on every 48th forcing row (default 48; 0 = off) that has an observation the members
  of each parameter point are weighted by the Gaussian likelihood of the observed water table (``Sigma_cm``, required:
  finite and > 0) and resampled on the GPU (``Seed``: default the ensemble's seed).  Moments, profiles and histograms
  describe the forecast of each row; the states continue from the analysis.  Added to ``<Output_Name>_ensemble.h5``:
  ``filter_rows``, ``filter_count``, ``filter_ess``, ``filter_loglik_rows``, ``filter_survivors`` ``[R]``, ``filter_loglik``
  (the log marginal likelihood of the well record, log cm^-1) and ``filter_sigma_cm`` (a sweep: a leading ``[P]`` axis), and
  the run ends with `` [Ensemble xN] filter log-likelihood = ... over R rows`` (a sweep: the best point).  A single-point
  ensemble on several GPUs is refused (resampling would move states between ranks) unless the block is sharded:
* ``"Filter": {..., "Sharded": true}``: a single-point ensemble's particle filter on ``--gpus N`` (include/hydrocol.h
  hc_set_filter_shard).  The members are dealt by ``multigpu.shard`` (any split), every assimilation gathers the members'
  water-table indices, every rank forms the whole ancestry, and the columns whose ancestor lives on another rank are
  exchanged; the states, tables, closing lines and the file are those of the one-GPU run to the bit (``gpus`` apart); the
  filter's tables are rank 0's.  ``false`` or no key: the refusal above.  A sweep accepts and ignores the key.  Added to
  the file when the key is given: ``filter_sharded``.
* ``"Filter": {..., "ESS_floor": 0.1}``: hold the effective sample size of every resampling above that fraction of the
  counted members (0 < f < 1; include/hydrocol.h hc_set_filter_tempering): per row and point the weights are raised to the
  largest exponent beta = k / 1024 of a bisection in exact integers that keeps it there -- the observation error inflated
  by 1 / sqrt(beta) where the stated one would spend the ensemble's diversity on one row.  ``filter_ess`` and
  ``filter_loglik_rows`` keep scoring the forecast with the stated error; ``filter_survivors`` counts the resampling that
  happened.  With ``Soil_Moisture``, ``Sharded``, a sweep and either noise source.  Added to the file: ``filter_ess_floor``
  and, over the ``filter_rows`` ``[R]``, ``filter_beta``, ``filter_ess_tempered``, ``filter_ess_target`` (a sweep: a leading
  ``[P]`` axis), and the run ends with `` [Ensemble xN] filter tempering: K of R rows tempered, smallest beta = ...``.
* ``"Filter": {..., "Rejuvenation": 0.95}``: rejuvenate the members' base noise vectors -- their conductivity fields, which
  resampling only ever loses -- after every resampling that copied a member (Liu & West's kernel shrinkage with that
  discount, 0.5 <= delta < 1; include/hydrocol.h hc_set_filter_rejuvenation): the vectors of a point are pulled towards
  their mean by a = (3 delta - 1) / (2 delta) and given a Gaussian jitter of sqrt(1 - a^2) times their spread, so that mean
  and variance per node stay what the resampling left and no two members share a field.  With ``Soil_Moisture``,
  ``ESS_floor``, ``Window_Offsets``, period totals, a sweep and either noise source; not together with ``"Sharded": true``
  on a single-point run (the gathered words are water-table indices).  With a single survivor there is no spread to restore:
  give an ``ESS_floor`` as well.  Added to the file: ``filter_rejuvenation_discount``, ``filter_rejuvenation_shrinkage`` and,
  over the ``filter_rows`` ``[R]``, ``filter_rejuvenated``, ``filter_rejuvenation_refused``, ``filter_noise_std_resampled``,
  ``filter_noise_std_rejuvenated`` (a sweep: a leading ``[P]`` axis), and the run ends with `` [Ensemble xN] filter
  rejuvenation: K of R rows, noise-field spread kept ... of resampled``.
* ``"Filter": {..., "Window_Offsets": [12, 24, 36]}``: the well's record inside the window (include/hydrocol.h
  hc_set_filter_window), the counterpart of ``EnKF.Window_Offsets`` with its rules.  Each entry is a number of rows before
  the assimilation row; nothing is resampled in between, so every member's weight becomes the likelihood of all the
  observations its trajectory passed, and ``filter_loglik_rows`` the joint increment.  Not together with ``"Sharded": true``
  on a single-point run (the sharded filter gathers the indices of the assimilation row only).  Without the key, or with an
  empty list, nothing changes.  Added to the file: ``filter_window_offsets`` ``[n]`` (ascending) and, over the
  ``filter_rows`` ``[R]``, ``filter_window_observed``, ``filter_window_obs_cm``, ``filter_window_prior_mean_cm``,
  ``filter_window_prior_std_cm`` ``[R][n]`` (NaN where the offset's row took no part; a sweep: a leading ``[P]`` axis), and
  the run ends with `` [Ensemble xN] filter window: K lagged observations over R rows``.
* ``"Filter": {..., "Smoother": {"Stride": 48, "Lag_rows": 480, "Quantiles": [0.05, 0.5, 0.95]}}``: the fixed-lag smoother
  of the water table by ancestry (include/hydrocol.h hc_set_filter_smoother): every slot carries the water-table indices of
  the member it descends from on every ``Stride``-th row, and a row is counted ``Lag_rows`` later (a multiple of ``Stride``,
  at most 64 of them; 0: the analysis) -- its distribution given the well's record up to then.  This is the one table that
  describes the posterior: every other one describes the forecast.  The rows the run's end leaves pending are counted with
  the lag they reached (``smooth_lag_rows``).  Far enough back every slot descends from one member: ``smooth_unique_paths``
  counts the distinct paths behind each row, and when it falls towards 1 give an ``ESS_floor`` or a shorter lag.  Refused:
  a block that is no object, unknown keys, bools, a ``Lag_rows`` that is no multiple of ``Stride`` or more than 64 of them,
  more than 16 levels, a filter whose ``Stride`` is 0, and ``"Sharded": true`` on a single-point run.  Added to the file,
  over the emitted rows ``smooth_rows`` ``[R]``: ``smooth_count``, ``smooth_lag_rows``, ``smooth_unique_paths``,
  ``smooth_crps_cm`` ``[R]``, ``smooth_hist`` ``[R][D]``, ``smooth_quantile_cm`` ``[R][L]``, ``smooth_quantile_levels``,
  ``smooth_crps_mean_cm``, ``smooth_stride`` and ``smooth_lag`` (a sweep: a leading ``[P]`` axis), and the run ends with
  `` [Ensemble xN] smoother: CRPS = ... cm at lag L rows over R rows, fewest paths K``.
* ``"Filter": {..., "Soil_Moisture": {"Filename": "sm.csv", "Depths_cm": [30, 60, 120], "Sigma": 0.02}}``: a soil-moisture
  record joins the well in the filter's weights (include/hydrocol.h hc_set_filter_soil_moisture): on a row with sensor
  values every member is weighted by the joint Gaussian likelihood of the well and of theta at the sensors' nodes, so the
  weights belong to a member and not to a 5 cm bin.  The block, its CSV and its refusals are those of ``EnKF.Soil_Moisture``
  below.  Not together with ``"Sharded": true`` on a single-point run (the sharded filter gathers water-table indices
  only); a sweep on any number of GPUs takes it.  Added to the file: ``filter_sm_depths_cm``, ``filter_sm_nodes``,
  ``filter_sm_sigma`` ``[m]`` and, over the ``filter_rows`` ``[R]``, ``filter_sm_observed``, ``filter_sm_obs``,
  ``filter_sm_prior_mean``, ``filter_sm_prior_std``, ``filter_sm_post_mean``, ``filter_sm_post_std`` ``[R][m]`` (the
  forecast ensemble and the resampled one; NaN on rows with no sensor value; a sweep: a leading ``[P]`` axis);
  ``filter_loglik_rows`` holds the joint increment on sensor rows, and the run ends with
  `` [Ensemble xN] soil-moisture forecast RMSE = ... over R rows``.
* ``"Ensemble": {..., "EnKF": {"Stride": 48, "Sigma_cm": 10.0, "Localisation_cm": 0, "Seed": s}}``: a stochastic ensemble
  Kalman filter on the well's continuous water table (include/hydrocol.h hc_set_enkf) -- on every 48th forcing row (default
  48; 0 = off) that has an observation each member's psi moves by the sample covariance with the water table, per parameter
  point, on the GPU (``Sigma_cm``, required: finite and > 0; ``Localisation_cm``: the Gaspari-Cohn half-width, default 0 =
  none; ``Seed``: default the ensemble's seed).  Not together with ``"Filter"``.  Moments, profiles and histograms describe
  the forecast.  Added to ``<Output_Name>_ensemble.h5``: ``enkf_rows``, ``enkf_count``, ``enkf_prior_mean_cm``,
  ``enkf_prior_std_cm``, ``enkf_innovation_cm``, ``enkf_post_mean_cm``, ``enkf_post_std_cm``, ``enkf_loglik_rows``,
  ``enkf_rejected`` ``[R]``, ``enkf_loglik``, ``enkf_sigma_cm`` and ``enkf_localisation_cm`` (a sweep: a leading ``[P]``
  axis), and the run ends with `` [Ensemble xN] EnKF log-likelihood = ... over R rows`` (a sweep: the best point).  A
  single-point ensemble on several GPUs is refused (the covariances would need a sum over ranks) unless the block is
  sharded:
* ``"EnKF": {..., "Sharded": true}``: a single-point ensemble's EnKF on ``--gpus N`` (include/hydrocol.h
  hc_set_enkf_shard).  The members are dealt in whole tiles of 256 (``multigpu.shard_tiles``: at least N tiles), every
  analysis gathers the ranks' tile partials before each of its reductions, and the states, tables, closing lines and the
  file are those of the one-GPU run to the bit (``gpus`` apart); the EnKF's tables are rank 0's.  ``false`` or no key:
  the refusal above.  A sweep accepts and ignores the key.  Added to the file when the key is given: ``enkf_sharded``.
* ``"EnKF": {..., "Soil_Moisture": {"Filename": "sm.csv", "Depths_cm": [30, 60, 120], "Sigma": 0.02}}``: a soil-moisture
  record joins the well in the EnKF's analyses (include/hydrocol.h hc_set_enkf_soil_moisture).  The CSV is header-less
  ``ID, Datenum, VWC_1, ..., VWC_m`` (as the forcing), one row per forcing row with the same ``Datenum``; an empty field or
  NaN is no observation, values lie in [0, 1].  A depth maps to the first node with ``z >= depth`` (the well's rule,
  src/simulation.py:255) and must lie in [z[0], z[D-1]]; at most 8 depths; ``Sigma`` (m^3/m^3, finite and > 0) is one
  number or one per depth.  Added to ``<Output_Name>_ensemble.h5``: ``enkf_sm_depths_cm``, ``enkf_sm_nodes``,
  ``enkf_sm_sigma`` ``[m]`` and, over the ``enkf_rows`` ``[R]``, ``enkf_sm_observed``, ``enkf_sm_obs``,
  ``enkf_sm_prior_mean``, ``enkf_sm_prior_std``, ``enkf_sm_post_mean``, ``enkf_sm_post_std`` ``[R][m]`` (NaN on rows with
  no sensor value; a sweep: a leading ``[P]`` axis), and the run ends with
  `` [Ensemble xN] soil-moisture forecast RMSE = ... over R rows`` (the prior mean theta against the record).
* ``"EnKF": {..., "Method": "sqrt", "Relaxation": 0.5}``: the analysis scheme of the EnKF (include/hydrocol.h
  hc_set_enkf_method).  ``Method``: ``"stochastic"`` (perturbed observations, the default) or ``"sqrt"``, the deterministic
  square-root analysis of Whitaker & Hamill (2002): the mean moves by the Kalman gain, the anomalies by a reduced gain,
  nothing is drawn (``Seed`` no longer matters).  ``Relaxation``: the relaxation to prior spread alpha, a finite number in
  [0, 1] (default 0 = none), for either method: after each analysis every node's spread is (1 - alpha) sigma_a + alpha
  sigma_b, and the posterior datasets describe the relaxed ensemble.  Added to ``<Output_Name>_ensemble.h5`` when either
  is given: ``enkf_method`` (0 = stochastic, 1 = sqrt) and ``enkf_relaxation``.
* ``"Ensemble": {..., "Noise_Correlation": {"Length_cm": 50.0, "Layers": true}}``: a vertical correlation length of the
  conductivity noise fields (include/hydrocol.h hc_set_noise_correlation): every base and refresh vector of the Philox
  source becomes an exponentially correlated field of unit variance, with ``Layers`` (default false) independent across
  the layer interfaces inside the column; applied after the spin-up, before the filters.  Refused with ``"Noise":
  "numpy"`` and with ``Filter.Rejuvenation``.  ``<Output_Name>_ensemble.h5`` gains ``noise_correlation_length_cm``,
  ``noise_correlation_layers`` and ``noise_correlation_a`` (``[D]``; a sweep: ``[P][D]``), and the run ends with
  `` [Ensemble xN] noise correlation: length ... cm, K breaks``.  Without the key every bit, file and line stays.
* ``"Ensemble": {..., "Forcing_Perturbation": {"Precipitation_Sigma": 0.3, "Demand_Sigma": 0.1, "Correlation_Days": 3,
  "Seed": s}}``: input uncertainty (include/hydrocol.h hc_set_forcing_perturbation).  Every member integrates with the
  record's rainfall and atmospheric demand times a log-normal factor of mean one of its own, constant over a day (48
  rows) and an AR(1) from day to day with e-folding time ``Correlation_Days``; the refresh rule, surface evaporation,
  daylight, the well's record and the spin-up stay the record's.  At least one sigma is required, each a finite number in
  [0, 1]; ``Correlation_Days`` in [0, 365], default 0 (white in time); ``Seed`` defaults to the ensemble's.  Applied after
  the spin-up, before the filters; the particle filter moves a member's factor state with it, the EnKF leaves it alone
  unless the block says ``"EnKF": true`` (below).
  Works with either noise source, both filters, every table, a sweep, a sharded EnKF and ``--gpus N`` (members are keyed
  by their global id).  Refused: a non-object, an unknown key, a bool or non-finite number, a value outside its range, and
  ``"Filter": {"Sharded": true}`` on a single-point run (the exchanged columns do not carry the factor state).
  ``<Output_Name>_ensemble.h5`` gains ``forcing_precipitation_sigma``, ``forcing_demand_sigma``,
  ``forcing_correlation_days``, ``forcing_phi`` and ``forcing_seed``, and the run ends with `` [Ensemble xN] forcing
  perturbation: precipitation sigma ..., demand sigma ..., correlation ... days``.  Without the key every bit, file and
  line stays.
* ``"Forcing_Perturbation": {..., "EnKF": true}`` or ``{"EnKF": {"Relaxation": 0.2}}``: joint state and forcing-error
  estimation (include/hydrocol.h hc_set_enkf_forcing).  Every EnKF analysis also updates each member's factor state g of
  the day the row lies in, from the same observations, draws and factor, with no taper on its covariance with the
  observations; the rest of that day, and through the AR(1) every later day, then run with the corrected factors.  The
  anomalies are relaxed to prior spread with the given ``Relaxation`` (``true``: the EnKF block's); g regains spread from
  its own recursion, so 0 is a sound choice.  Refused before any GPU call: a value that is neither a bool nor an object,
  an unknown inner key, a relaxation that is a bool or outside [0, 1], no ``EnKF`` block with ``Stride`` > 0 (a ``Filter``
  block instead included), and ``"EnKF": {"Sharded": true}`` on a single-point run (the exchanged partials cover psi
  only).  A sweep works on any number of GPUs.  Without the key, or with ``false``, nothing changes.  Added to
  ``<Output_Name>_ensemble.h5``: ``enkf_forcing`` (1), ``enkf_forcing_relaxation`` and, over the ``enkf_rows`` ``[R]``,
  ``enkf_forcing_prior_mean``, ``enkf_forcing_prior_std``, ``enkf_forcing_post_mean``, ``enkf_forcing_post_std``
  ``[R][2]`` (precipitation, demand) and ``enkf_forcing_rejected`` ``[R]`` (a sweep: a leading ``[P]`` axis), and the run
  ends with `` [Ensemble xN] EnKF forcing: posterior spread ... / ... of prior (precipitation / demand) over R rows``.
* ``"EnKF": {..., "Noise_Field": true}`` or ``{"Noise_Field": {"Relaxation": 0.5}}``: every analysis also updates each
  member's base noise vector -- its conductivity field -- together with its state, from the same observations, draws and
  factor (include/hydrocol.h hc_set_enkf_noise_field).  The vectors' anomalies are relaxed to prior spread with the
  given ``Relaxation`` (``true``: the block's); parameters regain no spread from the dynamics, so without one a long run
  collapses the field.  Refused: outside an EnKF block with ``Stride`` > 0, a value that is neither a bool nor an object
  with the one key ``Relaxation``, a relaxation outside [0, 1], and ``"Sharded": true`` on a single-point run (the
  exchanged partials cover psi only).  Without the key, or with ``false``, nothing changes.  Added to
  ``<Output_Name>_ensemble.h5``: ``enkf_noise_field`` (1), ``enkf_noise_relaxation`` and, over the ``enkf_rows`` ``[R]``,
  ``enkf_noise_prior_mean``, ``enkf_noise_prior_std``, ``enkf_noise_post_mean``, ``enkf_noise_post_std`` ``[R][D]`` and
  ``enkf_noise_rejected`` ``[R]`` (a sweep: a leading ``[P]`` axis), and the run ends with `` [Ensemble xN] EnKF noise
  field: posterior spread ... of prior over R rows`` (the mean over nodes and rows of sigma_post / sigma_prior).
* ``"EnKF": {..., "Window_Offsets": [12, 24, 36]}``: the well's record inside the window (the asynchronous EnKF of Sakov,
  Evensen & Bertino 2010; include/hydrocol.h hc_set_enkf_window).  Each entry is a number of rows before the analysis
  row: distinct integers in [1, ``Stride``), at most 8, and at most 8 together with the ``Soil_Moisture`` depths.  On such a
  row, if it has an observation, every member's water table is recorded when the row is solved, and joins the next
  analysis as one more well observation (error ``Sigma_cm``, errors taken as uncorrelated).  Without the key, or with an
  empty list, nothing changes.  Added to ``<Output_Name>_ensemble.h5``: ``enkf_window_offsets`` ``[n]`` (ascending) and,
  over the ``enkf_rows`` ``[R]``, ``enkf_window_observed``, ``enkf_window_obs_cm``, ``enkf_window_prior_mean_cm``,
  ``enkf_window_prior_std_cm``, ``enkf_window_innovation_cm`` ``[R][n]`` (NaN where the offset's row took no part; a sweep:
  a leading ``[P]`` axis), and the run ends with `` [Ensemble xN] EnKF window: K lagged observations over R rows``.
* ``"Ensemble": {"repair_predict": true}`` with ``Simulation_Flags.PREDICT``: run the repaired predictive lateral flow
   instead of raising the reference's ``TypeError``.
"""
import sys
from dataclasses import dataclass, replace
from pathlib import Path
from typing import Optional

REQUIRED_KEYS = ("Trees", "Well_No", "Output_Name", "IC_Filename",
                 "Data_Filename", "Water_Content", "Environmental",
                 "Soil_Properties", "Site_Information", "Simulation_Flags",
                 "Hydrological_Model", "Hydraulic_Conductivity")


def validateInputParametersFile(filename, quiet=False):
    """berkeley_hydro_main.py:13-61: key membership only, values are not validated here."""
    import json
    with open(filename, "r") as fh:
        settings = json.load(fh)
    missing = [key for key in REQUIRED_KEYS if key not in settings]
    if missing:
        raise ValueError(f" Key: {missing[0]}, is not given.")
    if not quiet:
        print(" Model parameters are given correctly.")
    return settings


def _speaks():
    """One voice per run: the single process, or rank 0 of a multi-GPU run."""
    import os
    return int(os.environ.get("RANK", "0")) == 0


def _read_parameters(params_file):
    """The first half of berkeley_hydro_main.py:65-100: no file -> message + exit 1; a bad file -> its message + exit 1.
    (The ranks of a run this command started itself stay quiet: their parent has said it.)"""
    import os
    if params_file is None:
        print(" The simulation can't run without input parameters.")
        sys.exit(1)
    try:
        return validateInputParametersFile(Path(params_file), quiet=("HYDROCOL_EXPECT_WORLD" in os.environ) or not _speaks())
    except ValueError as bad_key:
        print(bad_key)
        sys.exit(1)


def main(params_file=None, data_file=None, seed=None, device=0, gpus=None, _settings=None):
    """berkeley_hydro_main.py:65-145.  Inside a rank of a multi-GPU run (RANK / WORLD_SIZE set by the launcher) the rank
    takes its own GPU and its share of the members / points; only rank 0 reports and writes."""
    import pandas as pd
    from . import multigpu
    params = _settings if _settings is not None else _read_parameters(params_file)
    csv_path = Path(data_file) if data_file is not None else Path(params["Data_Filename"])
    ranks = None
    try:
        if params.get("Ensemble"):
            distribution_settings(params["Ensemble"])      # a bad Distribution block fails before any GPU is touched
            profile_distribution_settings(params["Ensemble"])
            storage_settings(params["Ensemble"])
            conductivity_settings(params["Ensemble"])
            period_settings(params["Ensemble"])
            uptake_settings(params["Ensemble"])
        n_gpus = multigpu.requested_gpus(gpus, params)
        if params.get("Ensemble"):
            filter_settings(params["Ensemble"], n_gpus)     # so does a bad Filter block
            enkf_settings(params["Ensemble"], n_gpus)       # and a bad EnKF block
            soil_moisture_settings(params["Ensemble"], n_gpus)
            soil_moisture_settings(params["Ensemble"], n_gpus, "Filter")
            enkf_method_settings(params["Ensemble"])
            enkf_window_settings(params["Ensemble"])
            enkf_noise_settings(params["Ensemble"])
            filter_window_settings(params["Ensemble"])
            filter_smoother_settings(params["Ensemble"])
            noise_correlation_settings(params["Ensemble"])
            forcing_perturbation_settings(params["Ensemble"])
        ranks = multigpu.Ranks(expect=n_gpus if (n_gpus > 1 or multigpu.in_rank()) else None)
        if ranks.world > 1:
            device = ranks.device_index()
        if ranks.rank == 0:
            print(f" Simulation water data file: {csv_path}")
        with open(csv_path, "r") as fh:
            forcing_table = pd.read_csv(fh, names=["ID", "Datenum", "Precipitation_cm", "WTD_m"])
        run_name = params["Output_Name"] if params["Output_Name"] is not None else "Sim_01"
        if seed is None:
            seed = params.get("Seed")
        ens = params.get("Ensemble")
        if ens:
            _run_ensemble(params, forcing_table, run_name, ens, device, ranks)
        elif ranks.world > 1:
            raise ValueError(" --gpus / Ensemble.GPUs needs an \"Ensemble\" block: one column is one GPU's work.")
        else:
            from .simulation import Simulation
            column_run = Simulation(run_name, seed=seed, device=device)
            column_run.setupModel(params, forcing_table)
            column_run.run()
            column_run.saveResults()
    except Exception as failure:  # noqa: BLE001 - the reference converts every failure to exit status 1
        import os
        print(failure if _speaks() else f" [rank {os.environ.get('RANK')}] {failure}")
        # A failure may belong to this rank alone (its GPU, its shard): the peers are then inside, or heading for, the
        # run's one all-reduce, and tearing the communicator down here can block on them.  Leave it alone and end the
        # process with status 1 -- the launcher stops the other ranks and reports the failure.
        sys.stdout.flush()
        if ranks is not None and ranks.world > 1:
            os._exit(1)
        sys.exit(1)
    ranks.close()


def _save(stem, arrays, what, ranks):
    """<stem>.h5 through libhdf5 (same container as Simulation.saveResults, simulation.py:697-706) or .npz; rank 0 only."""
    import numpy as np
    from . import hdf5io
    if ranks.rank != 0:
        return None
    if hdf5io.available():
        out = Path(stem + ".h5")
        hdf5io.write(out, arrays)
    else:
        out = Path(stem + ".npz")
        np.savez_compressed(out, **arrays)
    print(f" Saving the {what} to: {out}")
    return out


def _run_ensemble(params, water_data, output_name, ens, device, ranks):
    import numpy as np
    from . import multigpu
    from .digest import ColumnTables, ForcingDigest, load_site_well
    from .ensemble import EnsembleSimulation
    dist_stride, dist_levels = distribution_settings(ens)
    theta = profile_distribution_settings(ens)
    storage = storage_settings(ens)
    cond = conductivity_settings(ens)
    cov = covariance_settings(ens)
    periods = period_settings(ens)
    filt = filter_settings(ens, ranks.world)
    ess_floor = filter_ess_floor(ens)
    rejuvenation = filter_rejuvenation(ens)
    enkf = enkf_settings(ens, ranks.world)
    sm = soil_moisture_settings(ens, ranks.world)
    fsm = soil_moisture_settings(ens, ranks.world, "Filter")
    scheme = enkf_method_settings(ens)
    window = enkf_window_settings(ens)
    noise_alpha = enkf_noise_settings(ens)
    fwindow = filter_window_settings(ens)
    smoother = filter_smoother_settings(ens)
    corr = noise_correlation_settings(ens)
    pert = forcing_perturbation_settings(ens)
    cols = ColumnTables(params, load_site_well(params))
    forcing = ForcingDigest(params, water_data, cols)
    record = soil_moisture_record_of(sm, cols, water_data)      # before any GPU call
    storage_ranges(storage, cols)                               # (its refusals too)
    conductivity_layer_ranges(cond, cols)                       # (and the conductivity layers')
    if cov is not None:
        covariance_check(cov, cols.dim_d, forcing.dim_t, _profile_stride(ens), len(ens.get("Points") or [0]))
    frecord = soil_moisture_record_of(fsm, cols, water_data, "Filter")
    assim = Assimilation(filt, frecord, ess_floor, fwindow, rejuvenation, enkf, record, scheme, window, noise_alpha,
                         smoother=smoother, forcing_alpha=None if pert is None else pert.get("enkf_relaxation"))
    if cols.flags["PREDICT"] and not ens.get("repair_predict"):
        raise TypeError("'numpy.float64' object cannot be interpreted as an integer")     # richards_pde.py:327-330
    n_members = int(ens.get("Members", 4096))
    days = int(ens.get("Days", (forcing.dim_t - 1) // 48))
    rows = min(days * 48, forcing.dim_t - 1)
    plan = period_plan(periods, cols, forcing, rows)            # before any GPU call, like the storage's ranges
    uptake = uptake_settings(ens)
    run = RunSettings(dist=(dist_stride, dist_levels), theta=theta, storage=storage, cov=cov, periods=periods, plan=plan,
                      conductivity=cond, uptake=uptake, corr=corr, pert=pert, assim=assim)
    if ens.get("Points"):
        return _run_sweep(params, forcing, output_name, ens, n_members, rows, device, ranks, run)
    run = replace(run, ucells=uptake_plan(uptake, [cols]))      # (so are the uptake's layers)
    sharded = enkf_sharded(ens)
    fsharded = filter_sharded(ens)
    if sharded:
        # whole tiles of the EnKF's sums per rank, and the analyses gather them: the one-rank run on any number of GPUs
        lo, hi = multigpu.shard_tiles(n_members, ranks.rank, ranks.world)
        shard_kw = dict(enkf_shard=(n_members, multigpu.ShardExchange(ranks)))
    elif fsharded:
        # any split will do: every rank forms the whole ancestry and the ranks exchange the columns that change hands
        bounds = [0] + [multigpu.shard(n_members, r, ranks.world)[1] for r in range(ranks.world)]
        lo, hi = bounds[ranks.rank], bounds[ranks.rank + 1]
        shard_kw = dict(filter_shard=(bounds, ranks.rank, multigpu.ShardExchange(ranks)))
    else:
        lo, hi = multigpu.shard(n_members, ranks.rank, ranks.world)
        shard_kw = {}
    if hi <= lo:
        raise ValueError(f" Ensemble: {n_members} members do not shard over {ranks.world} GPUs (a rank would be empty).")
    run = replace(run, stride=_profile_stride(ens))
    sim = EnsembleSimulation(cols, forcing, hi - lo, seed=int(ens.get("Seed", 0)), device=device, member_offset=lo,
                             noise=str(ens.get("Noise", "philox")).lower(),
                             spinup=str(ens.get("Spinup", "shared")).lower(), **run.kwargs(), **shard_kw)
    label = f"Ensemble x{n_members}"
    _step_all(sim, rows, label, ranks)
    # the run's one collective: int64 (count, sum idx, sum idx^2) per row, exact and order-independent
    moments = ranks.allreduce_sum(np.asarray(sim.moments(), dtype=np.int64))
    mean_cm, std_cm = sim.wtd_mean_std(moments)
    # completeness, row by row: a solved row (its observation lies on the grid) must count every member of every shard,
    # a skipped row nobody (simulation.py:582-588); a run whose rows are all skipped has nothing to check
    expect = np.where(np.asarray(forcing.wtd_obs[1:rows + 1]) >= 0, n_members, 0).astype(np.int64)
    got = np.asarray(moments[0][1:rows + 1], dtype=np.int64)
    if not np.array_equal(got, expect):
        bad = int(np.flatnonzero(got != expect)[0])
        raise RuntimeError(f" Ensemble: the reduced moments hold {int(got[bad])} members on row {bad + 1}, expected "
                           f"{int(expect[bad])} ({int((got != expect).sum())} rows differ).")
    psi0 = np.asarray(sim.psi0)
    extra = {}
    if psi0.ndim == 2 and ranks.world > 1:
        # one spin-up per member: the shards' initial conditions, assembled like a sweep's (zeros elsewhere, summed) when
        # the table is small enough to travel; otherwise rank 0's block, with its member range
        if n_members * psi0.shape[1] * 8 <= 256 * 1024 * 1024:
            psi0 = multigpu.place_points(psi0, np.arange(lo, hi), n_members, ranks)
        else:
            extra["initial_cond_members"] = np.array([lo, hi])
    # the optional tables are integer sums like the moments: one more exact all-reduce each
    tables, lines = _reduce_diagnostics(ranks, sim, [0], [cols], forcing, run, device, label, keep_points=False)
    extra.update(tables)
    # the filters' tables describe the one point: every rank of a sharded run holds the same ones, and rank 0's are taken
    # (placed by it alone; a sum over the ranks would count them world times)
    eids = [0] if ranks.rank == 0 else []
    atables, assim_lines = _reduce_assimilation(ranks, sim, eids, 1, forcing.dim_t, cols, assim, label, keep_points=False)
    extra.update(atables)
    stables, smooth_line = _reduce_smoother(ranks, sim, eids, 1, forcing.dim_t, cols, forcing, assim, device, label,
                                            keep_points=False)
    extra.update(stables)
    if fsharded is not None:
        extra["filter_sharded"] = np.array(1 if fsharded else 0, dtype=np.int8)
    if sharded is not None:
        extra["enkf_sharded"] = np.array(1 if sharded else 0, dtype=np.int8)
    ctables, corr_line = _noise_correlation_arrays(corr, [cols], label, keep_points=False)
    extra.update(ctables)
    ptables, pert_line = _forcing_perturbation_arrays(pert, label)
    extra.update(ptables)
    arrays = dict(moments=moments, wtd_mean_cm=mean_cm, wtd_std_cm=std_cm, rows=np.array(rows),
                  members=np.array(n_members), gpus=np.array(ranks.world), initial_cond=psi0, **extra)
    _save(output_name.strip().replace(" ", "_") + "_ensemble", arrays, "ensemble water-table statistics", ranks)
    _print_lines(lines.pop("crps"), *assim_lines, smooth_line, *lines.values(), corr_line if ranks.rank == 0 else None,
                 pert_line if ranks.rank == 0 else None)
    sim.close()


def _print_lines(*lines):
    """The run's closing lines, those that are there, in the order given."""
    for line in lines:
        if line:
            print(line)


@dataclass(frozen=True)
class Assimilation:
    """The assimilation settings of a run as the settings functions return them (``filter_settings``,
    ``soil_moisture_record_of`` ... in the field order below; None / a zero stride: not given), from ``_run_ensemble`` to
    the simulation's constructor and the reducers."""
    filt: tuple = (0, None, None)
    frecord: Optional[dict] = None
    ess_floor: Optional[float] = None
    fwindow: Optional[tuple] = None
    rejuvenation: Optional[float] = None
    enkf: tuple = (0, None, None, None)
    record: Optional[dict] = None
    scheme: Optional[tuple] = None
    window: Optional[tuple] = None
    noise_alpha: Optional[float] = None
    smoother: Optional[tuple] = None
    forcing_alpha: Optional[float] = None   # Forcing_Perturbation.EnKF (it reaches the constructor inside RunSettings.pert)

    def kwargs(self):
        """The ``filter_*`` / ``enkf_*`` keywords of EnsembleSimulation / SweepSimulation: an owner that is off and an
        option that was not given pass nothing."""
        kw = {}
        if self.filt[0]:
            kw.update(filter_stride=self.filt[0], filter_sigma_cm=self.filt[1], filter_seed=self.filt[2])
            given = dict(filter_soil_moisture=self.frecord, filter_ess_floor=self.ess_floor,
                         filter_window_offsets=self.fwindow or None, filter_rejuvenation=self.rejuvenation)
            kw.update((k, v) for k, v in given.items() if v is not None)
            if self.smoother is not None:
                kw.update(filter_smoother={"stride": self.smoother[0], "lag_rows": self.smoother[0] * self.smoother[1]})
        if self.enkf[0]:
            kw.update(enkf_stride=self.enkf[0], enkf_sigma_cm=self.enkf[1], enkf_localisation_cm=self.enkf[2],
                      enkf_seed=self.enkf[3])
            given = dict(enkf_soil_moisture=self.record, enkf_window_offsets=self.window or None,
                         enkf_noise_field=None if self.noise_alpha is None else {"relaxation": self.noise_alpha})
            kw.update((k, v) for k, v in given.items() if v is not None)
            if self.scheme is not None:
                kw.update(enkf_method=self.scheme[0], enkf_relaxation=self.scheme[1])
        return kw


@dataclass(frozen=True)
class RunSettings:
    """Everything ``Ensemble`` asks of a run, as the ``*_settings`` functions returned it (None / a zero stride: not
    given) and with the plans made from it before any GPU call: built once by ``_run_ensemble`` and handed as one value
    to the simulation's constructor (:meth:`kwargs`), the sweep and the reducers."""
    stride: int = 0                         # the profile statistics' (_profile_stride), read where the run is built
    dist: tuple = (0, None)                 # distribution_settings: (stride, levels)
    theta: tuple = (0, None)                # profile_distribution_settings: (bins, levels)
    storage: Optional[tuple] = None
    cov: Optional[tuple] = None
    conductivity: Optional[tuple] = None    # conductivity_settings: the layers (none: ())
    periods: Optional[dict] = None
    plan: Optional[tuple] = None            # period_plan
    uptake: Optional[dict] = None
    ucells: Optional[object] = None         # uptake_plan, of the run's points
    corr: Optional[dict] = None
    pert: Optional[dict] = None
    assim: Assimilation = Assimilation()

    def kwargs(self):
        """The keywords of EnsembleSimulation / SweepSimulation: what was not given passes nothing."""
        kw = dict(profile_stride=self.stride, wtd_hist_stride=self.dist[0], theta_hist_bins=self.theta[0], **self.assim.kwargs())
        given = dict(noise_correlation=self.corr, forcing_perturbation=self.pert,
                     theta_cov_stride=None if self.cov is None else self.cov[0])
        kw.update((k, v) for k, v in given.items() if v is not None)
        if self.storage is not None:
            kw.update(storage_layers_cm=self.storage[0], storage_bins=self.storage[1])
        if self.conductivity is not None:
            kw.update(conductivity={"layers_cm": list(self.conductivity) or None})
        if self.periods is not None:
            kw.update(period_ends=self.plan[0], period_thresholds_cm=self.periods["thresholds_cm"],
                      period_bins=self.periods["bins"])
            if self.periods["bins"]:
                kw.update(period_flux_max_cm=self.periods["flux_max_cm"])
        if self.uptake is not None:
            kw.update(uptake_layers_cm=self.uptake["layers_cm"], uptake_bins=self.uptake["bins"])
        return kw


def _placed_table(ranks, sim, ids, P, T, D, stride, key, n=0):
    """The assimilation table ``key`` (stepper.ASSIM_TABLES) of the run's ``P`` points: this rank's handle ``sim`` (None:
    it holds no points) gives its points ``ids``, placed in the [P][n_arow] + trailing table and summed over the ranks
    (float64 as int64 bits: ``multigpu.place_points``) -- one collective.  ``n``: the owner's sensors or offsets, for the
    tables that have them."""
    import numpy as np
    from .multigpu import place_points
    from .stepper import assim_table_shape, stride_rows
    shape = (stride_rows(T, stride),) + assim_table_shape(key, D, n, n)
    local = sim.assim_table(key).reshape((-1,) + shape) if sim is not None else np.zeros((0,) + shape)
    return place_points(local, ids, P, ranks)


def _placed_diag(ranks, sim, ids, P, key, counts):
    """The parts of the diagnostic table ``key`` (stepper.DIAG_TABLES) of the run's ``P`` points: this rank's handle ``sim``
    (None: it holds no points, and gives the layout at P = 0 of ``counts``, stepper.diag_counts) gives its points ``ids``;
    the [P]-leading parts are placed at them, the global words (overflow, outside count) go as they are, and the whole
    is summed over the ranks as int64 -- one collective, an int32 histogram's outside count with it."""
    import numpy as np
    from .multigpu import place_points
    from .stepper import diag_entry, diag_layout, diag_placed, join_diag, split_diag
    if sim is not None:
        parts = sim.stepper.diag_parts(key)
    else:
        none = dict(counts, P=0)
        parts = split_diag(key, np.zeros(diag_layout(key, none)["words"][0], dtype=diag_entry(key).dtype), none)
    parts.update((name, place_points(parts[name], ids, P)) for name in diag_placed(key))
    return split_diag(key, ranks.allreduce_sum(join_diag(key, parts, wide=True)), dict(counts, P=P), wide=True)


def _reduce_assimilation(ranks, sim, ids, P, T, cols, a, label, keep_points):
    """The datasets and the closing lines of the particle filter and the EnKF (``a``: the run's :class:`Assimilation`),
    owner by owner: its own table placed once, the slots it assimilated taken from that, then its sensors', its
    window's and the noise field's tables, one collective each.  Every rank takes the same path."""
    import numpy as np
    where = (ranks, sim, ids, P, T, cols.dim_d)
    out, lines = {}, []
    for owner, settings in (("filter", a.filt), ("enkf", a.enkf)):
        stride = settings[0]
        if not stride:
            continue
        table = _placed_table(*where, stride, owner)
        slots = np.flatnonzero((table[..., 0] > 0).any(axis=0))         # the owner's filter_rows / enkf_rows
        if owner == "filter":
            parts = [_reduce_filter(*where, table, a, label, keep_points),
                     _reduce_sm(*where, stride, a.frecord, slots, label, keep_points, owner),
                     _reduce_window(*where, stride, a.fwindow, slots, label, keep_points, cols.z[0], owner)]
        else:
            parts = [_reduce_enkf(ranks, table, a.enkf, label, keep_points, cols.z[0]),
                     (_enkf_method_arrays(a.enkf, a.scheme), None),
                     _reduce_sm(*where, stride, a.record, slots, label, keep_points, owner),
                     _reduce_window(*where, stride, a.window, slots, label, keep_points, cols.z[0], owner),
                     _reduce_enkf_noise(*where, a.enkf, a.noise_alpha, label, keep_points),
                     _reduce_enkf_forcing(ranks, sim, ids, P, T, a.enkf, a.forcing_alpha, label, keep_points)]
        for datasets, line in parts:
            out.update(datasets)
            lines.append(line)
    return out, lines


NOISE_CORRELATION_KEYS = ("Length_cm", "Layers")


def noise_correlation_settings(ens):
    """Ensemble.Noise_Correlation -> {"length_cm": l, "layers": bool} (the ``noise_correlation=`` argument of
    EnsembleSimulation / SweepSimulation), or None when the key is absent.  Pure: runs before any GPU call, and a bad value
    is a ValueError (message + exit status 1).  Refused with ``"Noise": "numpy"`` (such a run shapes its own vectors) and with
    ``Filter.Rejuvenation`` (its jitter is white per node and would erode the correlation)."""
    import math
    from numbers import Real
    if "Noise_Correlation" not in ens:
        return None
    block = ens["Noise_Correlation"]
    if not isinstance(block, dict):
        raise ValueError(f" Ensemble: Noise_Correlation = {block!r} must be an object such as "
                         f"{{\"Length_cm\": 50.0, \"Layers\": true}}.")
    unknown = sorted(set(block) - set(NOISE_CORRELATION_KEYS))
    if unknown:
        raise ValueError(f" Ensemble: Noise_Correlation has unknown keys {unknown} (known: {list(NOISE_CORRELATION_KEYS)}).")
    length = block.get("Length_cm")
    if isinstance(length, bool) or not isinstance(length, Real) or not math.isfinite(length) or not length > 0:
        raise ValueError(f" Ensemble: Noise_Correlation.Length_cm = {length!r} must be a finite number > 0 (cm).")
    layers = block.get("Layers", False)
    if not isinstance(layers, bool):
        raise ValueError(f" Ensemble: Noise_Correlation.Layers = {layers!r} must be true or false.")
    if str(ens.get("Noise", "philox")).lower() != "philox":
        raise ValueError(f" Ensemble: Noise_Correlation with \"Noise\": {ens.get('Noise')!r}: the correlation shapes the Philox "
                         f"source's vectors; a NumPy stream's caller shapes its own.")
    filt = ens.get("Filter")
    if isinstance(filt, dict) and "Rejuvenation" in filt:
        raise ValueError(" Ensemble: Noise_Correlation and Filter.Rejuvenation exclude each other: the jitter is white per "
                         "node and would erode the correlation by a share h^2 per move.")
    return {"length_cm": float(length), "layers": layers}


def _noise_correlation_arrays(corr, cols_list, label, keep_points):
    """The datasets and the closing line of a run with a noise correlation: the tables are the points' own (every rank
    builds the same ones: no collective)."""
    import numpy as np
    from .stepper import noise_correlation_breaks, noise_correlation_tables
    if corr is None:
        return {}, None
    a = np.stack([noise_correlation_tables(c.z, corr["length_cm"],
                                           noise_correlation_breaks(c.layers, c.z) if corr["layers"] else ())[0]
                  for c in cols_list])
    out = {"noise_correlation_length_cm": np.array(corr["length_cm"], dtype=np.float64),
           "noise_correlation_layers": np.array(1 if corr["layers"] else 0, dtype=np.int8),
           "noise_correlation_a": a if keep_points else a[0]}
    line = f" [{label}] noise correlation: length {corr['length_cm']:g} cm, {int((a[:, 1:] == 0.0).sum())} breaks"
    return out, line


FORCING_PERTURBATION_KEYS = ("Precipitation_Sigma", "Demand_Sigma", "Correlation_Days", "Seed", "EnKF")


def forcing_perturbation_settings(ens):
    """Ensemble.Forcing_Perturbation -> {"precipitation_sigma", "demand_sigma", "correlation_days", "seed"} (the
    ``forcing_perturbation=`` argument of EnsembleSimulation / SweepSimulation, the seed filled in), or None when the key is
    absent.  Pure: runs before any GPU call, and a bad value is a ValueError (message + exit status 1)."""
    import math
    from numbers import Integral, Real
    if "Forcing_Perturbation" not in ens:
        return None
    block = ens["Forcing_Perturbation"]
    if not isinstance(block, dict):
        raise ValueError(f" Ensemble: Forcing_Perturbation = {block!r} must be an object such as "
                         f"{{\"Precipitation_Sigma\": 0.3, \"Demand_Sigma\": 0.1, \"Correlation_Days\": 3}}.")
    unknown = sorted(set(block) - set(FORCING_PERTURBATION_KEYS))
    if unknown:
        raise ValueError(f" Ensemble: Forcing_Perturbation has unknown keys {unknown} (known: "
                         f"{list(FORCING_PERTURBATION_KEYS)}).")
    if "Precipitation_Sigma" not in block and "Demand_Sigma" not in block:
        raise ValueError(" Ensemble: Forcing_Perturbation needs Precipitation_Sigma or Demand_Sigma.")

    def number(key, lo, hi):
        v = block.get(key, 0.0)
        if isinstance(v, bool) or not isinstance(v, Real) or not math.isfinite(v) or not lo <= v <= hi:
            raise ValueError(f" Ensemble: Forcing_Perturbation.{key} = {v!r} must be a finite number in [{lo:g}, {hi:g}].")
        return float(v)

    out = {"precipitation_sigma": number("Precipitation_Sigma", 0.0, 1.0), "demand_sigma": number("Demand_Sigma", 0.0, 1.0),
           "correlation_days": number("Correlation_Days", 0.0, 365.0)}
    seed = block.get("Seed", ens.get("Seed", 0))
    if isinstance(seed, bool) or not isinstance(seed, Integral) or seed < 0:
        raise ValueError(f" Ensemble: Forcing_Perturbation.Seed = {seed!r} must be an integer >= 0.")
    out["seed"] = int(seed)
    filt = ens.get("Filter")
    if isinstance(filt, dict) and filt.get("Sharded") and filt.get("Stride") and not ens.get("Points"):
        raise ValueError(" Ensemble: Forcing_Perturbation with \"Filter\": {\"Sharded\": true}: the columns the ranks exchange "
                         "do not carry the members' forcing state; run the filter unsharded.")
    alpha = _forcing_enkf_settings(ens, block)
    if alpha is not None:
        out["enkf_relaxation"] = alpha
    return out


def _forcing_enkf_settings(ens, block):
    """Forcing_Perturbation.EnKF -> the relaxation of the forcing state's anomalies in the EnKF's analysis, or None when
    the key is absent or false (the run, its file and its lines are then those of a block without it).  ``true``: the EnKF
    block's ``Relaxation`` (0 without one); ``{"Relaxation": a}``: a.  A ValueError for a value of another type, an unknown
    inner key, a relaxation that is a bool or outside [0, 1], no active EnKF block, and a sharded single-point run."""
    from numbers import Real
    from .stepper import forcing_enkf_settings
    if "EnKF" not in block:
        return None
    value = block["EnKF"]
    if not isinstance(value, (bool, dict)):
        raise ValueError(f" Ensemble: Forcing_Perturbation.EnKF = {value!r} must be true, false or {{\"Relaxation\": a}}.")
    enkf = ens.get("EnKF")
    inherited = enkf.get("Relaxation", 0.0) if isinstance(enkf, dict) else 0.0
    inherited = float(inherited) if isinstance(inherited, Real) and not isinstance(inherited, bool) else 0.0
    try:
        alpha = forcing_enkf_settings(value, inherited if 0.0 <= inherited <= 1.0 else 0.0)
    except ValueError as bad:
        raise ValueError(f" Ensemble: {str(bad)[0].upper()}{str(bad)[1:]}.") from None
    if alpha is None:
        return None
    if ens.get("Filter") is not None and not isinstance(enkf, dict):
        raise ValueError(" Ensemble: Forcing_Perturbation.EnKF with a \"Filter\" block: the particle filter carries the "
                         "members' forcing state already; the key serves the \"EnKF\" block.")
    stride = enkf.get("Stride", 48) if isinstance(enkf, dict) else 0
    if not isinstance(enkf, dict) or (isinstance(stride, Real) and not isinstance(stride, bool) and stride == 0):
        raise ValueError(" Ensemble: Forcing_Perturbation.EnKF needs an active \"EnKF\" block (EnKF.Stride > 0).")
    if enkf.get("Sharded") is True and not ens.get("Points"):
        raise ValueError(" Ensemble: Forcing_Perturbation.EnKF with \"EnKF\": {\"Sharded\": true}: the partials the ranks "
                         "exchange cover psi only, not the forcing state.")
    return alpha


def _reduce_enkf_forcing(ranks, sim, ids, P, T, enkf, forcing_alpha, label, keep_points):
    """The forcing analysis's datasets over the EnKF's analysed rows, the [P][n_arow][9] table placed at this rank's points
    and summed over the ranks like the EnKF's (float64 as int64 bits, one collective), and the closing line (rank 0)."""
    import numpy as np
    from .multigpu import place_points
    from .stepper import ENKF_FORCING_WIDTH, enkf_forcing_summary, stride_rows
    stride = enkf[0]
    if not stride or forcing_alpha is None:
        return {}, None
    shape = (stride_rows(T, stride), ENKF_FORCING_WIDTH)
    local = sim.stepper.enkf_forcing_table().reshape((-1,) + shape) if sim is not None else np.zeros((0,) + shape)
    table = place_points(local[:len(ids)], ids, P, ranks)
    summary = enkf_forcing_summary(table if keep_points else table[0], stride, forcing_alpha)
    out = {"enkf_forcing": np.array(1, dtype=np.int8), "enkf_forcing_relaxation": np.array(forcing_alpha, dtype=np.float64)}
    out.update(("enkf_" + k, summary[k]) for k in ("forcing_prior_mean", "forcing_prior_std", "forcing_post_mean",
                                                    "forcing_post_std", "forcing_rejected"))
    if ranks.rank != 0:
        return out, None
    ratio = summary["forcing_spread_ratio"]
    line = (f" [{label}] EnKF forcing: posterior spread {ratio[0]:.4f} / {ratio[1]:.4f} of prior (precipitation / demand) "
            f"over {int(summary['rows'].size)} rows")
    return out, line


def _forcing_perturbation_arrays(pert, label):
    """The datasets and the closing line of a run with perturbed forcing (every rank holds the same settings: no
    collective)."""
    import numpy as np
    from .stepper import forcing_coefficients
    if pert is None:
        return {}, None
    out = {"forcing_precipitation_sigma": np.array(pert["precipitation_sigma"], dtype=np.float64),
           "forcing_demand_sigma": np.array(pert["demand_sigma"], dtype=np.float64),
           "forcing_correlation_days": np.array(pert["correlation_days"], dtype=np.float64),
           "forcing_phi": np.array(forcing_coefficients(pert["correlation_days"])[0], dtype=np.float64),
           "forcing_seed": np.array(pert["seed"], dtype=np.uint64)}
    line = (f" [{label}] forcing perturbation: precipitation sigma {pert['precipitation_sigma']:g}, demand sigma "
            f"{pert['demand_sigma']:g}, correlation {pert['correlation_days']:g} days")
    return out, line


DEFAULT_QUANTILES = (0.05, 0.25, 0.5, 0.75, 0.95)


def distribution_settings(ens):
    """Ensemble.Distribution -> (stride, quantile levels); (0, None) when absent or off.  Pure: runs before any GPU call,
    and a bad value is a ValueError (message + exit status 1)."""
    import math
    from numbers import Real
    block = ens.get("Distribution")
    if block is None:
        return 0, None
    if not isinstance(block, dict):
        raise ValueError(f" Ensemble: Distribution = {block!r} must be an object such as "
                         f"{{\"Stride\": 48, \"Quantiles\": [0.05, 0.5, 0.95]}}.")
    stride = block.get("Stride", 48)
    if (isinstance(stride, bool) or not isinstance(stride, Real) or not math.isfinite(stride) or stride != int(stride)
            or stride < 0):
        raise ValueError(f" Ensemble: Distribution.Stride = {stride!r} must be a row stride >= 0 (0: off).")
    levels = block.get("Quantiles", list(DEFAULT_QUANTILES))
    if not isinstance(levels, (list, tuple)) or not levels:
        raise ValueError(f" Ensemble: Distribution.Quantiles = {levels!r} must be a non-empty list of levels in [0, 1].")
    if len(levels) > 16:
        raise ValueError(f" Ensemble: Distribution.Quantiles holds {len(levels)} levels; at most 16 are supported.")
    for q in levels:
        if isinstance(q, bool) or not isinstance(q, Real) or not math.isfinite(q):
            raise ValueError(f" Ensemble: Distribution.Quantiles: {q!r} is not a number.")
        if not 0.0 <= q <= 1.0:
            raise ValueError(f" Ensemble: Distribution.Quantiles: {q!r} lies outside [0, 1].")
    stride = int(stride)
    return (stride, tuple(float(q) for q in levels)) if stride else (0, None)


PROFILE_DISTRIBUTION_KEYS = ("Bins", "Quantiles")


def profile_distribution_settings(ens):
    """Ensemble.Profile_Distribution -> (bins, quantile levels); (0, None) when absent.  Pure: runs before any GPU call, and
    a bad value is a ValueError (message + exit status 1).  The histograms live on the profile rows, so the block needs
    ``"Profiles"`` >= 1."""
    import math
    from numbers import Real
    block = ens.get("Profile_Distribution")
    if block is None:
        return 0, None
    if not isinstance(block, dict):
        raise ValueError(f" Ensemble: Profile_Distribution = {block!r} must be an object such as "
                         f"{{\"Bins\": 128, \"Quantiles\": [0.05, 0.5, 0.95]}}.")
    unknown = sorted(set(block) - set(PROFILE_DISTRIBUTION_KEYS))
    if unknown:
        raise ValueError(f" Ensemble: Profile_Distribution has unknown keys {unknown} "
                         f"(known: {list(PROFILE_DISTRIBUTION_KEYS)}).")
    profiles = ens.get("Profiles", 0)
    if (isinstance(profiles, bool) or not isinstance(profiles, Real) or not math.isfinite(profiles)
            or profiles != int(profiles) or profiles < 1):
        raise ValueError(f" Ensemble: Profile_Distribution needs the profile rows: Profiles = {profiles!r} must be a row "
                         f"stride >= 1.")
    bins = block.get("Bins", 128)
    if isinstance(bins, bool) or not isinstance(bins, Real) or bins not in (32, 64, 128):
        raise ValueError(f" Ensemble: Profile_Distribution.Bins = {bins!r} must be 32, 64 or 128.")
    if "Quantiles" not in block:
        raise ValueError(" Ensemble: Profile_Distribution.Quantiles (a list of levels in [0, 1]) is required.")
    levels = block["Quantiles"]
    if not isinstance(levels, (list, tuple)) or not levels:
        raise ValueError(f" Ensemble: Profile_Distribution.Quantiles = {levels!r} must be a non-empty list of levels in "
                         f"[0, 1].")
    if len(levels) > 16:
        raise ValueError(f" Ensemble: Profile_Distribution.Quantiles holds {len(levels)} levels; at most 16 are supported.")
    for q in levels:
        if isinstance(q, bool) or not isinstance(q, Real) or not math.isfinite(q):
            raise ValueError(f" Ensemble: Profile_Distribution.Quantiles: {q!r} is not a number.")
        if not 0.0 <= q <= 1.0:
            raise ValueError(f" Ensemble: Profile_Distribution.Quantiles: {q!r} lies outside [0, 1].")
    return int(bins), tuple(float(q) for q in levels)


STORAGE_KEYS = ("Layers_cm", "Bins", "Quantiles")


def storage_settings(ens):
    """Ensemble.Storage -> (layers_cm, bins, quantile levels or None); None when absent.  Pure: runs before any GPU call,
    and a bad value is a ValueError (message + exit status 1).  The tables live on the profile rows, so the block needs
    ``"Profiles"`` >= 1.  ``Bins`` is optional (0: moments only); ``Quantiles`` needs it."""
    import math
    from numbers import Real
    block = ens.get("Storage")
    if block is None:
        return None
    if not isinstance(block, dict):
        raise ValueError(f" Ensemble: Storage = {block!r} must be an object such as "
                         f"{{\"Layers_cm\": [[0, 100], [100, 300]], \"Bins\": 128, \"Quantiles\": [0.05, 0.5, 0.95]}}.")
    unknown = sorted(set(block) - set(STORAGE_KEYS))
    if unknown:
        raise ValueError(f" Ensemble: Storage has unknown keys {unknown} (known: {list(STORAGE_KEYS)}).")
    profiles = ens.get("Profiles", 0)
    if (isinstance(profiles, bool) or not isinstance(profiles, Real) or not math.isfinite(profiles)
            or profiles != int(profiles) or profiles < 1):
        raise ValueError(f" Ensemble: Storage needs the profile rows: Profiles = {profiles!r} must be a row stride >= 1.")
    layers = block.get("Layers_cm")
    if not isinstance(layers, (list, tuple)) or not 1 <= len(layers) <= 8:
        raise ValueError(f" Ensemble: Storage.Layers_cm = {layers!r} must be a list of 1 to 8 [top, bottom] pairs in cm.")
    for lay in layers:
        if (not isinstance(lay, (list, tuple)) or len(lay) != 2
                or any(isinstance(v, bool) or not isinstance(v, Real) or not math.isfinite(v) for v in lay)):
            raise ValueError(f" Ensemble: Storage.Layers_cm: {lay!r} is not a [top, bottom] pair of numbers in cm.")
        if not lay[0] < lay[1]:
            raise ValueError(f" Ensemble: Storage.Layers_cm: {lay!r} must have top < bottom.")
    bins = block.get("Bins", 0)
    if "Bins" in block and (isinstance(bins, bool) or not isinstance(bins, Real) or bins not in (32, 64, 128, 256, 512, 1024)):
        raise ValueError(f" Ensemble: Storage.Bins = {bins!r} must be a power of two in 32 .. 1024.")
    if "Quantiles" in block and not bins:
        raise ValueError(" Ensemble: Storage.Quantiles needs Storage.Bins (the bands come from the histogram).")
    levels = None
    if bins:
        levels = block.get("Quantiles", list(DEFAULT_QUANTILES))
        if not isinstance(levels, (list, tuple)) or not levels:
            raise ValueError(f" Ensemble: Storage.Quantiles = {levels!r} must be a non-empty list of levels in [0, 1].")
        if len(levels) > 16:
            raise ValueError(f" Ensemble: Storage.Quantiles holds {len(levels)} levels; at most 16 are supported.")
        for q in levels:
            if isinstance(q, bool) or not isinstance(q, Real) or not math.isfinite(q):
                raise ValueError(f" Ensemble: Storage.Quantiles: {q!r} is not a number.")
            if not 0.0 <= q <= 1.0:
                raise ValueError(f" Ensemble: Storage.Quantiles: {q!r} lies outside [0, 1].")
        levels = tuple(float(q) for q in levels)
    return tuple((float(a), float(b)) for a, b in layers), int(bins), levels


def storage_ranges(storage, cols):
    """The node ranges of the block's layers on the column's grid (stepper.layer_ranges), with its refusals in the CLI's
    words: a layer that holds no node, or one of 4096 cm or more.  None without a block."""
    from .stepper import STORAGE_MAX_CM, layer_ranges
    if storage is None:
        return None
    try:
        ranges = layer_ranges(cols.z, storage[0])
    except ValueError as bad:
        raise ValueError(f" Ensemble: Storage.Layers_cm: {bad}.") from None
    for lay, (i0, i1) in zip(storage[0], ranges):
        if (int(i1) - int(i0)) * float(cols.dz) >= STORAGE_MAX_CM:
            raise ValueError(f" Ensemble: Storage.Layers_cm: {list(lay)!r} holds {(int(i1) - int(i0)) * float(cols.dz):g} cm "
                             f"of column; a layer must stay below {STORAGE_MAX_CM:g} cm.")
    return ranges


CONDUCTIVITY_KEYS = ("Layers_cm",)


def conductivity_settings(ens):
    """Ensemble.Conductivity -> the layers ((top, bottom), ...) in cm, () for none; None when absent or ``false``.  Pure:
    runs before any GPU call, and a bad value is a ValueError (message + exit status 1).  The table lives on the profile
    rows, so the key needs ``"Profiles"`` >= 1."""
    import math
    from numbers import Real
    block = ens.get("Conductivity")
    if block is None or block is False:
        return None
    if block is not True and not isinstance(block, dict):
        raise ValueError(f" Ensemble: Conductivity = {block!r} must be true or an object such as "
                         f"{{\"Layers_cm\": [[0, 100], [100, 300]]}}.")
    block = {} if block is True else block
    unknown = sorted(set(block) - set(CONDUCTIVITY_KEYS))
    if unknown:
        raise ValueError(f" Ensemble: Conductivity has unknown keys {unknown} (known: {list(CONDUCTIVITY_KEYS)}).")
    profiles = ens.get("Profiles", 0)
    if (isinstance(profiles, bool) or not isinstance(profiles, Real) or not math.isfinite(profiles)
            or profiles != int(profiles) or profiles < 1):
        raise ValueError(f" Ensemble: Conductivity needs the profile rows: Profiles = {profiles!r} must be a row stride >= 1.")
    if "Layers_cm" not in block:
        return ()
    layers = block["Layers_cm"]
    if not isinstance(layers, (list, tuple)) or not 1 <= len(layers) <= 8:
        raise ValueError(f" Ensemble: Conductivity.Layers_cm = {layers!r} must be a list of 1 to 8 [top, bottom] pairs in cm.")
    for lay in layers:
        if (not isinstance(lay, (list, tuple)) or len(lay) != 2
                or any(isinstance(v, bool) or not isinstance(v, Real) or not math.isfinite(v) for v in lay)):
            raise ValueError(f" Ensemble: Conductivity.Layers_cm: {lay!r} is not a [top, bottom] pair of numbers in cm.")
        if not lay[0] < lay[1]:
            raise ValueError(f" Ensemble: Conductivity.Layers_cm: {lay!r} must have top < bottom.")
    return tuple((float(a), float(b)) for a, b in layers)


def conductivity_layer_ranges(cond, cols):
    """The node ranges of the key's layers on the column's grid (stepper.conductivity_ranges), with its refusals in the
    CLI's words: a layer that holds no node, or one of 4096 cm or more.  None without the key."""
    from .stepper import conductivity_ranges
    if cond is None:
        return None
    try:
        return conductivity_ranges(cols.z, cols.dz, cond)
    except ValueError as bad:
        raise ValueError(f" Ensemble: Conductivity.Layers_cm: {bad}.") from None


COVARIANCE_KEYS = ("Node_Stride", "Sensor_Sigma")
COVARIANCE_MAX_BYTES = 1 << 31


def covariance_settings(ens):
    """Ensemble.Covariance -> (node stride, sensor sigma or None); None when absent.  Pure: runs before any GPU call, and a
    bad value is a ValueError (message + exit status 1).  The table lives on the profile rows, so the block needs
    ``"Profiles"`` >= 1.  ``Node_Stride`` defaults to 1; ``Sensor_Sigma`` [m3/m3] is optional."""
    import math
    from numbers import Real
    block = ens.get("Covariance")
    if block is None:
        return None
    if not isinstance(block, dict):
        raise ValueError(f" Ensemble: Covariance = {block!r} must be an object such as "
                         f"{{\"Node_Stride\": 4, \"Sensor_Sigma\": 0.02}}.")
    unknown = sorted(set(block) - set(COVARIANCE_KEYS))
    if unknown:
        raise ValueError(f" Ensemble: Covariance has unknown keys {unknown} (known: {list(COVARIANCE_KEYS)}).")
    profiles = ens.get("Profiles", 0)
    if (isinstance(profiles, bool) or not isinstance(profiles, Real) or not math.isfinite(profiles)
            or profiles != int(profiles) or profiles < 1):
        raise ValueError(f" Ensemble: Covariance needs the profile rows: Profiles = {profiles!r} must be a row stride >= 1.")
    s = block.get("Node_Stride", 1)
    if isinstance(s, bool) or not isinstance(s, Real) or not math.isfinite(s) or s != int(s) or s < 1:
        raise ValueError(f" Ensemble: Covariance.Node_Stride = {s!r} must be a whole number of nodes >= 1.")
    sigma = block.get("Sensor_Sigma")
    if sigma is not None and (isinstance(sigma, bool) or not isinstance(sigma, Real) or not math.isfinite(sigma)
                              or not sigma > 0):
        raise ValueError(f" Ensemble: Covariance.Sensor_Sigma = {sigma!r} must be a number > 0 (m3/m3).")
    return int(s), None if sigma is None else float(sigma)


def covariance_check(cov, D, T, stride, P=1):
    """The block's refusals that need the column and the record: a node stride beyond the column, a ``theta_cov`` dataset
    above 2 GiB and a table beyond the library's HC_THETA_COV_MAX_WORDS, in the CLI's words.  Returns the selected nodes'
    count n (None without a block)."""
    from .stepper import THETA_COV_MAX_WORDS, stride_rows, theta_cov_shape
    if cov is None:
        return None
    if cov[0] > D:
        raise ValueError(f" Ensemble: Covariance.Node_Stride = {cov[0]} exceeds the column's {D} nodes.")
    n, _, W = theta_cov_shape(D, cov[0])
    t_out = stride_rows(T, stride)
    size = int(P) * t_out * n * n * 8
    if size > COVARIANCE_MAX_BYTES or int(P) * t_out * W > THETA_COV_MAX_WORDS:
        raise ValueError(f" Ensemble: Covariance: theta_cov would hold {t_out} rows of {n} x {n} float64 "
                         f"({size / 2 ** 30:.1f} GiB; at most 2 GiB): take a larger node stride or a larger profile stride.")
    return n


PERIOD_KEYS = ("Rows", "Calendar", "Shallower_than_cm", "Bins", "Transpiration_max_cm", "Lateral_flow_max_cm", "Quantiles",
               "Uptake")
UPTAKE_KEYS = ("Layers_cm", "Bins", "Quantiles")


def uptake_settings(ens):
    """Ensemble.Periods.Uptake -> {"layers_cm", "bins", "levels"}; None when absent.  Pure: runs before any GPU call, and
    a bad value is a ValueError (message + exit status 1).  ``Layers_cm`` holds 1 to 8 [top, bottom] pairs in cm; ``Bins``
    is optional (0: moments and the profile only) and ``Quantiles`` needs it.  (The enclosing block's own checks -- among
    them the refusal of a sharded particle filter on a single-point run -- are period_settings'.)"""
    import math
    from numbers import Real
    from .stepper import UPTAKE_MAX_LAYERS
    periods = ens.get("Periods")
    block = periods.get("Uptake") if isinstance(periods, dict) else None
    if block is None:
        return None
    if not isinstance(block, dict):
        raise ValueError(f" Ensemble: Periods.Uptake = {block!r} must be an object such as "
                         f"{{\"Layers_cm\": [[0, 100], [100, 300], [300, 1500]], \"Bins\": 128}}.")
    unknown = sorted(set(block) - set(UPTAKE_KEYS))
    if unknown:
        raise ValueError(f" Ensemble: Periods.Uptake has unknown keys {unknown} (known: {list(UPTAKE_KEYS)}).")
    layers = block.get("Layers_cm")
    if not isinstance(layers, (list, tuple)) or not 1 <= len(layers) <= UPTAKE_MAX_LAYERS:
        raise ValueError(f" Ensemble: Periods.Uptake.Layers_cm = {layers!r} must be a list of 1 to {UPTAKE_MAX_LAYERS} "
                         f"[top, bottom] pairs in cm.")
    for lay in layers:
        ok = isinstance(lay, (list, tuple)) and len(lay) == 2 and all(
            not isinstance(v, bool) and isinstance(v, Real) and math.isfinite(v) for v in lay)
        if not ok or not lay[0] < lay[1]:
            raise ValueError(f" Ensemble: Periods.Uptake.Layers_cm: {lay!r} is not a [top, bottom] pair in cm with top < bottom.")
    bins = block.get("Bins", 0)
    if "Bins" in block and (isinstance(bins, bool) or not isinstance(bins, Real) or bins not in (32, 64, 128, 256, 512, 1024)):
        raise ValueError(f" Ensemble: Periods.Uptake.Bins = {bins!r} must be a power of two in 32 .. 1024.")
    if "Quantiles" in block and not bins:
        raise ValueError(" Ensemble: Periods.Uptake.Quantiles needs Periods.Uptake.Bins (it belongs to the histograms).")
    levels = None
    if bins:
        levels = block.get("Quantiles", [0.05, 0.5, 0.95])
        if not isinstance(levels, (list, tuple)) or not levels or len(levels) > 16:
            raise ValueError(f" Ensemble: Periods.Uptake.Quantiles = {levels!r} must be a list of 1 to 16 levels in [0, 1].")
        for q in levels:
            if isinstance(q, bool) or not isinstance(q, Real) or not math.isfinite(q) or not 0.0 <= q <= 1.0:
                raise ValueError(f" Ensemble: Periods.Uptake.Quantiles: {q!r} is not a level in [0, 1].")
        levels = tuple(float(q) for q in levels)
    return {"layers_cm": tuple((float(a), float(b)) for a, b in layers), "bins": int(bins), "levels": levels}


def uptake_plan(uptake, cols_list):
    """The layers' midpoint-cell ranges on the column (stepper.layer_cells), with the refusals in the CLI's words: ET off
    (there is no uptake), a layer that holds no midpoint, a layer that holds no root cell of some point.  None without a
    block.  Before any GPU call."""
    from .stepper import layer_cells
    if uptake is None:
        return None
    cols = cols_list[0]
    if not all(c.flags["ET"] for c in cols_list):
        raise ValueError(" Ensemble: Periods.Uptake needs the evapo-transpiration (Simulation_Flags.ET is off: there is no "
                         "root-water uptake to record).")
    try:
        cells = layer_cells(cols.z, uptake["layers_cm"])
    except ValueError as bad:
        raise ValueError(f" Ensemble: Periods.Uptake.Layers_cm: {bad}.") from None
    for c in cols_list:
        first = 0 if c.n_root_first else 1
        for lay, (lo, hi) in zip(uptake["layers_cm"], cells):
            if not (lo <= c.n_root_int and hi > first):
                raise ValueError(f" Ensemble: Periods.Uptake.Layers_cm: layer {list(lay)!r} cm holds no root cell (the root "
                                 f"zone ends at {float(c.z[c.n_root_int] + c.dz):g} cm).")
    return cells


def period_settings(ens):
    """Ensemble.Periods -> {"rows", "calendar", "thresholds_cm", "bins", "flux_max_cm", "levels"}; None when absent.
    Pure: runs before any GPU call, and a bad value is a ValueError (message + exit status 1).  Exactly one of ``Rows`` and
    ``Calendar``; ``Bins`` is optional (0: moments only), and ``Quantiles`` and the two ``..._max_cm`` keys need it.
    Refused with a sharded particle filter on a single-point run."""
    import math
    from numbers import Real
    from .stepper import PERIOD_MAX_ROWS, PERIOD_MAX_THRESHOLDS, flux_max_log2_of
    block = ens.get("Periods")
    if block is None:
        return None
    if not isinstance(block, dict):
        raise ValueError(f" Ensemble: Periods = {block!r} must be an object such as "
                         f"{{\"Rows\": 1440, \"Shallower_than_cm\": [100, 200], \"Bins\": 128}}.")
    unknown = sorted(set(block) - set(PERIOD_KEYS))
    if unknown:
        raise ValueError(f" Ensemble: Periods has unknown keys {unknown} (known: {list(PERIOD_KEYS)}).")
    if ("Rows" in block) == ("Calendar" in block):
        raise ValueError(" Ensemble: Periods needs exactly one of Rows (a period every so many rows) and Calendar "
                         "(\"month\" or \"year\").")
    rows = calendar = None
    if "Rows" in block:
        rows = block["Rows"]
        if (isinstance(rows, bool) or not isinstance(rows, Real) or not math.isfinite(rows) or rows != int(rows)
                or not 1 <= rows <= PERIOD_MAX_ROWS):
            raise ValueError(f" Ensemble: Periods.Rows = {rows!r} must be a whole number of rows in 1 .. {PERIOD_MAX_ROWS}.")
        rows = int(rows)
    else:
        calendar = block["Calendar"]
        if calendar not in ("month", "year"):
            raise ValueError(f" Ensemble: Periods.Calendar = {calendar!r} must be \"month\" or \"year\".")
    depths = block.get("Shallower_than_cm", [])
    if not isinstance(depths, (list, tuple)) or len(depths) > PERIOD_MAX_THRESHOLDS:
        raise ValueError(f" Ensemble: Periods.Shallower_than_cm = {depths!r} must be a list of at most "
                         f"{PERIOD_MAX_THRESHOLDS} depths in cm.")
    for d in depths:
        if isinstance(d, bool) or not isinstance(d, Real) or not math.isfinite(d):
            raise ValueError(f" Ensemble: Periods.Shallower_than_cm: {d!r} is not a depth in cm.")
    bins = block.get("Bins", 0)
    if "Bins" in block and (isinstance(bins, bool) or not isinstance(bins, Real) or bins not in (32, 64, 128, 256, 512, 1024)):
        raise ValueError(f" Ensemble: Periods.Bins = {bins!r} must be a power of two in 32 .. 1024.")
    for key in ("Quantiles", "Transpiration_max_cm", "Lateral_flow_max_cm"):
        if key in block and not bins:
            raise ValueError(f" Ensemble: Periods.{key} needs Periods.Bins (it belongs to the histograms).")
    levels = flux_max = None
    if bins:
        flux_max = []
        for key, default in (("Transpiration_max_cm", 16), ("Lateral_flow_max_cm", 4)):
            v = block.get(key, default)
            try:
                if isinstance(v, bool) or not isinstance(v, Real):
                    raise ValueError
                flux_max_log2_of(v)
            except ValueError:
                raise ValueError(f" Ensemble: Periods.{key} = {v!r} must be a power of two in 2^-8 .. 2^12 cm.") from None
            flux_max.append(float(v))
        levels = block.get("Quantiles", list(DEFAULT_QUANTILES))
        if not isinstance(levels, (list, tuple)) or not levels:
            raise ValueError(f" Ensemble: Periods.Quantiles = {levels!r} must be a non-empty list of levels in [0, 1].")
        if len(levels) > 16:
            raise ValueError(f" Ensemble: Periods.Quantiles holds {len(levels)} levels; at most 16 are supported.")
        for q in levels:
            if isinstance(q, bool) or not isinstance(q, Real) or not math.isfinite(q):
                raise ValueError(f" Ensemble: Periods.Quantiles: {q!r} is not a number.")
            if not 0.0 <= q <= 1.0:
                raise ValueError(f" Ensemble: Periods.Quantiles: {q!r} lies outside [0, 1].")
        levels = tuple(float(q) for q in levels)
    filt = ens.get("Filter")
    if isinstance(filt, dict) and filt.get("Sharded") and filt.get("Stride") and not ens.get("Points"):
        raise ValueError(" Ensemble: Periods with \"Filter\": {\"Sharded\": true}: the columns the ranks exchange do not carry "
                         "the members' period accumulators; run the filter unsharded.")
    return {"rows": rows, "calendar": calendar, "thresholds_cm": tuple(float(d) for d in depths), "bins": int(bins),
            "flux_max_cm": None if flux_max is None else tuple(flux_max), "levels": levels}


def period_plan(periods, cols, forcing, run_rows):
    """(end rows, threshold nodes) of the block on this record and column (stepper.period_ends, stepper.sensor_nodes), with
    their refusals in the CLI's words: a depth outside the column, no period that ends within the run's rows, too many or
    too long periods.  Periods that end after the run's last row are dropped.  None without a block."""
    from .stepper import PERIOD_MAX_PERIODS, PERIOD_MAX_ROWS, period_ends, sensor_nodes
    import numpy as np
    if periods is None:
        return None
    try:
        nodes = sensor_nodes(cols.z, periods["thresholds_cm"])
    except ValueError as bad:
        raise ValueError(f" Ensemble: Periods.Shallower_than_cm: {bad}.") from None
    if periods["rows"] is not None:
        ends = period_ends(forcing.dim_t, rows=periods["rows"])
    else:
        ends = period_ends(forcing.dim_t, datenum=forcing.datenum, calendar=periods["calendar"])
    ends = ends[ends <= int(run_rows)]
    if ends.size == 0:
        raise ValueError(f" Ensemble: Periods: no period ends within the run's {int(run_rows)} rows.")
    if ends.size > PERIOD_MAX_PERIODS:
        raise ValueError(f" Ensemble: Periods: {ends.size} periods; at most {PERIOD_MAX_PERIODS} are supported.")
    longest = int(np.diff(np.concatenate([[0], ends])).max())
    if longest > PERIOD_MAX_ROWS:
        raise ValueError(f" Ensemble: Periods: a period of {longest} rows; at most {PERIOD_MAX_ROWS} are supported.")
    return ends, nodes


FILTER_KEYS = ("Stride", "Sigma_cm", "Seed", "Sharded", "Soil_Moisture", "ESS_floor", "Window_Offsets", "Rejuvenation",
               "Smoother")


def filter_settings(ens, n_gpus=1):
    """Ensemble.Filter -> (stride, sigma_cm, seed or None = the ensemble's seed); (0, None, None) when absent or off.  Pure:
    runs before any GPU call, and a bad value is a ValueError (message + exit status 1).  A single-point ensemble on more
    than one GPU is refused -- resampling would have to move states between ranks -- unless the block says
    ``"Sharded": true`` (:func:`filter_sharded`).  ``ESS_floor`` (:func:`filter_ess_floor`) is checked here too;
    ``Window_Offsets`` by :func:`filter_window_settings`; ``Rejuvenation`` (:func:`filter_rejuvenation`) here."""
    import math
    from numbers import Integral, Real
    if "ESS_floor" in ens:
        raise ValueError(" Ensemble: ESS_floor belongs inside the \"Filter\" block.")
    if "Rejuvenation" in ens:
        raise ValueError(" Ensemble: Rejuvenation belongs inside the \"Filter\" block.")
    if "Window_Offsets" in ens:
        raise ValueError(" Ensemble: Window_Offsets belongs inside the \"Filter\" or the \"EnKF\" block.")
    block = ens.get("Filter")
    if block is None:
        return 0, None, None
    if not isinstance(block, dict):
        raise ValueError(f" Ensemble: Filter = {block!r} must be an object such as "
                         f"{{\"Stride\": 48, \"Sigma_cm\": 10.0}}.")
    unknown = sorted(set(block) - set(FILTER_KEYS))
    if unknown:
        raise ValueError(f" Ensemble: Filter has unknown keys {unknown} (known: {list(FILTER_KEYS)}).")
    stride = block.get("Stride", 48)
    if (isinstance(stride, bool) or not isinstance(stride, Real) or not math.isfinite(stride) or stride != int(stride)
            or stride < 0 or stride > (1 << 31) - 1):
        raise ValueError(f" Ensemble: Filter.Stride = {stride!r} must be a row stride >= 0 (0: off).")
    if "Sigma_cm" not in block:
        raise ValueError(" Ensemble: Filter.Sigma_cm (the observation error of the well, cm) is required.")
    sigma = block["Sigma_cm"]
    if isinstance(sigma, bool) or not isinstance(sigma, Real) or not math.isfinite(sigma) or not sigma > 0:
        raise ValueError(f" Ensemble: Filter.Sigma_cm = {sigma!r} must be a finite number > 0.")
    seed = block.get("Seed")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, Integral) or not 0 <= seed < (1 << 64)):
        raise ValueError(f" Ensemble: Filter.Seed = {seed!r} must be an integer in [0, 2^64).")
    sharded = block.get("Sharded", False)
    if not isinstance(sharded, bool):
        raise ValueError(f" Ensemble: Filter.Sharded = {sharded!r} must be true or false.")
    stride = int(stride)
    if "ESS_floor" in block:
        floor = block["ESS_floor"]
        if isinstance(floor, bool) or not isinstance(floor, Real) or not math.isfinite(floor) or not 0 < floor < 1:
            raise ValueError(f" Ensemble: Filter.ESS_floor = {floor!r} must be a finite number with 0 < ESS_floor < 1.")
        if not stride:
            raise ValueError(" Ensemble: Filter.ESS_floor needs an active filter (Filter.Stride > 0).")
    if "Rejuvenation" in block:
        delta = block["Rejuvenation"]
        if isinstance(delta, bool) or not isinstance(delta, Real) or not math.isfinite(delta) or not 0.5 <= delta < 1:
            raise ValueError(f" Ensemble: Filter.Rejuvenation = {delta!r} must be a finite number with "
                             f"0.5 <= Rejuvenation < 1.")
        if not stride:
            raise ValueError(" Ensemble: Filter.Rejuvenation needs an active filter (Filter.Stride > 0).")
        if sharded and not ens.get("Points"):
            raise ValueError(" Ensemble: Filter.Rejuvenation is not available with \"Sharded\": true: the sharded filter "
                             "gathers the members' water-table indices only, and the moments of the base noise vectors "
                             "would need an exchange of their own.")
    if not stride:
        return 0, None, None
    if not ens.get("Points") and int(n_gpus) > 1 and not sharded:
        raise ValueError(f" Ensemble: Filter with one parameter point runs on one GPU ({n_gpus} requested): resampling "
                         f"would move members between ranks.")
    return stride, float(sigma), (None if seed is None else int(seed))


def filter_ess_floor(ens):
    """Ensemble.Filter.ESS_floor -> the floor f (0 < f < 1) below which the effective sample size of a resampling is not
    allowed to fall, as a fraction of the counted members (include/hydrocol.h hc_set_filter_tempering), or None when the
    key is not given.  Checked by :func:`filter_settings`, which this runs first."""
    filter_settings(ens)
    block = ens.get("Filter")
    if not isinstance(block, dict) or "ESS_floor" not in block:
        return None
    return float(block["ESS_floor"])


def filter_rejuvenation(ens):
    """Ensemble.Filter.Rejuvenation -> Liu & West's discount delta (0.5 <= delta < 1) of the base noise vectors' move after
    a resampling (include/hydrocol.h hc_set_filter_rejuvenation), or None when the key is not given.  Checked by
    :func:`filter_settings`, which this runs first."""
    filter_settings(ens)
    block = ens.get("Filter")
    if not isinstance(block, dict) or "Rejuvenation" not in block:
        return None
    return float(block["Rejuvenation"])


def filter_window_settings(ens):
    """Ensemble.Filter.Window_Offsets -> the offsets as an ascending tuple, or None when the key is absent or the list empty
    (the run, its file and its lines are then those of a block without it).  Pure, like :func:`filter_settings`: a bad
    value is a ValueError (message + exit status 1), by the rules and in the words of :func:`enkf_window_settings`.  Needs
    an active filter; refused together with ``"Sharded": true`` on a single-point run."""
    if "Window_Offsets" in ens:
        raise ValueError(" Ensemble: Window_Offsets belongs inside the \"Filter\" or the \"EnKF\" block.")
    off = _window_settings(ens, "Filter")
    if off and not ens.get("Points") and ens["Filter"].get("Sharded", False):
        raise ValueError(" Ensemble: Filter.Window_Offsets is not available with \"Sharded\": true: the sharded filter "
                         "gathers the members' water-table indices of the assimilation row only.")
    return off


SMOOTHER_KEYS = ("Stride", "Lag_rows", "Quantiles")


def filter_smoother_settings(ens):
    """Ensemble.Filter.Smoother -> (stride, K = Lag_rows / Stride, quantile levels), or None when the block is absent (the
    run, its file and its lines are then those of a Filter block without it).  Pure, like :func:`filter_settings`, which
    this runs first: a bad value is a ValueError (message + exit status 1).  ``Stride`` (default 48) is the row stride of
    the record rows, ``Lag_rows`` (default 0: the analysis) a multiple of it with at most 64 strides, ``Quantiles`` at most
    16 levels in [0, 1] (default 0.05, 0.5, 0.95).  Needs an active filter; refused together with ``"Sharded": true`` on a
    single-point run."""
    import math
    from numbers import Real
    from .stepper import SMOOTHER_MAX_LAG, WTD_MAX_LEVELS
    if "Smoother" in ens:
        raise ValueError(" Ensemble: Smoother belongs inside the \"Filter\" block.")
    filt_stride = filter_settings(ens)[0]
    block = ens.get("Filter")
    if not isinstance(block, dict) or "Smoother" not in block:
        return None
    sm = block["Smoother"]
    if not isinstance(sm, dict):
        raise ValueError(f" Ensemble: Filter.Smoother = {sm!r} must be an object such as "
                         f"{{\"Stride\": 48, \"Lag_rows\": 480}}.")
    unknown = sorted(set(sm) - set(SMOOTHER_KEYS))
    if unknown:
        raise ValueError(f" Ensemble: Filter.Smoother has unknown keys {unknown} (known: {list(SMOOTHER_KEYS)}).")
    stride, lag_rows = sm.get("Stride", 48), sm.get("Lag_rows", 0)
    if (isinstance(stride, bool) or not isinstance(stride, Real) or not math.isfinite(stride) or stride != int(stride)
            or stride < 1 or stride > (1 << 31) - 1):
        raise ValueError(f" Ensemble: Filter.Smoother.Stride = {stride!r} must be a row stride >= 1.")
    if (isinstance(lag_rows, bool) or not isinstance(lag_rows, Real) or not math.isfinite(lag_rows)
            or lag_rows != int(lag_rows) or lag_rows < 0):
        raise ValueError(f" Ensemble: Filter.Smoother.Lag_rows = {lag_rows!r} must be a number of rows >= 0.")
    stride, lag_rows = int(stride), int(lag_rows)
    if lag_rows % stride:
        raise ValueError(f" Ensemble: Filter.Smoother.Lag_rows = {lag_rows} must be a multiple of its Stride = {stride}.")
    if lag_rows // stride > SMOOTHER_MAX_LAG:
        raise ValueError(f" Ensemble: Filter.Smoother.Lag_rows = {lag_rows} is {lag_rows // stride} strides of {stride} "
                         f"rows, at most {SMOOTHER_MAX_LAG}.")
    levels = sm.get("Quantiles", [0.05, 0.5, 0.95])
    if (not isinstance(levels, (list, tuple)) or len(levels) > WTD_MAX_LEVELS
            or any(isinstance(v, bool) or not isinstance(v, Real) or not math.isfinite(v) or not 0.0 <= v <= 1.0
                   for v in levels)):
        raise ValueError(f" Ensemble: Filter.Smoother.Quantiles = {levels!r} must be a list of at most {WTD_MAX_LEVELS} "
                         f"levels in [0, 1].")
    if not filt_stride:
        raise ValueError(" Ensemble: Filter.Smoother needs an active filter (Filter.Stride > 0).")
    if not ens.get("Points") and block.get("Sharded", False):
        raise ValueError(" Ensemble: Filter.Smoother is not available with \"Sharded\": true: the columns the ranks "
                         "exchange do not carry the smoother's ring.")
    return stride, lag_rows // stride, tuple(float(v) for v in levels)


def _reduce_smoother(ranks, sim, ids, P, T, ref, forcing, a, device, label, keep_points):
    """The smoother's datasets and closing line (``a``: the run's :class:`Assimilation`; no smoother: nothing): each
    rank flushes its handle ``sim`` (None: it holds no points), its points' tables are placed at ``ids`` of the run's
    ``P`` and summed over the ranks -- two collectives every rank joins -- and rank 0 forms the summary."""
    import numpy as np
    from .multigpu import place_points
    from .stepper import filter_smoother_summary, stride_rows
    if a.smoother is None:
        return {}, None
    stride, lag, levels = a.smoother
    n_srow, D = stride_rows(T, stride), ref.dim_d
    if sim is not None:
        sim.stepper.filter_smoother_flush()
        lhist, lpaths = sim.stepper.filter_smoother_hist(), sim.stepper.filter_smoother_paths()
    else:
        lhist, lpaths = np.zeros((0, n_srow, D), dtype=np.int32), np.zeros((0, n_srow, 2), dtype=np.int64)
    hist, paths = place_points(lhist, ids, P, ranks), place_points(lpaths, ids, P, ranks)
    if ranks.rank != 0:
        return {}, None
    if not keep_points:
        hist, paths = hist[0], paths[0]
    summ = filter_smoother_summary(hist, paths, forcing.wtd_obs, levels, ref.dz, ref.z, stride, device)
    emitted = np.flatnonzero((np.asarray(summ["lag_rows"]) >= 0).reshape(-1, n_srow).any(axis=0))
    out = {"smooth_rows": summ["rows"][emitted], "smooth_count": summ["count"][..., emitted],
           "smooth_hist": np.asarray(hist, dtype=np.int32)[..., emitted, :],
           "smooth_lag_rows": summ["lag_rows"][..., emitted], "smooth_unique_paths": summ["unique_paths"][..., emitted],
           "smooth_quantile_levels": np.asarray(summ["levels"], dtype=np.float64),
           "smooth_quantile_cm": summ["quantile_cm"][..., emitted, :], "smooth_crps_cm": summ["crps_cm"][..., emitted],
           "smooth_stride": np.array(stride, dtype=np.int64), "smooth_lag": np.array(lag, dtype=np.int64)}
    # the mean over the rows that counted members, per point (as wtd_crps_mean_cm)
    out["smooth_crps_mean_cm"] = np.asarray(summ["crps_mean_cm"], dtype=np.float64)
    solved = np.asarray(out["smooth_count"]) > 0
    n = int(solved.reshape(-1, emitted.size).any(axis=0).sum())
    mean = float(np.asarray(out["smooth_crps_cm"])[solved].mean()) if solved.any() else float("nan")
    fewest = int(np.asarray(out["smooth_unique_paths"])[solved].min()) if solved.any() else 0
    line = (f" [{label}] smoother: CRPS = {mean:.3f} cm at lag {lag * stride} rows over {n} rows, fewest paths {fewest}")
    return out, line


def filter_sharded(ens):
    """Ensemble.Filter.Sharded -> True / False, or None when the key is not given (or the filter is off).  With true a
    single-point ensemble's members are dealt to the GPUs, every assimilation gathers their water-table indices and the
    ranks exchange the columns whose ancestor lives elsewhere, so the run is the one-GPU run to the bit (include/hydrocol.h
    hc_set_filter_shard); a sweep ignores it (its points are dealt whole).  Checked by :func:`filter_settings`."""
    block = ens.get("Filter")
    if not isinstance(block, dict) or "Sharded" not in block or not filter_settings(ens)[0]:
        return None
    return bool(block["Sharded"])


ENKF_KEYS = ("Stride", "Sigma_cm", "Localisation_cm", "Seed", "Soil_Moisture", "Method", "Relaxation", "Window_Offsets",
             "Sharded", "Noise_Field")


def enkf_settings(ens, n_gpus=1):
    """Ensemble.EnKF -> (stride, sigma_cm, localisation_cm, seed or None = the ensemble's seed); (0, None, None, None)
    when absent or off.  Pure: runs before any GPU call, and a bad value is a ValueError (message + exit status 1).  Refused
    together with a "Filter" block, and for a single-point ensemble on more than one GPU (its covariances would need a sum
    over the ranks) unless the block says ``"Sharded": true`` (:func:`enkf_sharded`)."""
    import math
    from numbers import Integral, Real
    block = ens.get("EnKF")
    if block is None:
        return 0, None, None, None
    if not isinstance(block, dict):
        raise ValueError(f" Ensemble: EnKF = {block!r} must be an object such as {{\"Stride\": 48, \"Sigma_cm\": 10.0}}.")
    unknown = sorted(set(block) - set(ENKF_KEYS))
    if unknown:
        raise ValueError(f" Ensemble: EnKF has unknown keys {unknown} (known: {list(ENKF_KEYS)}).")
    stride = block.get("Stride", 48)
    if (isinstance(stride, bool) or not isinstance(stride, Real) or not math.isfinite(stride) or stride != int(stride)
            or stride < 0 or stride > (1 << 31) - 1):
        raise ValueError(f" Ensemble: EnKF.Stride = {stride!r} must be a row stride >= 0 (0: off).")
    if "Sigma_cm" not in block:
        raise ValueError(" Ensemble: EnKF.Sigma_cm (the observation error of the well, cm) is required.")
    sigma = block["Sigma_cm"]
    if isinstance(sigma, bool) or not isinstance(sigma, Real) or not math.isfinite(sigma) or not sigma > 0:
        raise ValueError(f" Ensemble: EnKF.Sigma_cm = {sigma!r} must be a finite number > 0.")
    loc = block.get("Localisation_cm", 0)
    if isinstance(loc, bool) or not isinstance(loc, Real) or not math.isfinite(loc) or not loc >= 0:
        raise ValueError(f" Ensemble: EnKF.Localisation_cm = {loc!r} must be a finite number >= 0 (0: none).")
    seed = block.get("Seed")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, Integral) or not 0 <= seed < (1 << 64)):
        raise ValueError(f" Ensemble: EnKF.Seed = {seed!r} must be an integer in [0, 2^64).")
    stride = int(stride)
    if not stride:
        return 0, None, None, None
    if ens.get("Filter") is not None:
        raise ValueError(" Ensemble: \"Filter\" and \"EnKF\" exclude each other: choose one.")
    sharded = block.get("Sharded", False)
    if not isinstance(sharded, bool):
        raise ValueError(f" Ensemble: EnKF.Sharded = {sharded!r} must be true or false.")
    if not ens.get("Points") and int(n_gpus) > 1 and not sharded:
        raise ValueError(f" Ensemble: EnKF with one parameter point runs on one GPU ({n_gpus} requested): its "
                         f"covariances would need a sum over the ranks.")
    return stride, float(sigma), float(loc), (None if seed is None else int(seed))


def enkf_sharded(ens):
    """Ensemble.EnKF.Sharded -> True / False, or None when the key is not given (or the EnKF is off).  With true a
    single-point ensemble's members are dealt to the GPUs in whole tiles of 256 and every analysis gathers the ranks' tile
    partials, so the run is the one-GPU run to the bit (include/hydrocol.h hc_set_enkf_shard); a sweep ignores it (its
    points are dealt whole).  Checked by :func:`enkf_settings`."""
    block = ens.get("EnKF")
    if not isinstance(block, dict) or "Sharded" not in block or not enkf_settings(ens)[0]:
        return None
    return bool(block["Sharded"])


ENKF_METHOD_NAMES = ("stochastic", "sqrt")


def enkf_method_settings(ens):
    """Ensemble.EnKF.Method / Relaxation -> (method, relaxation), or None when neither key is given (the run and its
    file are then those of a block without them).  Pure, like :func:`enkf_settings`: a bad value is a ValueError (message
    + exit status 1).  Needs an active EnKF."""
    import math
    from numbers import Real
    block = ens.get("EnKF")
    if not isinstance(block, dict) or ("Method" not in block and "Relaxation" not in block):
        return None
    method = block.get("Method", "stochastic")
    if not isinstance(method, str) or method not in ENKF_METHOD_NAMES:
        raise ValueError(f" Ensemble: EnKF.Method = {method!r} must be one of {list(ENKF_METHOD_NAMES)}.")
    alpha = block.get("Relaxation", 0.0)
    if isinstance(alpha, bool) or not isinstance(alpha, Real) or not math.isfinite(alpha) or not 0 <= alpha <= 1:
        raise ValueError(f" Ensemble: EnKF.Relaxation = {alpha!r} must be a finite number in [0, 1] (0: none).")
    stride = block.get("Stride", 48)
    if isinstance(stride, Real) and not isinstance(stride, bool) and stride == 0:
        raise ValueError(" Ensemble: EnKF.Method / EnKF.Relaxation need an active EnKF (EnKF.Stride > 0).")
    return method, float(alpha)


def enkf_noise_settings(ens):
    """Ensemble.EnKF.Noise_Field -> the relaxation of the noise field's anomalies, or None when the key is absent or false
    (the run, its file and its lines are then those of a block without it).  ``true``: the block's ``Relaxation`` (0
    without one); ``{"Relaxation": a}``: a.  Pure, like :func:`enkf_settings`: a bad value is a ValueError (message + exit
    status 1): a value that is neither a bool nor an object with the one key ``Relaxation``; a relaxation outside [0, 1]
    or a bool; a block whose Stride is 0; ``"Sharded": true`` on a single-point run (a sweep ignores Sharded)."""
    from numbers import Real
    from .stepper import noise_field_settings
    block = ens.get("EnKF")
    if not isinstance(block, dict) or "Noise_Field" not in block:
        if "Noise_Field" in ens:
            raise ValueError(" Ensemble: Noise_Field belongs inside the \"EnKF\" block.")
        return None
    inherited = block.get("Relaxation", 0.0)
    inherited = float(inherited) if isinstance(inherited, Real) and not isinstance(inherited, bool) else 0.0
    value = block["Noise_Field"]
    if value is None or (isinstance(value, dict) and list(value) != ["Relaxation"]):
        raise ValueError(f" Ensemble: EnKF.Noise_Field = {value!r} must be true, false or {{\"Relaxation\": a}}.")
    try:
        alpha = noise_field_settings(value, inherited if 0.0 <= inherited <= 1.0 else 0.0)
    except ValueError as bad:
        raise ValueError(f" Ensemble: EnKF.{bad}.") from None
    if alpha is None:
        return None
    stride = block.get("Stride", 48)
    if isinstance(stride, Real) and not isinstance(stride, bool) and stride == 0:
        raise ValueError(" Ensemble: EnKF.Noise_Field needs an active EnKF (EnKF.Stride > 0).")
    if block.get("Sharded") is True and not ens.get("Points"):
        raise ValueError(" Ensemble: EnKF.Noise_Field with \"Sharded\": true: the partials the ranks exchange cover psi "
                         "only, not the noise field.")
    return alpha


def _reduce_enkf_noise(ranks, sim, ids, P, T, D, enkf, noise_alpha, label, keep_points):
    """The noise field's datasets from this rank's handle over the EnKF's analysed rows (its ``enkf_rows``), the [P]
    table placed and summed over the ranks like the EnKF's (float64 as int64 bits), and the closing line (rank 0)."""
    import numpy as np
    from .stepper import enkf_noise_summary
    stride = enkf[0]
    if not stride or noise_alpha is None:
        return {}, None
    table = _placed_table(ranks, sim, ids, P, T, D, stride, "enkf_noise")
    summary = enkf_noise_summary(table if keep_points else table[0], stride, noise_alpha, D)
    out = {"enkf_noise_field": np.array(1, dtype=np.int8), "enkf_noise_relaxation": np.array(noise_alpha, dtype=np.float64)}
    out.update(("enkf_" + k, summary[k]) for k in ("noise_prior_mean", "noise_prior_std", "noise_post_mean",
                                                    "noise_post_std", "noise_rejected"))
    if ranks.rank != 0:
        return out, None
    line = (f" [{label}] EnKF noise field: posterior spread {summary['noise_spread_ratio']:.4f} of prior over "
            f"{int(summary['rows'].size)} rows")
    return out, line


def enkf_window_settings(ens):
    """Ensemble.EnKF.Window_Offsets -> the offsets as an ascending tuple, or None when the key is absent or the list empty
    (the run, its file and its lines are then those of a block without it).  Pure, like :func:`enkf_settings`: a bad
    value is a ValueError (message + exit status 1): not a list; an entry that is not an integer (a boolean, a float) or
    outside [1, Stride); a repeated entry; more than 8, alone or together with the Soil_Moisture depths.  Needs an active
    EnKF."""
    return _window_settings(ens, "EnKF")


def _window_settings(ens, owner):
    """The body of :func:`enkf_window_settings` (``owner`` = "EnKF") and :func:`filter_window_settings` ("Filter"): the
    owner's block read, its offsets checked against its stride and its Soil_Moisture depths."""
    from numbers import Real
    from . import stepper
    window_of = stepper.enkf_window_settings if owner == "EnKF" else stepper.filter_window_settings
    block = ens.get(owner)
    if not isinstance(block, dict) or block.get("Window_Offsets") is None:
        return None
    stride = block.get("Stride", 48)
    stride = int(stride) if isinstance(stride, Real) and not isinstance(stride, bool) and stride == int(stride) else 0
    if not stride:
        what = "EnKF" if owner == "EnKF" else "filter"
        raise ValueError(f" Ensemble: {owner}.Window_Offsets needs an active {what} ({owner}.Stride > 0).")
    sm = block.get("Soil_Moisture")
    depths = sm.get("Depths_cm") if isinstance(sm, dict) else None
    try:
        off = window_of(block["Window_Offsets"], stride, len(depths) if isinstance(depths, (list, tuple)) else 0)
    except ValueError as bad:
        raise ValueError(f" Ensemble: {bad}.") from None
    return off or None


def _reduce_window(ranks, sim, ids, P, T, D, stride, window, slots, label, keep_points, z0_cm, owner):
    """The window's datasets (``owner``: "enkf" or "filter", the prefix of the datasets and of the handle's table) from
    this rank's handle over the owner's assimilated ``slots`` (its ``enkf_rows`` / ``filter_rows``), the [P] table placed
    and summed over the ranks like the owner's, and the closing line (rank 0).  The EnKF's has the innovation too."""
    import numpy as np
    if not stride or not window:
        return {}, None
    table = _placed_table(ranks, sim, ids, P, T, D, stride, owner + "_window", len(window))
    sel = table[:, slots] if keep_points else table[0, slots]
    observed = sel[..., 0] == 1.0
    out = {f"{owner}_window_offsets": np.asarray(window, dtype=np.int64),
           f"{owner}_window_observed": observed.astype(np.int8), f"{owner}_window_obs_cm": sel[..., 1] + float(z0_cm),
           f"{owner}_window_prior_mean_cm": sel[..., 2] + float(z0_cm), f"{owner}_window_prior_std_cm": sel[..., 3]}
    if owner == "enkf":
        out["enkf_window_innovation_cm"] = sel[..., 1] - sel[..., 2]
    if ranks.rank != 0:
        return out, None
    first = table[0, slots, :, 0] == 1.0                   # the record is the same for every point
    line = f"{int(first.sum())} lagged observations over {int(first.any(axis=-1).sum())} rows"
    if owner == "enkf":
        return out, f" [{label}] EnKF window: {line} (offsets {list(window)})"
    return out, f" [{label}] filter window: {line}"


def _enkf_method_arrays(enkf, scheme):
    """``enkf_method`` (0 = stochastic, 1 = sqrt) and ``enkf_relaxation``, when the block names either."""
    import numpy as np
    if not enkf[0] or scheme is None:
        return {}
    return {"enkf_method": np.array(ENKF_METHOD_NAMES.index(scheme[0]), dtype=np.int8),
            "enkf_relaxation": np.array(scheme[1], dtype=np.float64)}


SM_KEYS = ("Filename", "Depths_cm", "Sigma")
SM_MAX_DEPTHS = 8


def soil_moisture_settings(ens, n_gpus=1, owner="EnKF"):
    """Ensemble.EnKF.Soil_Moisture (``owner`` = "Filter": Ensemble.Filter.Soil_Moisture, the same block) -> (filename,
    depths_cm tuple, sigma tuple per depth), or None when absent.  Pure, like :func:`enkf_settings` / :func:`filter_settings`
    (the owner's, which it runs first: its refusals -- "Filter" with "EnKF", one point on several GPUs -- hold): a bad value
    is a ValueError (message + exit status 1).  Needs the owner active.  The filter's record is refused together with
    ``"Sharded": true`` on a single-point run.  The depths are checked against the column and the file is read later
    (:func:`soil_moisture_record_of`)."""
    import math
    from numbers import Real
    if "Soil_Moisture" in ens:
        raise ValueError(" Ensemble: Soil_Moisture belongs inside the \"EnKF\" block (or the \"Filter\" block).")
    settings = enkf_settings if owner == "EnKF" else filter_settings
    block = ens.get(owner)
    if not isinstance(block, dict) or block.get("Soil_Moisture") is None:
        settings(ens, n_gpus)
        return None
    stride = settings(ens, n_gpus)[0]
    sm = block["Soil_Moisture"]
    if not stride:
        what = "EnKF" if owner == "EnKF" else "filter"
        raise ValueError(f" Ensemble: {owner}.Soil_Moisture needs an active {what} ({owner}.Stride > 0).")
    if owner == "Filter" and not ens.get("Points") and block.get("Sharded", False):
        raise ValueError(" Ensemble: Filter.Soil_Moisture is not available with \"Sharded\": true: the sharded filter "
                         "gathers the members' water-table indices only, and the sensors' weights need every member's "
                         "state on one GPU (a sweep's points are dealt whole and take the record).")
    if not isinstance(sm, dict):
        raise ValueError(f" Ensemble: {owner}.Soil_Moisture = {sm!r} must be an object such as "
                         f"{{\"Filename\": \"sm.csv\", \"Depths_cm\": [30, 60], \"Sigma\": 0.02}}.")
    unknown = sorted(set(sm) - set(SM_KEYS))
    if unknown:
        raise ValueError(f" Ensemble: {owner}.Soil_Moisture has unknown keys {unknown} (known: {list(SM_KEYS)}).")
    name = sm.get("Filename")
    if not isinstance(name, str) or not name:
        raise ValueError(f" Ensemble: {owner}.Soil_Moisture.Filename = {name!r} must name the sensor CSV.")

    def number(x):
        return not isinstance(x, bool) and isinstance(x, Real) and math.isfinite(x)

    depths = sm.get("Depths_cm")
    if not isinstance(depths, (list, tuple)) or not depths or not all(number(d) for d in depths):
        raise ValueError(f" Ensemble: {owner}.Soil_Moisture.Depths_cm = {depths!r} must be a non-empty list of finite "
                         f"depths (cm).")
    if len(depths) > SM_MAX_DEPTHS:
        raise ValueError(f" Ensemble: {owner}.Soil_Moisture.Depths_cm has {len(depths)} depths, at most {SM_MAX_DEPTHS}.")
    if "Sigma" not in sm:
        raise ValueError(f" Ensemble: {owner}.Soil_Moisture.Sigma (the sensors' error, m^3/m^3) is required.")
    sigma = sm["Sigma"]
    sig = list(sigma) if isinstance(sigma, (list, tuple)) else [sigma] * len(depths)
    if len(sig) != len(depths) or not all(number(x) and x > 0 for x in sig):
        raise ValueError(f" Ensemble: {owner}.Soil_Moisture.Sigma = {sigma!r} must be a finite number > 0 or one per depth "
                         f"({len(depths)}).")
    return name, tuple(float(d) for d in depths), tuple(float(x) for x in sig)


def read_soil_moisture_csv(path, datenum, n_depths):
    """The header-less sensor CSV ``ID, Datenum, VWC_1, ..., VWC_m`` -> values [T][m] (NaN = none).  It must have one row
    per forcing row with the forcing's ``Datenum`` (within 1e-6 day) and m value columns in [0, 1] (or empty / NaN)."""
    import numpy as np
    datenum = np.asarray(datenum, dtype=np.float64)
    rows = []
    with open(path, "r") as fh:
        for k, line in enumerate(fh):
            if not line.strip():
                continue
            fields = [f.strip() for f in line.rstrip("\r\n").split(",")]
            if len(fields) != 2 + n_depths:
                raise ValueError(f" Soil moisture: {path} row {k + 1} has {len(fields)} fields, expected "
                                 f"{2 + n_depths} (ID, Datenum and {n_depths} values).")
            try:
                rows.append([float(f) if f else float("nan") for f in fields[1:]])
            except ValueError:
                raise ValueError(f" Soil moisture: {path} row {k + 1} holds a field that is not a number.") from None
    table = np.array(rows, dtype=np.float64).reshape(-1, 1 + n_depths)
    if table.shape[0] != datenum.size:
        raise ValueError(f" Soil moisture: {path} has {table.shape[0]} rows, the forcing {datenum.size}.")
    bad = np.flatnonzero(~(np.abs(table[:, 0] - datenum) <= 1e-6))
    if bad.size:
        raise ValueError(f" Soil moisture: {path} row {int(bad[0]) + 1} has Datenum {float(table[bad[0], 0])!r}, the forcing "
                         f"{float(datenum[bad[0]])!r}.")
    values = table[:, 1:]
    out = ~np.isnan(values) & ~((values >= 0.0) & (values <= 1.0))
    if out.any():
        r, c = np.argwhere(out)[0]
        raise ValueError(f" Soil moisture: {path} row {int(r) + 1} value {int(c) + 1} = {float(values[r, c])!r} lies outside [0, 1].")
    return values


def soil_moisture_record_of(sm, cols, water_data, owner="EnKF"):
    """The sensor record (stepper.soil_moisture_record) of the ``owner`` block's settings ``sm`` on the column ``cols``: the
    depths mapped to nodes (refused outside the column) and the CSV read against the forcing's Datenum.  None without
    sensors."""
    from .stepper import sensor_nodes, soil_moisture_record
    if sm is None:
        return None
    name, depths, sigma = sm
    try:
        sensor_nodes(cols.z, depths)
    except ValueError as bad:
        raise ValueError(f" Ensemble: {owner}.Soil_Moisture.Depths_cm: {bad}.") from None
    if not Path(name).exists():
        raise ValueError(f" Soil moisture: the sensor file {name} does not exist.")
    values = read_soil_moisture_csv(name, water_data["Datenum"].to_numpy(), len(depths))
    return soil_moisture_record(cols.z, depths, values, sigma)


SM_DATASETS = ("observed", "obs", "prior_mean", "prior_std", "post_mean", "post_std")


def _reduce_sm(ranks, sim, ids, P, T, D, stride, record, slots, label, keep_points, owner="enkf"):
    """The sensors' datasets (``owner``: "enkf" or "filter", the prefix of the datasets and of the handle's table) from
    this rank's handle over the owner's assimilated ``slots`` (its ``enkf_rows`` / ``filter_rows``), the [P] table placed
    and summed over the ranks like the owner's, and the closing line (rank 0)."""
    import numpy as np
    from .stepper import enkf_sm_summary
    if not stride or record is None:
        return {}, None
    table = _placed_table(ranks, sim, ids, P, T, D, stride, owner + "_sm", int(np.asarray(record["nodes"]).size))
    sel = table[:, slots] if keep_points else table[0, slots]
    out = {f"{owner}_sm_depths_cm": np.asarray(record["depths_cm"], dtype=np.float64),
           f"{owner}_sm_nodes": np.asarray(record["nodes"], dtype=np.int32),
           f"{owner}_sm_sigma": np.asarray(record["sigma"], dtype=np.float64)}
    for j, k in enumerate(SM_DATASETS):
        v = sel[..., j]
        out[f"{owner}_sm_{k}"] = (v == 1.0).astype(np.int8) if k == "observed" else v
    summary = enkf_sm_summary(table if keep_points else table[0], stride, record["sigma"])
    if ranks.rank != 0:
        return out, None
    rows = int(summary["rows"].size)
    if keep_points:
        r = np.asarray(summary["rmse_all"], dtype=np.float64)
        best = int(np.nanargmin(r)) if np.isfinite(r).any() else 0
        line = f" [{label}] soil-moisture forecast RMSE: best point {best} = {r[best]:.5f} over {rows} rows"
    else:
        line = f" [{label}] soil-moisture forecast RMSE = {float(summary['rmse_all']):.5f} over {rows} rows"
    return out, line


def _reduce_enkf(ranks, table, enkf, label, keep_points, z0_cm):
    """The EnKF's datasets from its placed [P] ``table`` (:func:`_placed_table`) and the closing line (rank 0).  The
    means are given at the well's depths (``z0_cm`` = z[0] + the table's depths from the top node)."""
    import numpy as np
    from .stepper import enkf_summary
    stride, sigma, loc, _ = enkf
    summary = enkf_summary(table if keep_points else table[0], stride, sigma, float(z0_cm))
    out = {f"enkf_{k}": summary[k] for k in ("rows", "count", "prior_mean_cm", "prior_std_cm", "innovation_cm",
                                             "post_mean_cm", "post_std_cm", "loglik_rows", "rejected")}
    out.update(enkf_loglik=np.asarray(summary["loglik"], dtype=np.float64), enkf_sigma_cm=np.array(sigma, dtype=np.float64),
               enkf_localisation_cm=np.array(loc, dtype=np.float64))
    n = int(summary["rows"].size)
    if ranks.rank != 0:
        return out, None
    if keep_points:
        ll = np.asarray(summary["loglik"], dtype=np.float64)
        best = int(np.nanargmax(ll)) if np.isfinite(ll).any() else 0
        line = f" [{label}] EnKF log-likelihood: best point {best} = {ll[best]:.3f} over {n} rows"
    else:
        line = f" [{label}] EnKF log-likelihood = {float(summary['loglik']):.3f} over {n} rows"
    return out, line


def _reduce_filter(ranks, sim, ids, P, T, D, table, a, label, keep_points):
    """The filter's datasets from its placed [P] ``table`` (:func:`_placed_table`) and the closing line (rank 0).
    ``a.ess_floor`` (Filter.ESS_floor): the tempering's table placed likewise, its datasets and a second closing line;
    ``a.rejuvenation`` (Filter.Rejuvenation): the rejuvenation's, and a line of its own."""
    import numpy as np
    from .stepper import filter_summary, rejuvenation_shrinkage
    (stride, sigma, _), ess_floor, rejuvenation = a.filt, a.ess_floor, a.rejuvenation
    ttable = rtable = None
    if ess_floor is not None:
        ttable = _placed_table(ranks, sim, ids, P, T, D, stride, "filter_temper")
        ttable = ttable if keep_points else ttable[0]
    if rejuvenation is not None:
        rtable = _placed_table(ranks, sim, ids, P, T, D, stride, "filter_rejuvenation")
        rtable = rtable if keep_points else rtable[0]
    summary = filter_summary(table if keep_points else table[0], stride, sigma, temper_table=ttable,
                             rejuvenation_table=rtable)
    out = {"filter_rows": summary["rows"], "filter_count": summary["count"], "filter_ess": summary["ess"],
           "filter_loglik_rows": summary["loglik_rows"], "filter_survivors": summary["survivors"],
           "filter_loglik": np.asarray(summary["loglik"], dtype=np.float64),
           "filter_sigma_cm": np.array(sigma, dtype=np.float64)}
    if ess_floor is not None:
        out.update(filter_ess_floor=np.array(ess_floor, dtype=np.float64), filter_beta=summary["beta"],
                   filter_ess_tempered=summary["ess_tempered"], filter_ess_target=summary["ess_target"])
    if rejuvenation is not None:
        out.update(filter_rejuvenation_discount=np.array(rejuvenation, dtype=np.float64),
                   filter_rejuvenation_shrinkage=np.array(rejuvenation_shrinkage(rejuvenation)[0], dtype=np.float64),
                   filter_rejuvenated=summary["rejuvenated"].astype(np.int8),
                   filter_rejuvenation_refused=summary["rejuvenation_refused"],
                   filter_noise_std_resampled=summary["noise_std_resampled"],
                   filter_noise_std_rejuvenated=summary["noise_std_rejuvenated"])
    n = int(summary["rows"].size)
    if ranks.rank != 0:
        return out, None
    if keep_points:
        ll = np.asarray(summary["loglik"], dtype=np.float64)
        best = int(np.nanargmax(ll)) if np.isfinite(ll).any() else 0
        line = f" [{label}] filter log-likelihood: best point {best} = {ll[best]:.3f} over {n} rows"
    else:
        line = f" [{label}] filter log-likelihood = {float(summary['loglik']):.3f} over {n} rows"
    if ess_floor is not None:
        # (a sweep: the rows on which any point was tempered, the smallest beta of any point)
        beta = np.asarray(summary["beta"], dtype=np.float64).reshape(-1, n)
        k = int((beta < 1.0).any(axis=0).sum())
        least = float(np.nanmin(beta)) if np.isfinite(beta).any() else float("nan")
        line += f"\n [{label}] filter tempering: {k} of {n} rows tempered, smallest beta = {least:.6g}"
    if rejuvenation is not None:
        # (a sweep: the rows on which any point was rejuvenated; the ratio's mean over every point and row that was)
        moved = np.asarray(summary["rejuvenated"]).reshape(-1, n) > 0
        before = np.asarray(summary["noise_std_resampled"], dtype=np.float64).reshape(-1, n)[moved]
        after = np.asarray(summary["noise_std_rejuvenated"], dtype=np.float64).reshape(-1, n)[moved]
        ok = before > 0
        kept = float((after[ok] / before[ok]).mean()) if ok.any() else float("nan")
        line += (f"\n [{label}] filter rejuvenation: {int(moved.any(axis=0).sum())} of {n} rows, noise-field spread kept "
                 f"{kept:.4f} of resampled")
    return out, line


def _distribution_datasets(hist, dist):
    """The datasets of the water-table distribution (hist: the int64 sum over the ranks, stored as int32)."""
    import numpy as np
    return {"wtd_hist": np.asarray(hist, dtype=np.int32), "wtd_hist_rows": np.asarray(dist["rows"], dtype=np.int64),
            "wtd_hist_count": np.asarray(dist["count"], dtype=np.int64),
            "wtd_quantile_levels": np.asarray(dist["levels"], dtype=np.float64),
            "wtd_quantile_cm": np.asarray(dist["quantile_cm"]), "wtd_crps_cm": np.asarray(dist["crps_cm"]),
            "wtd_crps_mean_cm": np.asarray(dist["crps_mean_cm"], dtype=np.float64)}


def _crps_line(what, dist):
    """The closing line, after the reference's running MAE (simulation.py:633-649): the mean CRPS over the histogram rows
    that counted members (all points of a sweep together)."""
    import numpy as np
    solved = np.asarray(dist["count"]) > 0
    n = int(solved.sum())
    mean = float(np.asarray(dist["crps_cm"])[solved].mean()) if n else float("nan")
    return f" [{what}] CRPS = {mean:.3f} cm over {n} rows"


def _profile_stride(ens):
    """Ensemble.Profiles: stride of the profile rows (absent / 0: no profile statistics)."""
    stride = int(ens.get("Profiles", 0) or 0)
    if stride < 0:
        raise ValueError(f" Ensemble: Profiles = {stride} must be a positive row stride.")
    return stride


def _profile_datasets(stats):
    """The datasets of the profile statistics: the reference's output keys with _mean / _std (simulation.py:658-671)."""
    import numpy as np
    keys = ("theta_vol_mean", "theta_vol_std", "psi_press_mean", "psi_press_std", "S_eff_mean", "S_eff_std",
            "transpiration_mean", "transpiration_std", "lateral_flow_mean", "lateral_flow_std", "abs_error_mean")
    out = {k: np.asarray(stats[k]) for k in keys}
    out["profile_rows"] = np.asarray(stats["rows"])
    out["profile_count"] = np.asarray(stats["count"])
    out["profile_overflow"] = np.array(stats["overflow"], dtype=np.int64)
    return out


def _step_all(sim, rows, label, ranks):
    """Advance `sim` over its first `rows` forcing rows, 30 days per call, each call followed by the progress line."""
    where = "" if ranks.world == 1 else f" on {ranks.world} GPUs"
    done = 0
    while done < rows:
        n = min(48 * 30, rows - done)
        sim.advance(n)
        done += n
        if ranks.rank == 0:
            print(f" [{label}{where}] {done} rows done")


def _reduce_optional(ranks, sim, ids, cols_all, forcing, stride, dist_stride, dist_levels, device, label, keep_points):
    """The run's optional tables -- profile statistics (``stride``), water-table histograms (``dist_stride``) -- from this
    rank's handle ``sim`` (None: the rank holds no points), whose points are ``ids`` of the run's ``cols_all`` (an ensemble:
    point 0 of 1), placed in the whole run's tables and summed over the ranks (``multigpu.place_points``).  Returns their
    datasets (a sweep, ``keep_points``: with the leading [P] axis, at P = 1 too) and the closing CRPS line (rank 0, and
    only with histograms; None otherwise)."""
    import numpy as np
    from .stepper import diag_counts, join_diag, profile_tables_to_stats, wtd_distribution
    P, T, D, ref = len(cols_all), forcing.dim_t, cols_all[0].dim_d, cols_all[0]
    counts = diag_counts(P, T, D, profile_stride=stride, wtd_hist_stride=dist_stride)
    out, crps_line = {}, None
    if stride:
        table = join_diag("profile", _placed_diag(ranks, sim, ids, P, "profile", counts))
        stats = profile_tables_to_stats(table, P, T, D, stride, np.stack([c.por_node for c in cols_all]), ref.dz)
        if keep_points and P == 1:
            stats = {k: (v[None] if isinstance(v, np.ndarray) and k != "rows" else v) for k, v in stats.items()}
        out.update(_profile_datasets(stats))
    if dist_stride:
        # int32 counts, summed as int64 like the moments; rank 0 forms the summary
        hist = _placed_diag(ranks, sim, ids, P, "wtd_hist", counts)["hist"]
        hist = hist if keep_points else hist[0]
        if ranks.rank == 0:
            dist = wtd_distribution(hist, forcing.wtd_obs, dist_levels, ref.dz, ref.z, device, dist_stride)
            out.update(_distribution_datasets(hist, dist))
            crps_line = _crps_line(label, dist)
    return out, crps_line


def _reduce_theta(ranks, sim, ids, P, T, D, stride, theta, label, keep_points):
    """The soil-moisture histograms (``theta``: bins, levels) from this rank's handle ``sim`` (None: no points), its points
    ``ids`` placed in the run's [P] table and summed over the ranks like the water-table histograms -- int32 counts as
    int64, the outside count with them -- then the quantile bands and the closing line (rank 0)."""
    import numpy as np
    from .stepper import diag_counts, theta_distribution
    bins, levels = theta
    if not bins:
        return {}, None
    parts = _placed_diag(ranks, sim, ids, P, "theta_hist", diag_counts(P, T, D, profile_stride=stride, theta_bins=bins))
    hist, outside = parts["hist"] if keep_points else parts["hist"][0], parts["outside"]
    if ranks.rank != 0:
        return {}, None
    dist = theta_distribution(hist, levels, bins, stride)
    out = {"theta_hist": np.asarray(hist, dtype=np.int32), "theta_hist_rows": np.asarray(dist["rows"], dtype=np.int64),
           "theta_hist_count": np.asarray(dist["count"], dtype=np.int64), "theta_hist_bins": np.array(bins, dtype=np.int64),
           "theta_hist_outside": np.array(outside, dtype=np.int64),
           "theta_quantile_levels": np.asarray(dist["levels"], dtype=np.float64),
           "theta_quantile": np.asarray(dist["quantiles"], dtype=np.float64)}
    n = int((np.asarray(dist["count"]).reshape(-1, dist["rows"].size) > 0).any(axis=0).sum())
    line = f" [{label}] theta bands: {len(levels)} levels on {n} rows, {bins} bins"
    if outside:
        line += f" ({outside} values outside [0, 1])"
    return out, line


def _reduce_storage(ranks, sim, ids, P, T, cols, stride, storage, label, keep_points):
    """The layer-storage tables (``storage``: layers, bins, levels) from this rank's handle ``sim`` (None: no points), its
    points ``ids`` placed in the run's [P] tables and summed over the ranks like the profile table and the soil-moisture
    histograms -- the overflow and outside counts with them -- then mean, sigma, the quantile bands and the closing line
    (rank 0)."""
    import numpy as np
    from .stepper import diag_counts, join_diag, layer_storage_distribution, layer_storage_stats
    if storage is None:
        return {}, None
    layers, bins, levels = storage
    ranges = storage_ranges(storage, cols)
    L = len(ranges)
    counts = diag_counts(P, T, cols.dim_d, profile_stride=stride, storage_layers=L, storage_bins=bins)
    table = join_diag("storage", _placed_diag(ranks, sim, ids, P, "storage", counts))
    if bins:
        parts = _placed_diag(ranks, sim, ids, P, "storage_hist", counts)
        hist, outside = parts["hist"], parts["outside"]
    if ranks.rank != 0:
        return {}, None
    stats = layer_storage_stats(table, P, T, L, stride)
    lead = (lambda v: v[None]) if keep_points and P == 1 else (lambda v: v)
    out = {"storage_layers_cm": np.asarray(layers, dtype=np.float64), "storage_nodes": np.asarray(ranges, dtype=np.int64),
           "storage_rows": np.asarray(stats["rows"], dtype=np.int64),
           "storage_count": np.asarray(lead(stats["count"]), dtype=np.int64),
           "storage_mean_cm": np.asarray(lead(stats["mean_cm"]), dtype=np.float64),
           "storage_std_cm": np.asarray(lead(stats["std_cm"]), dtype=np.float64),
           "storage_overflow": np.array(stats["overflow"], dtype=np.int64)}
    if bins:
        hist = hist if keep_points else hist[0]
        dist = layer_storage_distribution(hist, ranges, cols.dz, levels, stride)
        out.update({"storage_hist": np.asarray(hist, dtype=np.int32), "storage_hist_bins": np.array(bins, dtype=np.int64),
                    "storage_hist_outside": np.array(outside, dtype=np.int64),
                    "storage_quantile_levels": np.asarray(dist["levels"], dtype=np.float64),
                    "storage_quantile_cm": np.asarray(dist["quantiles_cm"], dtype=np.float64)})
    n = int((np.asarray(stats["count"]).reshape(-1, stats["rows"].size) > 0).any(axis=0).sum())
    line = f" [{label}] storage: {L} layers on {n} rows"
    if stats["overflow"] or (bins and outside):
        line += f" ({stats['overflow']} values clamped, {outside if bins else 0} layer means outside [0, 1])"
    return out, line


def _reduce_conductivity(ranks, sim, ids, P, T, cols, stride, cond, label, keep_points):
    """The conductivity table (``cond``: the layers) from this rank's handle ``sim`` (None: no points), its points ``ids``
    placed in the run's [P] table and summed over the ranks like the profile table -- the overflow count with it -- then
    mean and sigma of ln K, the geometric means and the closing line (rank 0)."""
    import numpy as np
    from .stepper import conductivity_stats, diag_counts, join_diag
    if cond is None:
        return {}, None
    ranges = conductivity_layer_ranges(cond, cols)
    L, D = len(ranges), cols.dim_d
    counts = diag_counts(P, T, D, profile_stride=stride, conductivity_layers=L)
    table = join_diag("conductivity", _placed_diag(ranks, sim, ids, P, "conductivity", counts))
    if ranks.rank != 0:
        return {}, None
    stats = conductivity_stats(table, P, T, D, L, stride)
    lead = (lambda v: v[None]) if keep_points and P == 1 else (lambda v: v)
    out = {"conductivity_rows": np.asarray(stats["rows"], dtype=np.int64),
           "conductivity_count": np.asarray(lead(stats["count"]), dtype=np.int64),
           "conductivity_overflow": np.array(stats["overflow"], dtype=np.int64)}
    names = ["lnK_hrc_mean", "lnK_hrc_std", "K_hrc_geomean", "lnK_bkg_mean", "lnK_bkg_std", "K_bkg_geomean"]
    if L:
        out.update(K_eff_layers_cm=np.asarray(cond, dtype=np.float64), K_eff_nodes=np.asarray(ranges, dtype=np.int64),
                   K_eff_count=np.asarray(lead(stats["K_eff_count"]), dtype=np.int64))
        names += ["lnK_eff_mean", "lnK_eff_std", "K_eff_geomean"]
    out.update((name, np.asarray(lead(stats[name]), dtype=np.float64)) for name in names)
    n = int((np.asarray(stats["count"]).reshape(-1, stats["rows"].size, D * 2) > 0).any(axis=(0, 2)).sum())
    line = f" [{label}] conductivity: {D} nodes and {L} layers on {n} rows"
    if stats["overflow"]:
        line += f" ({stats['overflow']} values clamped)"
    return out, line


def _reduce_covariance(ranks, sim, ids, P, T, cols, stride, cov, label, keep_points):
    """The theta covariance table (``cov``: node stride, sensor sigma) from this rank's handle ``sim`` (None: no points), its
    points ``ids`` placed in the run's [P] table and summed over the ranks like the profile table -- the outside count with
    it -- then the covariances, the correlations with the water table, the sensor gain and the closing line (rank 0)."""
    import numpy as np
    from .stepper import diag_counts, theta_cov_finish, theta_cov_shape, theta_sensor_gain
    if cov is None:
        return {}, None
    s, sigma = cov
    n = theta_cov_shape(cols.dim_d, s)[0]
    parts = _placed_diag(ranks, sim, ids, P, "theta_cov", diag_counts(P, T, cols.dim_d, profile_stride=stride, cov_stride=s))
    table, outside = parts["cov"], parts["outside"]
    if ranks.rank != 0:
        return {}, None
    table = table if keep_points else table[0]
    fin = theta_cov_finish(table, cols.dz, s, cols.dim_d)
    nodes = np.arange(0, cols.dim_d, s, dtype=np.int64)
    out = {"theta_cov_node_stride": np.array(s, dtype=np.int64), "theta_cov_nodes": nodes,
           "theta_cov_depth_cm": np.asarray(cols.z, dtype=np.float64)[nodes],
           "theta_cov_rows": np.arange(table.shape[-2], dtype=np.int64) * int(stride),
           "theta_cov_count": np.asarray(fin["count"], dtype=np.int64),
           "theta_cov_outside": np.array(outside, dtype=np.int64),
           "theta_cov": np.asarray(fin["theta_cov"], dtype=np.float64),
           "wtd_theta_cov_cm": np.asarray(fin["wtd_theta_cov_cm"], dtype=np.float64),
           "wtd_var_cm2": np.asarray(fin["wtd_var_cm2"], dtype=np.float64),
           "theta_wtd_corr": np.asarray(fin["theta_wtd_corr"], dtype=np.float64)}
    if sigma is not None:
        out["theta_sensor_sigma"] = np.array(sigma, dtype=np.float64)
        out["theta_sensor_gain"] = np.asarray(theta_sensor_gain(fin, sigma), dtype=np.float64)
    rows = int((np.asarray(fin["count"]).reshape(-1, table.shape[-2]) > 0).any(axis=0).sum())
    line = f" [{label}] covariance: {n} nodes on {rows} rows"
    if outside:
        line += f" ({outside} members outside [0, 1])"
    return out, line


def _reduce_periods(ranks, sim, ids, P, cols, forcing, periods, plan, label, keep_points):
    """The period-totals tables (``periods``: the block's settings, ``plan``: end rows and threshold nodes) from this rank's
    handle ``sim`` (None: no points), its points ``ids`` placed in the run's [P] tables and summed over the ranks like the
    storage tables -- the overflow and outside counts with them -- then the statistics, the quantiles and the closing line
    (rank 0)."""
    import numpy as np
    from .stepper import diag_counts, flux_max_log2_of, join_diag, period_totals_distribution, period_totals_stats
    if periods is None:
        return {}, None
    ends, nodes = plan
    n_period, K, bins = len(ends), 4 + len(nodes), periods["bins"]
    counts = diag_counts(P, D=cols.dim_d, periods=n_period, thresholds=len(nodes), period_bins=bins)
    table = join_diag("period", _placed_diag(ranks, sim, ids, P, "period", counts))
    if bins:
        parts = _placed_diag(ranks, sim, ids, P, "period_hist", counts)
        hist_flux, hist_wtd, outside = parts["flux"], parts["wtd"], parts["outside"]
    if ranks.rank != 0:
        return {}, None
    stats = period_totals_stats(table, P, ends, len(nodes), float(cols.z[0]), cols.dz, forcing.wtd_obs)
    lead = (lambda v: v[None]) if keep_points and P == 1 else (lambda v: v)
    out = {"period_end_rows": np.asarray(ends, dtype=np.int64),
           "period_solved_rows": np.asarray(stats["solved_rows"], dtype=np.int64),
           "period_count": np.asarray(lead(stats["count"]), dtype=np.int64),
           "period_thresholds_cm": np.asarray(periods["thresholds_cm"], dtype=np.float64),
           "period_threshold_nodes": np.asarray(nodes, dtype=np.int64),
           "period_overflow": np.array(stats["overflow"], dtype=np.int64)}
    for name in ("transpiration", "lateral_flow", "wtd_shallowest", "wtd_deepest"):
        for what in ("mean_cm", "std_cm"):
            out[f"period_{name}_{what}"] = np.asarray(lead(stats[f"{name}_{what}"]), dtype=np.float64)
    for what in ("below_rows_mean", "below_rows_std", "below_fraction_mean"):
        out["period_" + what] = np.asarray(lead(stats[what]), dtype=np.float64)
    if bins:
        if not keep_points:
            hist_flux, hist_wtd = hist_flux[0], hist_wtd[0]
        dist = period_totals_distribution(hist_flux, hist_wtd, periods["levels"],
                                          [flux_max_log2_of(v) for v in periods["flux_max_cm"]], float(cols.z[0]), cols.dz)
        out.update({"period_hist_flux": np.asarray(hist_flux, dtype=np.int32),
                    "period_hist_wtd": np.asarray(hist_wtd, dtype=np.int32),
                    "period_hist_bins": np.array(bins, dtype=np.int64),
                    "period_hist_flux_max_cm": np.asarray(periods["flux_max_cm"], dtype=np.float64),
                    "period_hist_outside": np.array(outside, dtype=np.int64),
                    "period_quantile_levels": np.asarray(dist["levels"], dtype=np.float64)})
        for name in ("transpiration", "lateral_flow", "wtd_shallowest", "wtd_deepest"):
            out[f"period_{name}_quantile_cm"] = np.asarray(dist[f"{name}_quantile_cm"], dtype=np.float64)
    n = int((np.asarray(stats["count"]).reshape(-1, n_period) > 0).any(axis=0).sum())
    line = f" [{label}] periods: {n} periods, {K} quantities"
    if stats["overflow"] or (bins and outside):
        line += f" ({stats['overflow']} values clamped, {outside if bins else 0} totals outside their histogram)"
    return out, line


def _reduce_uptake(ranks, sim, ids, P, cols, uptake, cells, plan, label, keep_points):
    """The root-uptake tables (``uptake``: the block's settings, ``cells``: the layers' cell ranges, ``plan``: the periods')
    from this rank's handle ``sim`` (None: no points), its points ``ids`` placed in the run's [P] tables and summed over
    the ranks like the period totals' -- the overflow and outside counts with them -- then the statistics, the profile,
    the quantiles and the closing line (rank 0)."""
    import numpy as np
    from .stepper import diag_counts, join_diag, root_uptake_distribution, root_uptake_profile, root_uptake_stats
    if uptake is None:
        return {}, None
    ends = plan[0]
    n_period, L, bins, D = len(ends), len(cells), uptake["bins"], cols.dim_d
    counts = diag_counts(P, D=D, periods=n_period, uptake_layers=L, uptake_bins=bins)
    whole = _placed_diag(ranks, sim, ids, P, "uptake", counts)
    table = join_diag("uptake", whole)
    if bins:
        parts = _placed_diag(ranks, sim, ids, P, "uptake_hist", counts)
        hist, outside = parts["hist"], parts["outside"]
    if ranks.rank != 0:
        return {}, None
    stats = root_uptake_stats(table, P, ends, L, D)
    prof = root_uptake_profile(table, P, ends, L, D, cols.z)
    lead = (lambda v: v[None]) if keep_points and P == 1 else (lambda v: v)
    out = {"uptake_layers_cm": np.asarray(uptake["layers_cm"], dtype=np.float64),
           "uptake_cells": np.asarray(cells, dtype=np.int64),
           "uptake_depth_cm": np.asarray(prof["depth_cm"], dtype=np.float64),
           "uptake_count": np.asarray(lead(stats["count"]), dtype=np.int64),
           "uptake_overflow": np.array(stats["overflow"], dtype=np.int64),
           "uptake_profile": np.asarray(lead(prof["profile"]), dtype=np.float64),
           "uptake_depth_quantile_cm": np.asarray(lead(prof["depth_quantile_cm"]), dtype=np.float64)}
    for name in ("total_mean_cm", "total_std_cm", "layer_mean_cm", "layer_std_cm", "share_of_mean"):
        out["uptake_" + name] = np.asarray(lead(stats[name]), dtype=np.float64)
    if bins:
        if not keep_points:
            hist = hist[0]
        dist = root_uptake_distribution(hist, uptake["levels"])
        out.update({"uptake_share_hist": np.asarray(hist, dtype=np.int32),
                    "uptake_hist_outside": np.array(outside, dtype=np.int64),
                    "uptake_quantile_levels": np.asarray(dist["levels"], dtype=np.float64),
                    "uptake_share_quantile": np.asarray(dist["share_quantile"], dtype=np.float64)})
    n = int((np.asarray(stats["count"]).reshape(-1, n_period) > 0).any(axis=0).sum())
    # the depth above which half of the run's uptake lies: the periods' (and points') limbs summed, then the quantile
    limbs = whole["uprof"].astype(object).sum(axis=(0, 1))
    cum = np.cumsum(limbs[:, 0] + limbs[:, 1] * (1 << 20))
    median = float(cols.z[int(np.argmax(2 * cum >= cum[-1]))] + cols.dz) if int(cum[-1]) > 0 else float("nan")
    line = f" [{label}] uptake: {L} layers over {n} periods, median depth {median:g} cm"
    if stats["overflow"]:
        line += f" ({stats['overflow']} values clamped)"
    return out, line


def _reduce_diagnostics(ranks, sim, ids, cols_all, forcing, run, device, label, keep_points):
    """Every diagnostic block of the run (``run``: its :class:`RunSettings`), reduced over the ranks in the one order both
    an ensemble and a sweep write their datasets in (a later block's dataset replaces an earlier one of the same name).
    Returns the datasets and {block: closing line or None}, ``crps`` first, the others in the order their lines are printed."""
    P, T, ref, stride = len(cols_all), forcing.dim_t, cols_all[0], run.stride
    reducers = (
        ("crps", lambda: _reduce_optional(ranks, sim, ids, cols_all, forcing, stride, run.dist[0], run.dist[1], device, label,
                                          keep_points)),
        ("theta", lambda: _reduce_theta(ranks, sim, ids, P, T, ref.dim_d, stride, run.theta, label, keep_points)),
        ("storage", lambda: _reduce_storage(ranks, sim, ids, P, T, ref, stride, run.storage, label, keep_points)),
        ("covariance", lambda: _reduce_covariance(ranks, sim, ids, P, T, ref, stride, run.cov, label, keep_points)),
        ("conductivity", lambda: _reduce_conductivity(ranks, sim, ids, P, T, ref, stride, run.conductivity, label,
                                                      keep_points)),
        ("periods", lambda: _reduce_periods(ranks, sim, ids, P, ref, forcing, run.periods, run.plan, label, keep_points)),
        ("uptake", lambda: _reduce_uptake(ranks, sim, ids, P, ref, run.uptake, run.ucells, run.plan, label, keep_points)))
    out, lines = {}, {}
    for block, reduce in reducers:
        tables, lines[block] = reduce()
        out.update(tables)
    return out, lines


def _run_sweep(params, forcing, output_name, ens, n_members, rows, device, ranks, run=RunSettings()):
    """Parameter points x members (``run``: the :class:`RunSettings`): this rank's points in one handle
    (ensemble.SweepSimulation), the whole table assembled over the ranks (multigpu.assemble_points)."""
    import numpy as np
    from . import multigpu
    from .digest import ColumnTables, load_site_well
    from .ensemble import SweepSimulation, check_sweep_points, deal_points
    from .stepper import moments_to_mean_std
    # a sweep runs in-kernel Philox noise from one spin-up per point; anything else is refused, not ignored
    if str(ens.get("Noise", "philox")).lower() != "philox":
        raise ValueError(f" Sweep: Ensemble.Noise = {ens.get('Noise')!r} is not supported with Points (philox only).")
    if str(ens.get("Spinup", "point")).lower() not in ("point", "shared"):
        raise ValueError(f" Sweep: Ensemble.Spinup = {ens.get('Spinup')!r} is not supported with Points "
                         f"(one spin-up per parameter point).")
    well = load_site_well(params)
    merged = check_sweep_points(params, ens["Points"])
    P = len(merged)
    mine = deal_points(P, ranks.rank, ranks.world)
    # every point's tables: a rank without points still joins the collectives (the grid is the well's, whoever owns it)
    cols_all = [ColumnTables(m, well) for m in merged]
    points, ref, T = [cols_all[k] for k in mine], cols_all[0], forcing.dim_t
    local, sim = {}, None
    label = f"Sweep {P} points x{n_members}"
    run = replace(run, stride=_profile_stride(ens), ucells=uptake_plan(run.uptake, cols_all))       # before any GPU call
    if mine:
        sim = SweepSimulation(points, forcing, n_members, seed=int(ens.get("Seed", 0)), device=device, point_ids=mine,
                              **run.kwargs())
        _step_all(sim, rows, label, ranks)
        table = sim.moments()
        for j, k in enumerate(mine):
            local[k] = {"moments": table[j], "psi0": sim.psi0[j],
                        "spinup_iterations": None if sim.spinup_iters is None else int(sim.spinup_iters[j])}
    moments, psi0, spin = multigpu.assemble_points(ranks, P, local, T, ref.dim_d)
    mean_cm, std_cm = moments_to_mean_std(moments, ref.dz, ref.z[0])
    arrays = dict(moments=moments, wtd_mean_cm=mean_cm, wtd_std_cm=std_cm, rows=np.array(rows),
                  members=np.array(n_members), points=np.array(P), gpus=np.array(ranks.world), initial_cond=psi0,
                  spinup_iterations=spin)
    tables, lines = _reduce_diagnostics(ranks, sim, mine, cols_all, forcing, run, device, label, keep_points=True)
    arrays.update(tables)
    atables, assim_lines = _reduce_assimilation(ranks, sim, mine, P, T, ref, run.assim, label, keep_points=True)
    arrays.update(atables)
    stables, smooth_line = _reduce_smoother(ranks, sim, mine, P, T, ref, forcing, run.assim, device, label, keep_points=True)
    arrays.update(stables)
    ctables, corr_line = _noise_correlation_arrays(run.corr, cols_all, label, keep_points=True)
    arrays.update(ctables)
    ptables, pert_line = _forcing_perturbation_arrays(run.pert, label)
    arrays.update(ptables)
    if sim is not None:
        sim.close()
    _save(output_name.strip().replace(" ", "_") + "_ensemble", arrays, "sweep's water-table statistics", ranks)
    _print_lines(lines.pop("crps"), *assim_lines, smooth_line, *lines.values(), corr_line if ranks.rank == 0 else None,
                 pert_line if ranks.rank == 0 else None)


def run_cli(argv=None):
    """berkeley_hydro_main.py:149-177, plus the self-launch of a multi-GPU run."""
    argv = sys.argv if argv is None else argv
    if len(argv) > 1:
        import argparse
        parser = argparse.ArgumentParser(description=" Berkeley Hydrological Simulation ")
        parser.add_argument("--params", help=" Input file (.json) with simulation parameters.")
        parser.add_argument("--data", help=" Input file (.csv) with simulation data (e.g.: precipitation, wtd).")
        parser.add_argument("--seed", type=int, default=None, help=" Seed of the noise stream (reproducible runs).")
        parser.add_argument("--device", type=int, default=0, help=" GPU ordinal.")
        parser.add_argument("--gpus", type=int, default=None,
                            help=" GPUs of this node to run an \"Ensemble\" block on (one process each; default: Ensemble.GPUs or 1).")
        args = parser.parse_args(argv[1:])
        from . import multigpu
        settings = _read_parameters(args.params)
        n_gpus = multigpu.requested_gpus(args.gpus, settings)
        if settings.get("Ensemble") and n_gpus > 1 and not multigpu.in_rank():
            try:                                    # a bad Filter or EnKF block ends the command before any rank starts
                filter_settings(settings["Ensemble"], n_gpus)
                enkf_settings(settings["Ensemble"], n_gpus)
                soil_moisture_settings(settings["Ensemble"], n_gpus)
                soil_moisture_settings(settings["Ensemble"], n_gpus, "Filter")
                enkf_method_settings(settings["Ensemble"])
                enkf_window_settings(settings["Ensemble"])
                enkf_noise_settings(settings["Ensemble"])
                filter_window_settings(settings["Ensemble"])
                filter_smoother_settings(settings["Ensemble"])
                noise_correlation_settings(settings["Ensemble"])
                forcing_perturbation_settings(settings["Ensemble"])
            except ValueError as bad:
                print(bad)
                sys.exit(1)
        if n_gpus > 1 and not multigpu.in_rank():
            # the parent only starts the ranks (nothing here has touched a GPU) and hands their exit status on
            script = Path(argv[0]).resolve()
            status = multigpu.launch_ranks(n_gpus, script, argv[1:])
            if status != 0:
                sys.exit(1)
            return                                  # (rank 0 has said " Simulation completed.")
        main(args.params, args.data, args.seed, args.device, args.gpus, _settings=settings)
        if _speaks():
            print(' Simulation completed.')
    else:
        sys.exit('Error: Not enough input parameters.')
