"""ctypes binding of libhydrocol.so (C-ABI declared in include/hydrocol.h).

There is no CPU path: if the shared library is missing, or no gfx950 device is visible,
the calls below raise.  Build with ``python -c "import __graft_entry__ as g; g.build()"``.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np

CSRC = Path(__file__).resolve().parent / "csrc"
LIB_PATH = CSRC / "libhydrocol.so"

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_bp = C.POINTER(C.c_uint8)
_lp = C.POINTER(C.c_int64)


class HcError(RuntimeError):
    """A libhydrocol call returned a negative status."""


class ColumnParams(C.Structure):
    """hc_column_params"""
    _fields_ = ([(k, C.c_int32) for k in ("dim_d", "model", "flag_et", "flag_lf", "flag_hlift",
                                          "n_root_first", "n_root_int", "n_groups")] +
                [(k, C.c_double) for k in ("theta_res", "alpha", "n", "m", "psi_sat", "epsilon",
                                           "lambda_exp", "sigma_noise", "sat_soil", "dz", "ipsi50", "lai",
                                           "surface_evap", "interception", "evap_delta_min")] +
                [("flag_predict", C.c_int32), ("sat_cells", C.c_int32)])


class StepArgs(C.Structure):
    """hc_step_args"""
    _fields_ = [("row_begin", C.c_int64), ("n_rows", C.c_int64), ("spinup", C.c_int32),
                ("accumulate_moments", C.c_int32), ("fresh_noise", _dp), ("wtd_out", _ip),
                ("stats_out", _ip), ("psi_rows_out", _dp), ("diag_out", _dp), ("kernel_ms", C.c_double),
                ("launches", C.c_int64)]


class SpinupArgs(C.Structure):
    """hc_spinup_args"""
    _fields_ = [("forcing_row", C.c_int64), ("max_iterations", C.c_int32), ("zwtd_cm", C.c_double),
                ("z0_cm", C.c_double), ("iterations_out", _ip), ("kernel_ms", C.c_double)]


# hc_enkf_exchange_fn: (ctx, device_buf, n_words, first_word, count_words) -> 0 = ok
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64)

# hc_filter_route_fn: (ctx, send, send_words[n_shards], recv, recv_words[n_shards]) -> 0 = ok
ROUTE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, _lp, C.c_void_p, _lp)

EXPORTS = {
    "hc_create": ([C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "hc_destroy": ([C.c_void_p], C.c_int),
    "hc_last_error": ([], C.c_char_p),
    "hc_version": ([], C.c_char_p),
    "hc_set_column": ([C.c_void_p, C.POINTER(ColumnParams), _dp, _dp, _ip], C.c_int),
    "hc_add_point": ([C.c_void_p, C.POINTER(ColumnParams), _dp, _dp], C.c_int),
    "hc_get_point_count": ([C.c_void_p], C.c_int),
    "hc_set_forcing": ([C.c_void_p, C.c_int64, _dp, _dp, _bp, _ip, _bp], C.c_int),
    "hc_set_forcing_row": ([C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_uint8, C.c_int32], C.c_int),
    "hc_set_members": ([C.c_void_p, C.c_int64], C.c_int),
    "hc_set_state": ([C.c_void_p, _dp, C.c_int], C.c_int),
    "hc_get_state": ([C.c_void_p, _dp, C.c_int64, C.c_int64], C.c_int),
    "hc_set_noise_host": ([C.c_void_p, _dp], C.c_int),
    "hc_get_noise_base": ([C.c_void_p, _dp, C.c_int64, C.c_int64], C.c_int),
    "hc_set_noise_philox": ([C.c_void_p, C.c_uint64, C.c_int64], C.c_int),
    "hc_philox_normals": ([C.c_void_p, C.c_int64, C.c_int64, _dp], C.c_int),
    "hc_set_noise_correlation": ([C.c_void_p, _dp, _dp], C.c_int),
    "hc_get_noise_correlation": ([C.c_void_p, _ip, _dp, _dp], C.c_int),
    "hc_noise_field_normals": ([C.c_void_p, C.c_int64, C.c_int64, _dp], C.c_int),
    "hc_get_noise_field_base": ([C.c_void_p, _dp, C.c_int64, C.c_int64], C.c_int),
    "hc_set_noise_field_base": ([C.c_void_p, _dp], C.c_int),
    "hc_set_forcing_perturbation": ([C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_uint64], C.c_int),
    "hc_clear_forcing_perturbation": ([C.c_void_p], C.c_int),
    "hc_set_forcing_member_offset": ([C.c_void_p, C.c_int64], C.c_int),
    "hc_get_forcing_perturbation": ([C.c_void_p, _ip, _dp, _dp, _dp, _dp, C.POINTER(C.c_uint64)], C.c_int),
    "hc_get_forcing_state": ([C.c_void_p, _dp, C.POINTER(C.c_int64)], C.c_int),
    "hc_set_forcing_state": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_forcing_normals": ([C.c_void_p, C.c_int64, C.c_int64, C.c_int64, _dp], C.c_int),
    "hc_forcing_factors": ([C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _dp], C.c_int),
    "hc_step_rows": ([C.c_void_p, C.POINTER(StepArgs)], C.c_int),
    "hc_spinup": ([C.c_void_p, C.POINTER(SpinupArgs)], C.c_int),
    "hc_synchronize": ([C.c_void_p], C.c_int),
    "hc_get_counters": ([C.c_void_p, C.POINTER(C.c_uint64)], C.c_int),
    "hc_set_generic_exponents": ([C.c_void_p, C.c_int32], C.c_int),
    "hc_set_rows_per_launch": ([C.c_void_p, C.c_int32], C.c_int),
    "hc_set_iteration_budget": ([C.c_void_p, C.c_int32], C.c_int),
    "hc_set_scipy_152": ([C.c_void_p, C.c_int32], C.c_int),
    "hc_get_moments": ([C.c_void_p, _lp], C.c_int),
    "hc_export_moments": ([C.c_void_p, C.c_void_p], C.c_int),
    "hc_set_moments": ([C.c_void_p, _lp], C.c_int),
    "hc_reset_moments": ([C.c_void_p], C.c_int),
    "hc_allreduce_moments": ([C.POINTER(C.c_void_p), C.c_int], C.c_int),
    "hc_get_noise_scale": ([C.c_void_p, _dp, C.c_int64, C.c_int64], C.c_int),
    "hc_set_noise_scale": ([C.c_void_p, _dp, C.c_int64, C.c_int64], C.c_int),
    "hc_set_point_member_bases": ([C.c_void_p, _lp], C.c_int),
    "hc_get_point_costs": ([C.c_void_p, C.POINTER(C.c_uint64)], C.c_int),
    "hc_set_profile_stats": ([C.c_void_p, C.c_int32], C.c_int),
    "hc_get_profile_stats_words": ([C.c_void_p, _lp], C.c_int),
    "hc_profile_snapshot": ([C.c_void_p, C.c_int64], C.c_int),
    "hc_get_profile_stats": ([C.c_void_p, _lp, C.c_int64], C.c_int),
    "hc_set_profile_stats_tables": ([C.c_void_p, _lp, C.c_int64], C.c_int),
    "hc_export_profile_stats": ([C.c_void_p, C.c_void_p, C.c_int64], C.c_int),
    "hc_reset_profile_stats": ([C.c_void_p], C.c_int),
    "hc_get_profile_overflow": ([C.c_void_p, C.POINTER(C.c_uint64)], C.c_int),
    "hc_set_wtd_hist": ([C.c_void_p, C.c_int32], C.c_int),
    "hc_get_wtd_hist": ([C.c_void_p, _ip, C.c_int64], C.c_int),
    "hc_set_wtd_hist_table": ([C.c_void_p, _ip, C.c_int64], C.c_int),
    "hc_reset_wtd_hist": ([C.c_void_p], C.c_int),
    "hc_set_theta_hist": ([C.c_void_p, C.c_int32], C.c_int),
    "hc_get_theta_hist": ([C.c_void_p, _ip, C.c_int64], C.c_int),
    "hc_set_theta_hist_table": ([C.c_void_p, _ip, C.c_int64], C.c_int),
    "hc_reset_theta_hist": ([C.c_void_p], C.c_int),
    "hc_get_theta_hist_outside": ([C.c_void_p, C.POINTER(C.c_uint64)], C.c_int),
    "hc_get_theta_hist_bins": ([C.c_void_p, _ip], C.c_int),
    "hc_set_layer_storage": ([C.c_void_p, C.c_int32, _ip, C.c_int32], C.c_int),
    "hc_get_layer_storage_words": ([C.c_void_p, _lp], C.c_int),
    "hc_get_layer_storage": ([C.c_void_p, _lp, C.c_int64], C.c_int),
    "hc_set_layer_storage_tables": ([C.c_void_p, _lp, C.c_int64], C.c_int),
    "hc_export_layer_storage": ([C.c_void_p, C.c_void_p, C.c_int64], C.c_int),
    "hc_get_layer_storage_hist": ([C.c_void_p, _ip, C.c_int64], C.c_int),
    "hc_set_layer_storage_hist_table": ([C.c_void_p, _ip, C.c_int64], C.c_int),
    "hc_reset_layer_storage": ([C.c_void_p], C.c_int),
    "hc_get_layer_storage_outside": ([C.c_void_p, C.POINTER(C.c_uint64)], C.c_int),
    "hc_get_layer_storage_overflow": ([C.c_void_p, C.POINTER(C.c_uint64)], C.c_int),
    "hc_get_layer_storage_layout": ([C.c_void_p, _ip, _ip, _ip], C.c_int),
    "hc_set_conductivity_stats": ([C.c_void_p, C.c_int32, _ip], C.c_int),
    "hc_clear_conductivity_stats": ([C.c_void_p], C.c_int),
    "hc_get_conductivity_stats_words": ([C.c_void_p, _lp], C.c_int),
    "hc_get_conductivity_stats": ([C.c_void_p, _lp, C.c_int64], C.c_int),
    "hc_set_conductivity_stats_tables": ([C.c_void_p, _lp, C.c_int64], C.c_int),
    "hc_export_conductivity_stats": ([C.c_void_p, C.c_void_p, C.c_int64], C.c_int),
    "hc_reset_conductivity_stats": ([C.c_void_p], C.c_int),
    "hc_get_conductivity_stats_layout": ([C.c_void_p, _ip, _ip, _ip], C.c_int),
    "hc_get_conductivity_stats_overflow": ([C.c_void_p, C.POINTER(C.c_uint64)], C.c_int),
    "hc_conductivity_eval": ([C.c_void_p, C.c_int64, _dp], C.c_int),
    "hc_set_theta_cov": ([C.c_void_p, C.c_int32], C.c_int),
    "hc_get_theta_cov_layout": ([C.c_void_p, _ip, _ip, _lp], C.c_int),
    "hc_get_theta_cov_words": ([C.c_void_p, _lp], C.c_int),
    "hc_get_theta_cov": ([C.c_void_p, _lp, C.c_int64], C.c_int),
    "hc_set_theta_cov_tables": ([C.c_void_p, _lp, C.c_int64], C.c_int),
    "hc_export_theta_cov": ([C.c_void_p, C.c_void_p, C.c_int64], C.c_int),
    "hc_reset_theta_cov": ([C.c_void_p], C.c_int),
    "hc_get_theta_cov_outside": ([C.c_void_p, C.POINTER(C.c_uint64)], C.c_int),
    "hc_set_period_totals": ([C.c_void_p, C.c_int32, _lp, C.c_int32, _ip, C.c_int32, _ip], C.c_int),
    "hc_get_period_totals_words": ([C.c_void_p, _lp], C.c_int),
    "hc_get_period_totals": ([C.c_void_p, _lp, C.c_int64], C.c_int),
    "hc_set_period_totals_tables": ([C.c_void_p, _lp, C.c_int64], C.c_int),
    "hc_export_period_totals": ([C.c_void_p, C.c_void_p, C.c_int64], C.c_int),
    "hc_get_period_totals_hist": ([C.c_void_p, _ip, C.c_int64], C.c_int),
    "hc_set_period_totals_hist_table": ([C.c_void_p, _ip, C.c_int64], C.c_int),
    "hc_export_period_totals_hist": ([C.c_void_p, C.c_void_p, C.c_int64], C.c_int),
    "hc_get_period_totals_acc": ([C.c_void_p, _lp, C.c_int64], C.c_int),
    "hc_set_period_totals_acc": ([C.c_void_p, _lp, C.c_int64], C.c_int),
    "hc_reset_period_totals": ([C.c_void_p], C.c_int),
    "hc_get_period_totals_outside": ([C.c_void_p, C.POINTER(C.c_uint64)], C.c_int),
    "hc_get_period_totals_overflow": ([C.c_void_p, C.POINTER(C.c_uint64)], C.c_int),
    "hc_get_period_totals_layout": ([C.c_void_p, _ip, _ip, _ip, _ip, _ip, _lp, C.c_int64], C.c_int),
    "hc_set_root_uptake": ([C.c_void_p, C.c_int32, _ip, _ip, C.c_int32], C.c_int),
    "hc_get_root_uptake_words": ([C.c_void_p, _lp], C.c_int),
    "hc_get_root_uptake": ([C.c_void_p, _lp, C.c_int64], C.c_int),
    "hc_set_root_uptake_tables": ([C.c_void_p, _lp, C.c_int64], C.c_int),
    "hc_export_root_uptake": ([C.c_void_p, C.c_void_p, C.c_int64], C.c_int),
    "hc_get_root_uptake_hist": ([C.c_void_p, _ip, C.c_int64], C.c_int),
    "hc_set_root_uptake_hist_table": ([C.c_void_p, _ip, C.c_int64], C.c_int),
    "hc_export_root_uptake_hist": ([C.c_void_p, C.c_void_p, C.c_int64], C.c_int),
    "hc_get_root_uptake_acc": ([C.c_void_p, _lp, C.c_int64], C.c_int),
    "hc_set_root_uptake_acc": ([C.c_void_p, _lp, C.c_int64], C.c_int),
    "hc_reset_root_uptake": ([C.c_void_p], C.c_int),
    "hc_get_root_uptake_outside": ([C.c_void_p, C.POINTER(C.c_uint64)], C.c_int),
    "hc_get_root_uptake_overflow": ([C.c_void_p, C.POINTER(C.c_uint64)], C.c_int),
    "hc_get_root_uptake_layout": ([C.c_void_p, _ip, _ip, _ip, _ip], C.c_int),
    "hc_root_uptake_eval": ([C.c_void_p, C.c_int64, _dp, _dp], C.c_int),
    "hc_wtd_distribution": ([C.c_int, _ip, _ip, C.c_int64, C.c_int32, _dp, C.c_int32, C.c_double, _lp, _ip, _dp], C.c_int),
    "hc_set_filter": ([C.c_void_p, C.c_int32, C.c_double, C.c_uint64], C.c_int),
    "hc_get_filter_stats": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_set_filter_stats": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_get_filter_base": ([C.c_void_p, _dp, C.c_int64, C.c_int64], C.c_int),
    "hc_set_filter_base": ([C.c_void_p, _dp], C.c_int),
    "hc_get_filter_ancestors": ([C.c_void_p, _lp], C.c_int),
    "hc_get_filter_weights": ([C.c_void_p, _lp], C.c_int),
    "hc_get_filter_draw": ([C.c_void_p, _lp], C.c_int),
    "hc_set_filter_soil_moisture": ([C.c_void_p, C.c_int32, _ip, _dp, _dp], C.c_int),
    "hc_get_filter_sm_stats": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_set_filter_sm_stats": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_get_filter_sm_width": ([C.c_void_p, _ip], C.c_int),
    "hc_get_filter_member_weights": ([C.c_void_p, _lp], C.c_int),
    "hc_get_filter_loglik": ([C.c_void_p, _dp], C.c_int),
    "hc_get_filter_sm_theta": ([C.c_void_p, _dp], C.c_int),
    "hc_set_filter_window": ([C.c_void_p, C.c_int32, _ip], C.c_int),
    "hc_get_filter_window_stats": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_set_filter_window_stats": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_get_filter_window_capture": ([C.c_void_p, _ip, _lp], C.c_int),
    "hc_set_filter_window_capture": ([C.c_void_p, _ip, _lp], C.c_int),
    "hc_get_filter_window_width": ([C.c_void_p, _ip, _ip], C.c_int),
    "hc_set_filter_smoother": ([C.c_void_p, C.c_int32, C.c_int32], C.c_int),
    "hc_get_filter_smoother_layout": ([C.c_void_p, _ip, _ip, _lp], C.c_int),
    "hc_get_filter_smoother_hist": ([C.c_void_p, _ip, C.c_int64], C.c_int),
    "hc_set_filter_smoother_hist_table": ([C.c_void_p, _ip, C.c_int64], C.c_int),
    "hc_get_filter_smoother_paths": ([C.c_void_p, _lp, C.c_int64], C.c_int),
    "hc_set_filter_smoother_paths": ([C.c_void_p, _lp, C.c_int64], C.c_int),
    "hc_get_filter_smoother_ring": ([C.c_void_p, _ip, _lp, _lp, _lp], C.c_int),
    "hc_set_filter_smoother_ring": ([C.c_void_p, _ip, _lp, _lp, C.c_int64], C.c_int),
    "hc_filter_smoother_flush": ([C.c_void_p], C.c_int),
    "hc_reset_filter_smoother": ([C.c_void_p], C.c_int),
    "hc_set_filter_tempering": ([C.c_void_p, C.c_double], C.c_int),
    "hc_get_filter_temper_stats": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_set_filter_temper_stats": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_get_filter_temper_trials": ([C.c_void_p, _lp], C.c_int),
    "hc_set_filter_rejuvenation": ([C.c_void_p, C.c_double], C.c_int),
    "hc_get_filter_rejuvenation": ([C.c_void_p, _dp, _dp], C.c_int),
    "hc_get_filter_rejuvenation_stats": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_set_filter_rejuvenation_stats": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_get_filter_rejuvenation_moments": ([C.c_void_p, _dp], C.c_int),
    "hc_filter_rejuvenation_normals": ([C.c_void_p, C.c_int64, C.c_int64, C.c_int64, _dp], C.c_int),
    "hc_set_enkf": ([C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_uint64], C.c_int),
    "hc_get_enkf_stats": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_set_enkf_stats": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_get_enkf_gain": ([C.c_void_p, _dp], C.c_int),
    "hc_get_enkf_y": ([C.c_void_p, _dp], C.c_int),
    "hc_get_enkf_eps": ([C.c_void_p, _dp], C.c_int),
    "hc_set_enkf_soil_moisture": ([C.c_void_p, C.c_int32, _ip, _dp, _dp], C.c_int),
    "hc_get_enkf_sm_stats": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_set_enkf_sm_stats": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_get_enkf_sm_width": ([C.c_void_p, _ip], C.c_int),
    "hc_get_enkf_sm_y": ([C.c_void_p, _dp], C.c_int),
    "hc_get_enkf_sm_gain": ([C.c_void_p, _dp], C.c_int),
    "hc_get_enkf_sm_eps": ([C.c_void_p, _dp], C.c_int),
    "hc_set_enkf_method": ([C.c_void_p, C.c_int32, C.c_double], C.c_int),
    "hc_get_enkf_method": ([C.c_void_p, _ip, _dp], C.c_int),
    "hc_get_enkf_sqrt_gain": ([C.c_void_p, _dp], C.c_int),
    "hc_get_enkf_sqrt_shift": ([C.c_void_p, _dp], C.c_int),
    "hc_get_enkf_relaxation": ([C.c_void_p, _dp, _dp, _dp], C.c_int),
    "hc_set_enkf_noise_field": ([C.c_void_p, C.c_int32, C.c_double], C.c_int),
    "hc_get_enkf_noise_field": ([C.c_void_p, C.POINTER(C.c_int32), _dp], C.c_int),
    "hc_get_enkf_noise_stats": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_set_enkf_noise_stats": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_get_enkf_noise_gain": ([C.c_void_p, _dp], C.c_int),
    "hc_get_enkf_noise_sqrt_gain": ([C.c_void_p, _dp], C.c_int),
    "hc_get_enkf_noise_sqrt_shift": ([C.c_void_p, _dp], C.c_int),
    "hc_set_enkf_forcing": ([C.c_void_p, C.c_int32, C.c_double], C.c_int),
    "hc_get_enkf_forcing": ([C.c_void_p, C.POINTER(C.c_int32), _dp], C.c_int),
    "hc_get_enkf_g_table": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_set_enkf_g_table": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_get_enkf_g_gain": ([C.c_void_p, _dp], C.c_int),
    "hc_get_enkf_g_sqrt_gain": ([C.c_void_p, _dp], C.c_int),
    "hc_get_enkf_g_sqrt_shift": ([C.c_void_p, _dp], C.c_int),
    "hc_get_enkf_noise_base": ([C.c_void_p, _dp, C.c_int64, C.c_int64], C.c_int),
    "hc_set_enkf_noise_base": ([C.c_void_p, _dp], C.c_int),
    "hc_set_enkf_window": ([C.c_void_p, C.c_int32, _ip], C.c_int),
    "hc_get_enkf_window_stats": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_set_enkf_window_stats": ([C.c_void_p, _dp, C.c_int64], C.c_int),
    "hc_get_enkf_window_capture": ([C.c_void_p, _dp, _lp], C.c_int),
    "hc_set_enkf_window_capture": ([C.c_void_p, _dp, _lp], C.c_int),
    "hc_get_enkf_width": ([C.c_void_p, _ip], C.c_int),
    "hc_get_enkf_window_width": ([C.c_void_p, _ip, _ip], C.c_int),
    "hc_get_enkf_window_y": ([C.c_void_p, _dp], C.c_int),
    "hc_get_enkf_window_eps": ([C.c_void_p, _dp], C.c_int),
    "hc_get_enkf_window_gain": ([C.c_void_p, _dp], C.c_int),
    "hc_get_enkf_shard_words": ([C.c_void_p, C.c_int64, _lp], C.c_int),
    "hc_set_enkf_shard": ([C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, EXCHANGE_FN, C.c_void_p], C.c_int),
    "hc_get_enkf_shard": ([C.c_void_p, _lp, _lp], C.c_int),
    "hc_get_filter_shard_words": ([C.c_void_p, C.c_int32, _lp, C.c_int32, _lp], C.c_int),
    "hc_set_filter_shard": ([C.c_void_p, C.c_int32, _lp, C.c_int32, C.c_void_p, C.c_int64, EXCHANGE_FN, ROUTE_FN, C.c_void_p],
                            C.c_int),
    "hc_get_filter_shard": ([C.c_void_p, _ip, _ip, _lp], C.c_int),
    "hc_rhs": ([C.c_void_p, C.c_int64, C.c_int32, _dp, _dp], C.c_int),
    "hc_rhs_ex": ([C.c_void_p, C.c_int64, C.c_int32, C.c_int32, _dp, _dp, _dp], C.c_int),
    "hc_model_nodes": ([C.c_void_p, _dp, _dp], C.c_int),
    "hc_plugin_eval": ([C.c_int, C.POINTER(ColumnParams), C.c_int64, C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _dp],
                       C.c_int),
}

# hc_rhs_ex's `variant` (include/hydrocol.h: HC_RHS_HOOK, HC_RHS_AS_STEPPED, HC_RHS_HOOK_LAYOUT)
RHS_VARIANTS = {"hook": 0, "step": 1, "hook_layout": 2}

_lib = None
_torch_first = False       # torch was in the process before the library: the two use ONE HIP runtime (torch's)


def load(with_torch=False):
    """Load libhydrocol.so; raises if it has not been built.

    ``with_torch``: the caller will hand the library device memory that torch allocated (the buffer of hc_set_enkf_shard
    or hc_set_filter_shard).
    torch ships a HIP runtime of its own, and the loader gives the library that one only when torch is in the process
    first; loaded the other way round, the process holds two runtimes and torch's finds no GPU.  So torch is imported
    here before the library, and a process that loaded the library before torch is an error, not a second runtime."""
    global _lib, _torch_first
    if with_torch and _lib is None:
        import torch  # noqa: F401
    if _lib is None:
        _torch_first = "torch" in sys.modules
    if with_torch and not _torch_first:
        raise HcError("libhydrocol was loaded before torch, so torch would bring a second HIP runtime into this process: "
                      "import torch before the first hydromodel_amd handle is made (EnsembleSimulation(enkf_shard=...) "
                      "and the CLI do so themselves)")
    if _lib is None:
        if not LIB_PATH.exists():
            raise HcError(f"{LIB_PATH} is missing: the HIP extension has not been built "
                          f"(run __graft_entry__.build()); there is no CPU fallback")
        lib = C.CDLL(str(LIB_PATH))
        for name, (argtypes, restype) in EXPORTS.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = lib
    return _lib


def kernel_hash():
    """The device-code identity the loaded library was built with (hc_version(): "... kernels <hash>")."""
    v = load().hc_version().decode()
    return v.rsplit("kernels ", 1)[1] if "kernels " in v else "unknown"


def check(rc):
    if rc != 0:
        raise HcError(f"libhydrocol status {rc}: {load().hc_last_error().decode()}")


def dptr(a):
    return a.ctypes.data_as(_dp)


def iptr(a):
    return a.ctypes.data_as(_ip)


def bptr(a):
    return a.ctypes.data_as(_bp)


def lptr(a):
    return a.ctypes.data_as(_lp)


def as_f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)
