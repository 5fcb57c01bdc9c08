"""EnsembleStepper: Python face of one libhydrocol handle (one GPU, one parameter point).

Mirrors what ``Simulation.run`` does per row (``/root/reference/code/src/simulation.py:576-626``)
for N ensemble members at once; see include/hydrocol.h for the entry points.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib as L
from .multigpu import place_points  # noqa: F401  (the sweep's tables over the ranks: place at point ids, sum)


def column_params(cols, surface_evap, flags=None):
    """Fill hc_column_params from a digest.ColumnTables."""
    fl = dict(cols.flags)
    if flags:
        fl.update(flags)
    p = L.ColumnParams()
    # PREDICT: the reference raises TypeError at richards_pde.py:327-330 (np.linspace with a float count).  The stepper
    # runs the repaired form -- `low_lim` as an int, nothing drains when it is <= 0 -- as a declared extension with
    # no reference oracle; Simulation / the CLI only reach it with "Ensemble": {"repair_predict": true}.
    p.flag_predict = int(bool(fl.get("PREDICT")))
    p.sat_cells = int(cols.sat_cells)
    p.dim_d, p.model = cols.dim_d, cols.model
    p.flag_et, p.flag_lf, p.flag_hlift = int(fl["ET"]), int(fl["LF"]), int(fl["HLIFT"])
    p.n_root_first, p.n_root_int, p.n_groups = cols.n_root_first, cols.n_root_int, cols.n_groups
    p.theta_res, p.alpha, p.n, p.m = cols.theta.res, cols.soil.alpha, cols.soil.n, cols.soil.m
    p.psi_sat, p.epsilon = cols.soil.psi_sat, max(cols.soil.epsilon, 1.0e-8)
    p.lambda_exp, p.sigma_noise, p.sat_soil = (cols.k_hc.lambda_exponent, cols.k_hc.sigma_noise,
                                               cols.k_hc.sat_soil)
    p.dz, p.ipsi50, p.lai = cols.dz, cols.ipsi50, cols.lai
    p.surface_evap, p.interception = surface_evap, cols.interception
    p.evap_delta_min = cols.evap_delta_min
    return p


class EnsembleStepper:
    """N members x D depth nodes on one MI355X.

    ``cols`` is one ``digest.ColumnTables`` or a sequence of them (parameter points of a sweep sharing grid and
    forcing): with P points the N members are point-major, point k owns members [k N/P, (k+1) N/P), and one launch
    advances all of them; ``moments()`` then returns [P][3][T]."""

    conductivity, conductivity_ranges = False, np.zeros((0, 2), dtype=np.int32)      # (off until set_conductivity_stats)

    def __init__(self, cols, forcing, n_members, device=0, flags=None, profile_stride=0):
        self.lib = L.load()
        points = list(cols) if isinstance(cols, (list, tuple)) else [cols]
        cols = points[0]
        self.points, self.P = points, len(points)
        self.cols, self.forcing = cols, forcing
        self.D, self.N, self.T = cols.dim_d, int(n_members), forcing.dim_t
        if self.N % self.P:
            raise ValueError(f"{self.N} members do not divide into {self.P} parameter points")
        h = C.c_void_p()
        L.check(self.lib.hc_create(int(device), C.byref(h)))
        self.h = h
        self.params = column_params(cols, forcing.surface_evap, flags)
        node, mid = L.as_f64(cols.node_table()), L.as_f64(cols.mid_table())
        groups = np.ascontiguousarray(cols.groups, dtype=np.int32)
        L.check(self.lib.hc_set_column(self.h, C.byref(self.params), L.dptr(node), L.dptr(mid), L.iptr(groups)))
        for pt in points[1:]:
            if pt.dim_d != self.D or not np.array_equal(pt.z, cols.z):
                raise ValueError("parameter points must share the depth grid")
            pp = column_params(pt, forcing.surface_evap, flags)
            node, mid = L.as_f64(pt.node_table()), L.as_f64(pt.mid_table())
            L.check(self.lib.hc_add_point(self.h, C.byref(pp), L.dptr(node), L.dptr(mid)))
        precip, atm = L.as_f64(forcing.precip), L.as_f64(forcing.atm)
        # bit 0: daylight, bit 1: wet season (read in PREDICT mode only), include/hydrocol.h
        day = np.ascontiguousarray(forcing.daylight | (forcing.wet_season << 1), dtype=np.uint8)
        wobs = np.ascontiguousarray(forcing.wtd_obs, dtype=np.int32)
        refr = np.ascontiguousarray(forcing.refresh, dtype=np.uint8)
        L.check(self.lib.hc_set_forcing(self.h, self.T, L.dptr(precip), L.dptr(atm), L.bptr(day),
                                        L.iptr(wobs), L.bptr(refr)))
        L.check(self.lib.hc_set_members(self.h, self.N))
        self.last_kernel_ms = 0.0
        self.last_launches = 0
        self.profile_stride = 0
        self.wtd_hist_stride = 0
        self.theta_hist_bins = 0
        self.storage_ranges, self.storage_bins = np.zeros((0, 2), dtype=np.int32), 0
        self.theta_cov_stride = 0
        self.conductivity, self.conductivity_ranges = False, np.zeros((0, 2), dtype=np.int32)
        self.period_ends, self.period_threshold_nodes = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32)
        self.period_bins, self.period_flux_max_log2 = 0, (0, 0)
        self.uptake_cells, self.uptake_bins = np.zeros((0, 2), dtype=np.int32), 0
        self.filter_stride, self.filter_sigma_cm, self.filter_seed = 0, 0.0, 0
        self.filter_sm_nodes = None
        self.filter_ess_floor = 0.0
        self.filter_rejuvenation = 0.0
        self.filter_window_offsets = ()
        self.filter_smoother = (0, 0)
        self.enkf_stride, self.enkf_sigma_cm, self.enkf_localisation_cm, self.enkf_seed = 0, 0.0, 0.0, 0
        self.enkf_sm_nodes = None
        self.enkf_method, self.enkf_relaxation = "stochastic", 0.0
        self.enkf_window_offsets = ()
        self.enkf_noise_field, self.enkf_noise_relaxation = False, 0.0
        self.enkf_forcing, self.enkf_forcing_relaxation = False, 0.0
        self.noise_corr = None
        self.philox = False
        self.device = int(device)
        self.enkf_shard, self._shard_keep, self._shard_error = None, None, None
        self.filter_shard, self._filter_shard_keep = None, None
        if profile_stride:
            self.set_profile_stats(profile_stride)

    def close(self):
        if getattr(self, "h", None):
            self.lib.hc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    # -- state / noise -------------------------------------------------------------
    def set_state(self, psi):
        psi = L.as_f64(psi)
        if psi.shape == (self.D,):
            L.check(self.lib.hc_set_state(self.h, L.dptr(psi), 1))
        elif psi.shape == (self.N, self.D):
            L.check(self.lib.hc_set_state(self.h, L.dptr(psi), 0))
        elif psi.shape == (self.P, self.D):                       # one column per parameter point
            L.check(self.lib.hc_set_state(self.h, L.dptr(psi), 2))
        else:
            raise ValueError(f"state must be [{self.D}], [{self.P}, {self.D}] (per point) or "
                             f"[{self.N}, {self.D}], got {psi.shape}")

    def get_state(self, first=0, count=None):
        count = self.N - first if count is None else count
        out = np.empty((count, self.D))
        L.check(self.lib.hc_get_state(self.h, L.dptr(out), first, count))
        return out

    def set_noise_host(self, base):
        base = L.as_f64(base)
        if base.shape != (self.N, self.D):
            raise ValueError(f"base noise must be [{self.N}, {self.D}]")
        L.check(self.lib.hc_set_noise_host(self.h, L.dptr(base)))
        self.philox = False
        self._filter_off()

    def get_noise_base(self, first=0, count=None):
        count = self.N - first if count is None else count
        out = np.empty((count, self.D))
        L.check(self.lib.hc_get_noise_base(self.h, L.dptr(out), first, count))
        return out

    def set_noise_philox(self, seed, member_offset=0):
        L.check(self.lib.hc_set_noise_philox(self.h, int(seed), int(member_offset)))
        self.philox = True
        self._filter_off()

    def philox_normals(self, member, draw):
        out = np.empty(self.D)
        L.check(self.lib.hc_philox_normals(self.h, int(member), int(draw), L.dptr(out)))
        return out

    # -- correlated noise fields (include/hydrocol.h hc_set_noise_correlation) ------------------------------------------
    def set_noise_correlation(self, a, b=None):
        """Correlate the Philox source's vectors down the column by the recursion of :func:`noise_correlate` with the
        tables ``a``, ``b`` ([D] for every point, or [P][D]; :func:`noise_correlation_tables` builds them); ``None``
        turns it off.  Needs a Philox run.  The handle then feeds the step kernel its own normals as caller noise: set
        it after the spin-up and before a particle filter or the EnKF's noise field, and :meth:`set_noise_scale` is
        refused while it is on."""
        if a is None:
            L.check(self.lib.hc_set_noise_correlation(self.h, None, None))
            self.noise_corr = None
            return
        if b is None:
            raise ValueError("the noise correlation needs both tables, a and b")
        a, b = L.as_f64(a), L.as_f64(b)
        if a.shape == (self.D,) and b.shape == (self.D,):
            a, b = L.as_f64(np.tile(a, (self.P, 1))), L.as_f64(np.tile(b, (self.P, 1)))
        if a.shape != (self.P, self.D) or b.shape != (self.P, self.D):
            raise ValueError(f"the noise correlation's tables must be [{self.D}] or [{self.P}, {self.D}], got {a.shape} and {b.shape}")
        self.noise_corr = None                   # (hc_set_noise_correlation leaves it off if it refuses)
        L.check(self.lib.hc_set_noise_correlation(self.h, L.dptr(a), L.dptr(b)))
        self.noise_corr = (a.copy(), b.copy())

    def noise_correlation(self):
        """``None`` while it is off, else the tables (a, b), each [P][D], as the library holds them."""
        on = np.zeros(1, dtype=np.int32)
        a, b = np.zeros((self.P, self.D)), np.zeros((self.P, self.D))
        L.check(self.lib.hc_get_noise_correlation(self.h, L.iptr(on), L.dptr(a), L.dptr(b)))
        return (a, b) if on[0] else None

    def noise_field_normals(self, member, draw):
        """[D] what the noise source now yields for (member, draw), unscaled (test hook): :meth:`philox_normals` run
        through the correlation when one is set."""
        out = np.empty(self.D)
        L.check(self.lib.hc_noise_field_normals(self.h, int(member), int(draw), L.dptr(out)))
        return out

    def noise_field_base(self):
        """[N][D] base noise vectors of a Philox run with a correlation set (a checkpoint's)."""
        out = np.empty((self.N, self.D))
        L.check(self.lib.hc_get_noise_field_base(self.h, L.dptr(out), 0, self.N))
        return out

    def set_noise_field_base(self, base):
        base = L.as_f64(base)
        if base.shape != (self.N, self.D):
            raise ValueError(f"base noise must be [{self.N}, {self.D}]")
        L.check(self.lib.hc_set_noise_field_base(self.h, L.dptr(base)))

    # -- perturbed forcing (include/hydrocol.h hc_set_forcing_perturbation) --------------------------------------------
    def set_forcing_perturbation(self, precipitation_sigma=0.0, demand_sigma=0.0, correlation_days=0.0, seed=0, phi=None,
                                 c=None, member_offset=None):
        """Give every member its own log-normal factor of mean one on the rainfall and on the atmospheric demand, per
        day (row // 48), an AR(1) in time with e-folding time ``correlation_days`` (or explicit ``phi``, ``c``); the
        recursion is :func:`forcing_recursion_of`.  Both sigmas 0 keeps every factor at exactly 1.0 on the wider build.
        ``None`` as the first argument turns it off.  Set it after the spin-up and before a filter.  The members are
        keyed by the global ids of their noise streams; ``member_offset`` gives the first member's id where there is no
        such stream (a shard of a host-noise ensemble: otherwise its ids start at 0)."""
        self.enkf_forcing, self.enkf_forcing_relaxation = False, 0.0     # (the library turns the EnKF's part off with it)
        if precipitation_sigma is None:
            L.check(self.lib.hc_clear_forcing_perturbation(self.h))
            return
        if phi is None:
            phi, c = forcing_coefficients(correlation_days)
        L.check(self.lib.hc_set_forcing_perturbation(self.h, float(precipitation_sigma), float(demand_sigma), float(phi),
                                                     float(c), int(seed)))
        if member_offset is not None:
            L.check(self.lib.hc_set_forcing_member_offset(self.h, int(member_offset)))

    def forcing_perturbation(self):
        """``None`` while it is off, else ``{"precipitation_sigma", "demand_sigma", "phi", "c", "seed"}`` as the library
        holds them."""
        on = np.zeros(1, dtype=np.int32)
        v = np.zeros(4)
        seed = C.c_uint64(0)
        L.check(self.lib.hc_get_forcing_perturbation(self.h, L.iptr(on), L.dptr(v[0:]), L.dptr(v[1:]), L.dptr(v[2:]),
                                                     L.dptr(v[3:]), C.byref(seed)))
        if not on[0]:
            return None
        return {"precipitation_sigma": float(v[0]), "demand_sigma": float(v[1]), "phi": float(v[2]), "c": float(v[3]),
                "seed": int(seed.value)}

    def forcing_state(self):
        """(g [2][N], day): the members' AR(1) state of the two streams and the day it stands at (-1: no row stepped
        yet); a checkpoint's."""
        g = np.empty((2, self.N))
        day = C.c_int64(0)
        L.check(self.lib.hc_get_forcing_state(self.h, L.dptr(g), C.byref(day)))
        return g, int(day.value)

    def set_forcing_state(self, g, day):
        g = L.as_f64(g)
        if g.shape != (2, self.N):
            raise ValueError(f"the forcing state must be [2, {self.N}]")
        L.check(self.lib.hc_set_forcing_state(self.h, L.dptr(g), int(day)))

    def forcing_normals(self, member, first_day, n_days):
        """[n_days][2] the raw normals xi of the stream key ``member`` (a global id) for the two streams (test hook)."""
        out = np.empty((int(n_days), 2))
        L.check(self.lib.hc_forcing_normals(self.h, int(member), int(first_day), int(n_days), L.dptr(out)))
        return out

    def forcing_factors(self, first_member, count, first_day, n_days):
        """[n_days][2][count] the factors of the handle's slots first_member ... by the stateless recursion from day 0, on
        the device code that fills them for the step kernel (valid for slots that neither a resampling nor an analysis
        of :meth:`set_enkf_forcing` has touched)."""
        out = np.empty((int(n_days), 2, int(count)))
        L.check(self.lib.hc_forcing_factors(self.h, int(first_member), int(count), int(first_day), int(n_days), L.dptr(out)))
        return out

    # -- stepping ------------------------------------------------------------------
    def n_refresh(self, row_begin, n_rows):
        """Noise vectors rows [row_begin, row_begin + n_rows) consume: refresh rows that are actually solved (a row
        whose observation is off the grid is skipped before anything is drawn, simulation.py:582-602)."""
        sl = slice(row_begin, row_begin + n_rows)
        return int((self.forcing.refresh[sl].astype(bool) & (self.forcing.wtd_obs[sl] >= 0)).sum())

    def step_rows(self, row_begin, n_rows, fresh_noise=None, spinup=False, moments=True,
                  want_wtd=False, want_stats=False, want_psi=False, want_diag=False):
        a = L.StepArgs()
        a.row_begin, a.n_rows, a.spinup = int(row_begin), int(n_rows), int(spinup)
        a.accumulate_moments = int(moments and not spinup)     # spin-up solves belong to no forcing row
        keep = []
        if fresh_noise is not None:
            fresh_noise = L.as_f64(fresh_noise)
            need = 0 if spinup else self.n_refresh(row_begin, n_rows)
            if fresh_noise.size != need * self.N * self.D:
                raise ValueError(f"fresh_noise must hold {need} x [{self.N}, {self.D}] values")
            a.fresh_noise = L.dptr(fresh_noise)
            keep.append(fresh_noise)
        out = {}
        if want_wtd:
            out["wtd"] = np.zeros((n_rows, self.N), dtype=np.int32)
            a.wtd_out = L.iptr(out["wtd"])
        if want_stats:
            out["stats"] = np.zeros((n_rows, self.N, 6), dtype=np.int32)
            a.stats_out = L.iptr(out["stats"])
        if want_psi:
            out["psi"] = np.zeros((n_rows, self.N, self.D))
            a.psi_rows_out = L.dptr(out["psi"])
        if want_diag:
            out["diag"] = np.zeros((n_rows, self.N, 2))
            a.diag_out = L.dptr(out["diag"])
        rc = self.lib.hc_step_rows(self.h, C.byref(a))
        failure, self._shard_error = self._shard_error, None
        if rc and failure is not None:             # the shard's exchange raised inside the call (set_enkf_shard,
            #                                            set_filter_shard)
            raise L.HcError(f"libhydrocol status {rc}: {self.lib.hc_last_error().decode()}") from failure
        L.check(rc)
        if want_stats:
            # slot 5 of the C-ABI record = refresh flag | failed attempts << 8 (include/hydrocol.h)
            out["failed"] = out["stats"][:, :, 5] >> 8
            out["stats"][:, :, 5] &= 0xFF
        self.last_kernel_ms, self.last_launches = a.kernel_ms, a.launches
        out["kernel_ms"], out["launches"] = a.kernel_ms, a.launches
        return out

    def counters(self):
        """{'jac_retry': ..., 'failed_attempts': ..., 'guard_trips': ...} since the handle was created."""
        out = (C.c_uint64 * 4)()
        L.check(self.lib.hc_get_counters(self.h, out))
        return {"jac_retry": int(out[0]), "failed_attempts": int(out[1]), "guard_trips": int(out[2]),
                "guard_last_member": int(out[3]) >> 24, "guard_last_row": int(out[3]) & 0xFFFFFF}

    def moments(self):
        """[3][T] (count, sum idx, sum idx^2 per forcing row); [P][3][T] when the handle holds P > 1 points."""
        m = np.zeros((self.P, 3, self.T), dtype=np.int64)
        L.check(self.lib.hc_get_moments(self.h, L.lptr(m)))
        return m[0] if self.P == 1 else m

    def export_moments(self, device_ptr):
        """Copy the moment table device-to-device to `device_ptr` (P * 3 * T int64 on this handle's device)."""
        L.check(self.lib.hc_export_moments(self.h, C.c_void_p(int(device_ptr))))

    def set_moments(self, m):
        m = np.ascontiguousarray(m, dtype=np.int64)
        if m.size != self.P * 3 * self.T:
            raise ValueError(f"moments must hold {self.P} x [3, {self.T}] values")
        L.check(self.lib.hc_set_moments(self.h, L.lptr(m)))

    def noise_scale(self, first=0, count=None):
        """Per-member damping of the Philox base vector, 0.8^(failed attempts on non-refresh rows) (richards_pde.py:522)."""
        count = self.N - first if count is None else count
        out = np.empty(count)
        L.check(self.lib.hc_get_noise_scale(self.h, L.dptr(out), int(first), int(count)))
        return out

    def set_noise_scale(self, scale, first=0):
        scale = L.as_f64(scale)
        L.check(self.lib.hc_set_noise_scale(self.h, L.dptr(scale), int(first), int(scale.size)))

    def set_point_member_bases(self, bases):
        """Global id of each parameter point's first member (Philox key of member j of point k = bases[k] + j)."""
        bases = np.ascontiguousarray(bases, dtype=np.int64)
        if bases.shape != (self.P,):
            raise ValueError(f"need one member base per parameter point ({self.P})")
        L.check(self.lib.hc_set_point_member_bases(self.h, L.lptr(bases)))
        self._filter_off()

    def point_costs(self):
        """RHS evaluations spent on each parameter point's members so far ([P]; zeros for a single point)."""
        out = (C.c_uint64 * self.P)()
        L.check(self.lib.hc_get_point_costs(self.h, out))
        return np.array(list(out), dtype=np.uint64)

    def set_generic_exponents(self, on=True):
        """Pin the generic-exponent cell model (include/hydrocol.h): same bits for a point alone or inside a sweep."""
        L.check(self.lib.hc_set_generic_exponents(self.h, int(bool(on))))

    def set_rows_per_launch(self, rows):
        """Rows per kernel launch; 0 = the library's choice (48 = one simulated day for >= 65 536 members, proportionally
        more for smaller ensembles, at most a year; shorter when per-row outputs are requested -- include/hydrocol.h)."""
        L.check(self.lib.hc_set_rows_per_launch(self.h, int(rows)))

    def set_iteration_budget(self, phase_steps):
        L.check(self.lib.hc_set_iteration_budget(self.h, int(phase_steps)))

    def set_scipy_152(self, on=True):
        """``select_initial_step`` as the reference's pinned scipy==1.5.2 has it (no clamp to the interval); default: scipy >= 1.9."""
        L.check(self.lib.hc_set_scipy_152(self.h, int(bool(on))))

    def reset_moments(self):
        L.check(self.lib.hc_reset_moments(self.h))

    # -- the diagnostic tables (DIAG_TABLES below): one path for every accumulated table of the handle ---------------
    def diag_counts(self):
        """The counts the handle's diagnostic tables are shaped by (:func:`diag_counts`), from its settings."""
        return diag_counts(self.P, self.T, self.D, self.N, self.profile_stride, self.wtd_hist_stride, self.theta_hist_bins,
                           len(self.storage_ranges), self.storage_bins, self.theta_cov_stride, len(self.period_ends),
                           len(self.period_threshold_nodes), self.period_bins, len(self.uptake_cells), self.uptake_bins,
                           len(self.conductivity_ranges))

    def diag_words(self, key):
        """Elements of the raw table ``key`` of DIAG_TABLES, trailing words included: the library's count where it has
        an entry point for it, else the layout's."""
        name = f"hc_get_{diag_entry(key).stem}_words"
        if name not in L.EXPORTS:
            return diag_layout(key, self.diag_counts())["words"][0]
        n = C.c_int64()
        L.check(getattr(self.lib, name)(self.h, C.byref(n)))
        return int(n.value)

    def diag_raw(self, key):
        """The raw device table ``key`` as the library hands it out: flat, the entry's element type, its trailing words
        (overflow, outside count) included."""
        e = diag_entry(key)
        t = np.zeros(self.diag_words(key), dtype=e.dtype)
        L.check(getattr(self.lib, "hc_get_" + e.stem)(self.h, _diag_ptr(t), t.size))
        return t

    def set_diag_raw(self, key, raw):
        """Install a raw table (a checkpoint's, a sum over handles): flattened, made contiguous and checked here for every
        entry -- int32 counts in [0, 2^31 - 1], the outside count in its carrier's range; the library checks the size."""
        t = pack_diag(key, *unpack_diag(key, raw))
        L.check(getattr(self.lib, diag_entry(key).set)(self.h, _diag_ptr(t), t.size))

    def diag_parts(self, key):
        """{part: shaped array} of the table ``key`` (:func:`split_diag`), with ``outside`` as an integer where the entry
        carries an outside count; the overflow word of an int64 table is its part ``ovf`` [1]."""
        return split_diag(key, self.diag_raw(key), self.diag_counts())

    def set_diag_parts(self, key, parts):
        """Install the table from its parts (:func:`join_diag`; ``outside`` defaults to 0), checked as :meth:`set_diag_raw`."""
        self.set_diag_raw(key, join_diag(key, parts))

    def export_diag(self, key, device_ptr):
        """Copy the raw table device-to-device to ``device_ptr`` (``diag_words(key)`` elements on this handle's device)."""
        name = "hc_export_" + diag_entry(key).stem
        if name not in L.EXPORTS:
            raise ValueError(f"the table {key!r} has no device-to-device export")
        L.check(getattr(self.lib, name)(self.h, C.c_void_p(int(device_ptr)), self.diag_words(key)))

    def reset_diag(self, key):
        """Zero the table ``key`` -- and, where its family has one reset for all its tables, the others with it."""
        L.check(getattr(self.lib, diag_entry(key).reset)(self.h))

    def _diag_counter(self, name):
        """A trailing count read on its own (``hc_get_*_outside`` / ``hc_get_*_overflow``)."""
        out = C.c_uint64()
        L.check(getattr(self.lib, name)(self.h, C.byref(out)))
        return int(out.value)

    # -- ensemble profile statistics (include/hydrocol.h hc_set_profile_stats) ---------------------------------------
    def set_profile_stats(self, stride):
        """Accumulate psi / theta of every ``stride``-th forcing row and the fluxes of every solved row (0 = off).  Row 0 is
        the state before any solve: call :meth:`profile_snapshot` once the initial states are in place."""
        stride = int(stride)
        if stride < 0:
            raise ValueError(f"profile stride must be >= 0, got {stride}")
        L.check(self.lib.hc_set_profile_stats(self.h, stride))
        self.profile_stride = stride
        self.theta_hist_bins = 0          # keyed to the profile rows: the library turned it off
        self.storage_ranges, self.storage_bins = np.zeros((0, 2), dtype=np.int32), 0      # ... and the layer storage
        self.theta_cov_stride = 0         # ... and the theta covariance
        self.conductivity, self.conductivity_ranges = False, np.zeros((0, 2), dtype=np.int32)     # ... and the conductivities

    def profile_snapshot(self, row=0):
        L.check(self.lib.hc_profile_snapshot(self.h, int(row)))

    def profile_words(self):
        return self.diag_words("profile")

    def profile_table(self):
        """The raw int64 table (layout: :func:`profile_layout`)."""
        return self.diag_raw("profile")

    def set_profile_table(self, table):
        self.set_diag_raw("profile", table)

    def profile_overflow(self):
        return self._diag_counter("hc_get_profile_overflow")

    def profile_stats(self, table=None):
        """Mean / sigma arrays of ``profile_table()`` (or of ``table``, e.g. summed over ranks): :func:`profile_tables_to_stats`."""
        t = self.profile_table() if table is None else table
        return profile_tables_to_stats(t, self.P, self.T, self.D, self.profile_stride,
                                       np.stack([pt.por_node for pt in self.points]), self.cols.dz)

    # -- ensemble water-table histograms (include/hydrocol.h hc_set_wtd_hist) ----------------------------------------
    def set_wtd_hist(self, stride):
        """Count the members' water-table indices of every ``stride``-th forcing row into a [P][n_hrow][D] int32 table
        (0 = off).  Row 0 (the initial state) stays empty: the reference computes no water table for it."""
        stride = int(stride)
        if stride < 0:
            raise ValueError(f"histogram stride must be >= 0, got {stride}")
        L.check(self.lib.hc_set_wtd_hist(self.h, stride))
        self.wtd_hist_stride = stride

    def wtd_hist_table(self):
        """[P][n_hrow][D] int32 (slot j <-> forcing row j stride: :func:`wtd_hist_rows`)."""
        return self.diag_parts("wtd_hist")["hist"]

    def set_wtd_hist_table(self, table):
        self.set_diag_parts("wtd_hist", {"hist": table})

    # -- ensemble soil-moisture histograms (include/hydrocol.h hc_set_theta_hist) ---------------------------------------
    def set_theta_hist(self, bins):
        """Count every member's theta_vol at every node of the profile rows into ``bins`` (32, 64 or 128) equal bins of
        [0, 1] (0 = off); needs :meth:`set_profile_stats`, and comes before :meth:`profile_snapshot` for row 0 to be
        counted."""
        bins = int(bins)
        self.theta_hist_bins = 0
        L.check(self.lib.hc_set_theta_hist(self.h, bins))
        self.theta_hist_bins = bins

    def theta_hist_table(self):
        """[P][n_prow][D][B] int32: members of each point per bin of theta, node and profile row (:func:`theta_hist_of`)."""
        return self.diag_parts("theta_hist")["hist"]

    def set_theta_hist_table(self, table, outside=0):
        """Install a table (a checkpoint's, a sum over handles) and the outside count that goes with it."""
        self.set_diag_parts("theta_hist", {"hist": table, "outside": outside})

    def reset_theta_hist(self):
        self.reset_diag("theta_hist")

    def theta_hist_outside(self):
        """Members' values that fell in no bin (theta NaN, below 0 or above 1) since the table was made."""
        return self._diag_counter("hc_get_theta_hist_outside")

    # -- ensemble soil-water storage by depth layer (include/hydrocol.h hc_set_layer_storage) ---------------------------
    def set_layer_storage(self, ranges, bins=0):
        """Accumulate every member's storage dz sum theta over the node ranges ``ranges`` [L][2] = (i0, i1) (see
        :func:`layer_ranges`) on the profile rows: exact moments, and with ``bins`` (a power of two in 32 .. 1024) the
        histogram of the layer's mean theta.  No ranges = off.  Needs :meth:`set_profile_stats`, and comes before
        :meth:`profile_snapshot` for row 0 to be counted."""
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1, 2))
        if r.size and (r.min() < -INT32_MAX or r.max() > INT32_MAX):
            raise ValueError("layer ranges must be node indices")
        r32 = np.ascontiguousarray(r, dtype=np.int32)
        self.storage_ranges, self.storage_bins = np.zeros((0, 2), dtype=np.int32), 0
        L.check(self.lib.hc_set_layer_storage(self.h, r32.shape[0], L.iptr(r32), int(bins)))
        self.storage_ranges, self.storage_bins = r32, int(bins) if r32.shape[0] else 0

    def layer_storage_layout(self):
        """(ranges [L][2], bins) as the library holds them."""
        n, b = C.c_int32(), C.c_int32()
        r = np.zeros((STORAGE_MAX_LAYERS, 2), dtype=np.int32)
        L.check(self.lib.hc_get_layer_storage_layout(self.h, C.byref(n), C.byref(b), L.iptr(r)))
        return r[:n.value].copy(), int(b.value)

    def layer_storage_words(self):
        return self.diag_words("storage")

    def layer_storage_table(self):
        """The raw int64 moments table (layout: :func:`layer_storage_table_layout`)."""
        return self.diag_raw("storage")

    def set_layer_storage_table(self, table):
        self.set_diag_raw("storage", table)

    def layer_storage_hist_table(self):
        """[P][n_prow][L][B] int32: members of each point per bin of the layer's mean theta and profile row."""
        return self.diag_parts("storage_hist")["hist"]

    def set_layer_storage_hist_table(self, table, outside=0):
        """Install a histogram table (a checkpoint's, a sum over handles) and the outside count that goes with it."""
        self.set_diag_parts("storage_hist", {"hist": table, "outside": outside})

    def reset_layer_storage(self):
        self.reset_diag("storage")

    def layer_storage_outside(self):
        """Members' layer means that fell in no bin (NaN, below 0 or above 1) since the tables were made."""
        return self._diag_counter("hc_get_layer_storage_outside")

    def layer_storage_overflow(self):
        return self._diag_counter("hc_get_layer_storage_overflow")

    def layer_storage_stats(self, table=None):
        """Mean / sigma [cm] of ``layer_storage_table()`` (or of ``table``, e.g. summed over ranks): :func:`layer_storage_stats`."""
        t = self.layer_storage_table() if table is None else table
        return layer_storage_stats(t, self.P, self.T, len(self.storage_ranges), self.profile_stride)

    # -- ensemble conductivity profiles (include/hydrocol.h hc_set_conductivity_stats) ----------------------------------------
    def set_conductivity_stats(self, ranges=(), on=True):
        """Accumulate ln K_hrc and ln K_bkg of every member at every node of the profile rows -- with the noise vector each
        row was solved with -- and, with node ranges ``ranges`` [L][2] = (i0, i1) (see :func:`layer_ranges`), ln of the
        layers' effective vertical conductivity: exact integer moments.  ``on=False`` = off.  Needs
        :meth:`set_profile_stats`, and comes before :meth:`profile_snapshot` for row 0 to be counted.  While it is on, a
        launch ends on every profile row."""
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1, 2))
        if r.size and (r.min() < -INT32_MAX or r.max() > INT32_MAX):
            raise ValueError("layer ranges must be node indices")
        r32 = np.ascontiguousarray(r, dtype=np.int32)
        self.conductivity, self.conductivity_ranges = False, np.zeros((0, 2), dtype=np.int32)
        if not on:
            L.check(self.lib.hc_clear_conductivity_stats(self.h))
            return
        L.check(self.lib.hc_set_conductivity_stats(self.h, r32.shape[0], L.iptr(r32)))
        self.conductivity, self.conductivity_ranges = True, r32

    def conductivity_layout(self):
        """(on, ranges [L][2]) as the library holds them."""
        on, n = C.c_int32(), C.c_int32()
        r = np.zeros((STORAGE_MAX_LAYERS, 2), dtype=np.int32)
        L.check(self.lib.hc_get_conductivity_stats_layout(self.h, C.byref(on), C.byref(n), L.iptr(r)))
        return bool(on.value), r[:n.value].copy()

    def conductivity_table(self):
        """The raw int64 table (layout: :func:`conductivity_table_layout`)."""
        return self.diag_raw("conductivity")

    def set_conductivity_table(self, table):
        self.set_diag_raw("conductivity", table)

    def reset_conductivity_stats(self):
        self.reset_diag("conductivity")

    def conductivity_overflow(self):
        return self._diag_counter("hc_get_conductivity_stats_overflow")

    def conductivity_stats(self, table=None):
        """Mean / sigma of ln K and the geometric-mean K of ``conductivity_table()`` (or of ``table``, e.g. summed over
        ranks): :func:`conductivity_stats`."""
        t = self.conductivity_table() if table is None else table
        return conductivity_stats(t, self.P, self.T, self.D, len(self.conductivity_ranges), self.profile_stride)

    def conductivity_eval(self, row):
        """[4][N][D] = K_hrc, K_bkg, ln K_hrc, ln K_bkg of the members' current states with the noise vector of forcing row
        ``row`` and no failed attempt (``hc_conductivity_eval``: the table's own device code)."""
        out = np.zeros((4, self.N, self.D))
        L.check(self.lib.hc_conductivity_eval(self.h, int(row), L.dptr(out)))
        return out

    # -- ensemble covariance of theta(z) and the water table (include/hydrocol.h hc_set_theta_cov) -------------------------
    def set_theta_cov(self, node_stride):
        """Accumulate the second moments of every member's theta_vol at the nodes 0, s, 2 s, ... and of its water-table
        index on the profile rows, in exact integers (0 = off); needs :meth:`set_profile_stats`, and comes before
        :meth:`profile_snapshot` for row 0 to be counted."""
        s = int(node_stride)
        if not -INT32_MAX <= s <= INT32_MAX:
            raise ValueError("the node stride must be a node count")
        self.theta_cov_stride = 0
        L.check(self.lib.hc_set_theta_cov(self.h, s))
        self.theta_cov_stride = s

    def theta_cov_layout(self):
        """(node stride, selected nodes n, words per row W) as the library holds them; zeros when off."""
        s, n, w = C.c_int32(), C.c_int32(), C.c_int64()
        L.check(self.lib.hc_get_theta_cov_layout(self.h, C.byref(s), C.byref(n), C.byref(w)))
        return int(s.value), int(n.value), int(w.value)

    def theta_cov_words(self):
        return self.diag_words("theta_cov")

    def theta_cov_table(self):
        """[P][n_prow][W] int64: count, S1 [E], S2 packed (:func:`theta_cov_of`) per point and profile row."""
        return self.diag_parts("theta_cov")["cov"]

    def set_theta_cov_table(self, table, outside=0):
        """Install a table (a checkpoint's, a sum over handles) and the outside count that goes with it."""
        self.set_diag_parts("theta_cov", {"cov": table, "outside": outside})

    def reset_theta_cov(self):
        self.reset_diag("theta_cov")

    def theta_cov_outside(self):
        """Members that were not counted (a selected theta NaN, below 0 or above 1) since the table was made."""
        return self._diag_counter("hc_get_theta_cov_outside")

    # -- period totals per member (include/hydrocol.h hc_set_period_totals) ---------------------------------------------
    def set_period_totals(self, ends, threshold_nodes=(), bins=0, flux_max_log2=(0, 0)):
        """Accumulate per member, over the periods that end on the forcing rows ``ends`` (ascending, inclusive; see
        :func:`period_ends`), the transpiration and lateral-flow totals, the shallowest and deepest water-table index
        and the rows with the water table at or above each of ``threshold_nodes`` (at most 4); reduce them over the
        members of each point at every end row: exact moments and, with ``bins`` (a power of two in 32 .. 1024),
        histograms of the flux totals over [0, 2^e) cm, e = ``flux_max_log2`` (transpiration, lateral flow), and of both
        extremes.  No ends = off."""
        e = np.ascontiguousarray(np.asarray(ends, dtype=np.int64).reshape(-1))
        t = np.asarray(threshold_nodes, dtype=np.int64).reshape(-1)
        f = np.asarray(flux_max_log2, dtype=np.int64).reshape(-1)
        if f.size != 2:
            raise ValueError("flux_max_log2 is (transpiration, lateral flow)")
        if (t.size and np.abs(t).max() > INT32_MAX) or np.abs(f).max() > INT32_MAX or e.size > INT32_MAX:
            raise ValueError("threshold nodes are node indices, flux_max_log2 exponents in -8 .. 12")
        t32, f32 = np.ascontiguousarray(t, dtype=np.int32), np.ascontiguousarray(f, dtype=np.int32)
        self.period_ends, self.period_threshold_nodes = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32)
        self.period_bins, self.period_flux_max_log2 = 0, (0, 0)
        try:
            L.check(self.lib.hc_set_period_totals(self.h, e.size, L.lptr(e), t32.size, L.iptr(t32), int(bins), L.iptr(f32)))
        finally:
            self._sync_root_uptake()     # other ends turn the root uptake off
        if e.size:
            self.period_ends, self.period_threshold_nodes = e, t32
            self.period_bins, self.period_flux_max_log2 = int(bins), ((int(f[0]), int(f[1])) if bins else (0, 0))

    def period_totals_layout(self):
        """(ends, threshold_nodes, bins, flux_max_log2) as the library holds them."""
        n, k, b = C.c_int32(), C.c_int32(), C.c_int32()
        thr, fx = np.zeros(PERIOD_MAX_THRESHOLDS, dtype=np.int32), np.zeros(2, dtype=np.int32)
        L.check(self.lib.hc_get_period_totals_layout(self.h, C.byref(n), C.byref(k), C.byref(b), L.iptr(thr), L.iptr(fx), None, 0))
        ends = np.zeros(n.value, dtype=np.int64)
        L.check(self.lib.hc_get_period_totals_layout(self.h, C.byref(n), C.byref(k), C.byref(b), L.iptr(thr), L.iptr(fx),
                                                     L.lptr(ends), ends.size))
        return ends, thr[:k.value].copy(), int(b.value), (int(fx[0]), int(fx[1]))

    @property
    def period_k(self):
        return 4 + len(self.period_threshold_nodes)

    def period_totals_words(self):
        return self.diag_words("period")

    def period_totals_table(self):
        """The raw int64 moments table (layout: :func:`period_totals_table_layout`)."""
        return self.diag_raw("period")

    def set_period_totals_table(self, table):
        self.set_diag_raw("period", table)

    def period_totals_hist_raw(self):
        """The raw int32 histogram table: phist_flux, phist_wtd, then the outside count in two entries."""
        return self.diag_raw("period_hist")

    def period_totals_hists(self):
        """(phist_flux [P][n_period][2][B], phist_wtd [P][n_period][2][D]) int32: members of each point per bin."""
        parts = self.diag_parts("period_hist")
        return parts["flux"], parts["wtd"]

    def set_period_totals_hists(self, hist_flux, hist_wtd, outside=0):
        """Install both histograms (a checkpoint's, a sum over handles) and the outside count that goes with them."""
        self.set_diag_parts("period_hist", {"flux": hist_flux, "wtd": hist_wtd, "outside": outside})

    def period_totals_acc(self):
        """The members' accumulators [K][N] int64 as they stand (the running period's; reset values after an end row)."""
        return self.diag_parts("period_acc")["acc"]

    def set_period_totals_acc(self, acc):
        self.set_diag_parts("period_acc", {"acc": acc})

    def reset_period_totals(self):
        self.reset_diag("period")

    def period_totals_outside(self):
        """Members' values that fell in no bin of their histogram since the tables were made."""
        return self._diag_counter("hc_get_period_totals_outside")

    def period_totals_overflow(self):
        return self._diag_counter("hc_get_period_totals_overflow")

    def period_totals_stats(self, table=None):
        """The science arrays of ``period_totals_table()`` (or of ``table``, e.g. summed over ranks):
        :func:`period_totals_stats`."""
        t = self.period_totals_table() if table is None else table
        return period_totals_stats(t, self.P, self.period_ends, len(self.period_threshold_nodes), float(self.cols.z[0]),
                                   float(self.params.dz), self.forcing.wtd_obs)

    # -- root-water uptake by depth (include/hydrocol.h hc_set_root_uptake) ---------------------------------------------
    def set_root_uptake(self, cells, bins=0):
        """Accumulate per member, over the periods of :meth:`set_period_totals` (which comes first), the root-water
        uptake of every solved daylight row in total and in the layers ``cells`` = [(lo, hi), ...] (ranges of midpoint
        cells, see :func:`layer_cells`; at most 8), and per period the uptake at every midpoint; reduce the totals over
        the members of each point at every end row: exact moments and, with ``bins`` (a power of two in 32 .. 1024),
        histograms of each layer's share of a member's total.  No layers = off."""
        r = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
        if r.size and np.abs(r).max() > INT32_MAX:
            raise ValueError("uptake layers are ranges of midpoint cells")
        lo, hi = (np.ascontiguousarray(r[:, k], dtype=np.int32) for k in (0, 1))
        self.uptake_cells, self.uptake_bins = np.zeros((0, 2), dtype=np.int32), 0
        L.check(self.lib.hc_set_root_uptake(self.h, r.shape[0], L.iptr(lo), L.iptr(hi), int(bins)))
        if r.shape[0]:
            self.uptake_cells, self.uptake_bins = r.astype(np.int32), int(bins)

    def root_uptake_layout(self):
        """(cells [L][2], bins) as the library holds them."""
        n, b = C.c_int32(), C.c_int32()
        lo, hi = np.zeros(UPTAKE_MAX_LAYERS, dtype=np.int32), np.zeros(UPTAKE_MAX_LAYERS, dtype=np.int32)
        L.check(self.lib.hc_get_root_uptake_layout(self.h, C.byref(n), C.byref(b), L.iptr(lo), L.iptr(hi)))
        return np.stack([lo[:n.value], hi[:n.value]], axis=1), int(b.value)

    def _sync_root_uptake(self):
        self.uptake_cells, self.uptake_bins = self.root_uptake_layout()

    def root_uptake_words(self):
        return self.diag_words("uptake")

    def root_uptake_table(self):
        """The raw int64 table (layout: :func:`root_uptake_table_layout`)."""
        return self.diag_raw("uptake")

    def set_root_uptake_table(self, table):
        self.set_diag_raw("uptake", table)

    def root_uptake_hist_raw(self):
        """The raw int32 share histograms with the outside count in their two last entries."""
        return self.diag_raw("uptake_hist")

    def root_uptake_hist(self):
        """[P][n_period][L][B] int32: members of each point per bin of the layer's share of their total."""
        return self.diag_parts("uptake_hist")["hist"]

    def set_root_uptake_hist(self, hist, outside=0):
        """Install the share histograms (a checkpoint's, a sum over handles) and the outside count that goes with them."""
        self.set_diag_parts("uptake_hist", {"hist": hist, "outside": outside})

    def root_uptake_acc(self):
        """The members' accumulators [L + 1][N] int64 as they stand (the running period's; 0 after an end row)."""
        return self.diag_parts("uptake_acc")["acc"]

    def set_root_uptake_acc(self, acc):
        self.set_diag_parts("uptake_acc", {"acc": acc})

    def reset_root_uptake(self):
        self.reset_diag("uptake")

    def root_uptake_outside(self):
        """Members with a zero period total, which no share histogram holds (0 without bins)."""
        return self._diag_counter("hc_get_root_uptake_outside")

    def root_uptake_overflow(self):
        return self._diag_counter("hc_get_root_uptake_overflow")

    def root_uptake_eval(self, row):
        """(theta_mid, u), [N][D - 1] each: theta at the midpoints of the members' current states and the uptake the RHS
        applies there on forcing row ``row``, from the device code the tables are built with (test hook)."""
        th, u = np.zeros((self.N, self.D - 1)), np.zeros((self.N, self.D - 1))
        L.check(self.lib.hc_root_uptake_eval(self.h, int(row), L.dptr(th), L.dptr(u)))
        return th, u

    def root_uptake_tables(self, point=0):
        """The five midpoint tables [5][D - 1] of a point as the device holds them (:func:`root_uptake_mid_tables`)."""
        return root_uptake_mid_tables(self.points[point])

    def root_uptake_stats(self, table=None):
        """The science arrays of ``root_uptake_table()`` (or of ``table``, e.g. summed over ranks):
        :func:`root_uptake_stats`; with ``root_uptake_profile``'s arrays."""
        t = self.root_uptake_table() if table is None else table
        out = root_uptake_stats(t, self.P, self.period_ends, len(self.uptake_cells), self.D)
        out.update(root_uptake_profile(t, self.P, self.period_ends, len(self.uptake_cells), self.D, self.cols.z))
        return out

    # -- particle filter on the well's water table (include/hydrocol.h hc_set_filter) ----------------------------------
    def set_filter(self, stride, sigma_cm=None, seed=0):
        """Resample the members on every ``stride``-th forcing row that has an observation (0 = off): weights from the
        Gaussian likelihood of the observed water table (``sigma_cm``), systematic resampling per parameter point.  The
        tables accumulate the forecast; the states after the call are the analysis.  In a Philox run this fills the base
        noise vectors: call it after any spin-up and noise-scale restore."""
        stride = int(stride)
        if stride < 0:
            raise ValueError(f"filter stride must be >= 0, got {stride}")
        sigma = float(sigma_cm) if stride else 0.0
        if stride and not (np.isfinite(sigma) and sigma > 0.0):
            raise ValueError(f"filter sigma_cm = {sigma_cm!r} must be finite and > 0")
        self.filter_stride, self.filter_sigma_cm, self.filter_seed = 0, 0.0, 0   # hc_set_filter turns it off first,
        #                                                                            and leaves it off if it refuses
        self.filter_shard, self._filter_shard_keep = None, None                  # ... and the sharding with it
        self.filter_sm_nodes = None                                              # ... and the sensor record
        self.filter_ess_floor = 0.0                                              # ... and the tempering
        self.filter_rejuvenation = 0.0                                           # ... and the rejuvenation
        self.filter_window_offsets = ()                                          # ... and the window
        self.filter_smoother = (0, 0)                                            # ... and the smoother
        L.check(self.lib.hc_set_filter(self.h, stride, sigma, int(seed) & 0xFFFFFFFFFFFFFFFF))
        self.filter_stride, self.filter_sigma_cm, self.filter_seed = stride, sigma, int(seed)

    def _filter_off(self):
        """The library turned the filters off (a new noise source or new point keys, include/hydrocol.h): so does this side."""
        self.filter_stride, self.filter_sigma_cm, self.filter_seed = 0, 0.0, 0
        self.filter_sm_nodes = None
        self.filter_ess_floor = 0.0
        self.filter_rejuvenation = 0.0
        self.filter_window_offsets = ()
        self.filter_smoother = (0, 0)
        self.enkf_stride, self.enkf_sigma_cm, self.enkf_localisation_cm, self.enkf_seed = 0, 0.0, 0.0, 0
        self.enkf_sm_nodes = None
        self.enkf_method, self.enkf_relaxation = "stochastic", 0.0
        self.enkf_window_offsets = ()
        self.enkf_shard = None
        self.enkf_noise_field, self.enkf_noise_relaxation = False, 0.0
        self.enkf_forcing, self.enkf_forcing_relaxation = False, 0.0
        self.filter_shard, self._filter_shard_keep = None, None
        self.noise_corr = None                                                   # ... and the noise correlation

    # -- the assimilation tables: one path for the nine of them (ASSIM_TABLES below) -------------------------------------
    def assim_table(self, key):
        """[P][n_arow] + the key's trailing shape (:func:`assim_table_shape`) float64, n_arow the slots of the owner's
        stride: ``hc_get_<key>_stats``.  The named accessors below document the columns."""
        owner = ASSIM_TABLES[key][0]
        trailing = assim_table_shape(key, self.D, getattr(self, owner + "_sm_n"), getattr(self, owner + "_window_n"))
        t = np.zeros((self.P, stride_rows(self.T, getattr(self, owner + "_stride"))) + trailing)
        L.check(getattr(self.lib, f"hc_get_{key}_stats")(self.h, L.dptr(t), t.size))
        return t

    def set_assim_table(self, key, table):
        """``hc_set_<key>_stats``: the table :meth:`assim_table` gave, in any shape (a checkpoint's)."""
        t = L.as_f64(table).reshape(-1)
        L.check(getattr(self.lib, f"hc_set_{key}_stats")(self.h, L.dptr(t), t.size))

    def filter_table(self):
        """[P][n_arow][4] float64: count, ESS, log-likelihood increment, survivors per assimilation slot (slot j <-> row
        j stride; count 0 and NaN where nothing was assimilated)."""
        return self.assim_table("filter")

    def set_filter_table(self, table):
        self.set_assim_table("filter", table)

    def filter_base(self):
        """[N][D] base noise vectors of a filtered Philox run (what resampling carries from ancestor to slot)."""
        out = np.empty((self.N, self.D))
        L.check(self.lib.hc_get_filter_base(self.h, L.dptr(out), 0, self.N))
        return out

    def set_filter_base(self, base):
        base = L.as_f64(base)
        if base.shape != (self.N, self.D):
            raise ValueError(f"base noise must be [{self.N}, {self.D}]")
        L.check(self.lib.hc_set_filter_base(self.h, L.dptr(base)))

    def filter_ancestors(self):
        """[N] int64: the handle-local member each slot took its state from at the last assimilation (test hook); with
        :meth:`set_filter_shard` the global member id."""
        out = np.zeros(self.N, dtype=np.int64)
        L.check(self.lib.hc_get_filter_ancestors(self.h, L.lptr(out)))
        return out

    def filter_weights(self):
        """[P][D] int64: q_b of the last assimilation (test hook)."""
        out = np.zeros((self.P, self.D), dtype=np.int64)
        L.check(self.lib.hc_get_filter_weights(self.h, L.lptr(out)))
        return out

    def filter_draw(self):
        """[P] int64: the systematic offset r of the last assimilation (test hook)."""
        out = np.zeros(self.P, dtype=np.int64)
        L.check(self.lib.hc_get_filter_draw(self.h, L.lptr(out)))
        return out

    # -- tempered weights (include/hydrocol.h hc_set_filter_tempering) ---------------------------------------------------
    def set_filter_tempering(self, ess_floor):
        """Hold the effective sample size of every resampling above ``ess_floor`` (a fraction of the counted members,
        0 < f < 1; 0 = off): the weights are raised to the largest exponent beta = k / 1024 of a bisection that keeps it
        there.  The filter's table keeps scoring the forecast with the stated error.  The filter must be on
        (:meth:`set_filter` first; it removes the tempering again)."""
        f = float(ess_floor)
        if f != 0.0 and not (np.isfinite(f) and 0.0 < f < 1.0):
            raise ValueError(f"filter ess_floor = {ess_floor!r} must be 0 (off) or finite with 0 < f < 1")
        self.filter_ess_floor = 0.0
        L.check(self.lib.hc_set_filter_tempering(self.h, f))
        self.filter_ess_floor = f

    def filter_temper_table(self):
        """[P][n_arow][4] float64: beta, the ESS at beta, the target T and the trials evaluated per assimilation slot (NaN
        where nothing was assimilated or no member was counted)."""
        return self.assim_table("filter_temper")

    def set_filter_temper_table(self, table):
        self.set_assim_table("filter_temper", table)

    def filter_temper_trials(self):
        """[P][11][4] int64: {k, Q_k, S_k low word, S_k high word} of the last assimilation's trials in trial order,
        unused rows k = -1 (test hook)."""
        out = np.zeros((self.P, TEMPER_TRIALS, TEMPER_WIDTH), dtype=np.int64)
        L.check(self.lib.hc_get_filter_temper_trials(self.h, L.lptr(out)))
        return out

    # -- rejuvenated base vectors (include/hydrocol.h hc_set_filter_rejuvenation) -----------------------------------------
    def set_filter_rejuvenation(self, discount):
        """After every resampling that copied a member (0 < survivors < N_p) pull the point's base noise vectors towards
        their mean and jitter them (Liu & West's kernel shrinkage with ``discount`` delta, 0.5 <= delta < 1; 0 = off), so
        that the per-node mean and variance stay what the resampling left and no two members share a field.  The filter
        must be on and not sharded (:meth:`set_filter` first; it removes the setting again)."""
        d = rejuvenation_discount(discount)
        if d and self.filter_shard is not None:
            raise ValueError("filter rejuvenation with a sharded filter: the gathered words are water-table indices, the "
                             "moments of the base vectors would need an exchange of their own")
        self.filter_rejuvenation = 0.0
        L.check(self.lib.hc_set_filter_rejuvenation(self.h, d))
        self.filter_rejuvenation = d

    def filter_rejuvenation_shrinkage(self):
        """(delta, a) as the library holds them; (0, 0) when off."""
        d, a = np.zeros(1), np.zeros(1)
        L.check(self.lib.hc_get_filter_rejuvenation(self.h, L.dptr(d), L.dptr(a)))
        return float(d[0]), float(a[0])

    def filter_rejuvenation_table(self):
        """[P][n_arow][4] float64: applied, members refused, sqrt(mean_d s_d^2) of the resampled base vectors and of the
        rejuvenated ones per assimilation slot (the last two NaN when not applied; all NaN where nothing was assimilated)."""
        return self.assim_table("filter_rejuvenation")

    def set_filter_rejuvenation_table(self, table):
        self.set_assim_table("filter_rejuvenation", table)

    def filter_rejuvenation_moments(self):
        """[P][3][D] float64 of the last assimilation: mean_d and s_d of the resampled base vectors, s_d of the vectors the
        move left (test hook)."""
        out = np.zeros((self.P, 3, self.D))
        L.check(self.lib.hc_get_filter_rejuvenation_moments(self.h, L.dptr(out)))
        return out

    def filter_rejuvenation_normals(self, row, first=0, count=None):
        """[count][D] float64: the jitter's standard normals of the handle's slots ``first`` ... at forcing row ``row``
        (stateless test hook; the filter on)."""
        count = self.N - int(first) if count is None else int(count)
        out = np.zeros((count, self.D))
        L.check(self.lib.hc_filter_rejuvenation_normals(self.h, int(row), int(first), count, L.dptr(out)))
        return out

    # -- soil-moisture sensors in the particle filter (include/hydrocol.h hc_set_filter_soil_moisture) -------------------
    def _sm_record(self, nodes, values, sigma):
        """(nodes int32 [n], values [T][n], sigma [n]) of a soil-moisture record as the library takes it; n = 0: none."""
        nodes = np.ascontiguousarray([] if nodes is None else nodes, dtype=np.int32).reshape(-1)
        n = int(nodes.size)
        if n == 0:
            return nodes, None, None
        v = L.as_f64(values).reshape(self.T, n) if np.size(values) == self.T * n else None
        if v is None:
            raise ValueError(f"soil-moisture values must hold [{self.T}][{n}] entries, got {np.shape(values)}")
        return nodes, v, L.as_f64(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (n,)).copy())

    def set_filter_soil_moisture(self, nodes, values=None, sigma=None):
        """Add a record of volumetric water content at the depth nodes ``nodes`` (at most 8) to the particle filter's
        weights, which then belong to a member and not to a bin: ``values`` [T][n] in [0, 1], NaN = no observation on that
        row; ``sigma`` the sensors' error (m^3/m^3), one number or one per sensor.  ``nodes`` empty or None removes the
        record.  The filter must be on (:meth:`set_filter` first; it removes the record again) and not sharded."""
        nodes, v, sg = self._sm_record(nodes, values, sigma)
        self.filter_sm_nodes = None
        if nodes.size == 0:
            L.check(self.lib.hc_set_filter_soil_moisture(self.h, 0, None, None, None))
            return
        L.check(self.lib.hc_set_filter_soil_moisture(self.h, int(nodes.size), L.iptr(nodes), L.dptr(v), L.dptr(sg)))
        self.filter_sm_nodes = nodes.copy()

    @property
    def filter_sm_n(self):
        return 0 if self.filter_sm_nodes is None else int(self.filter_sm_nodes.size)

    def filter_sm_table(self):
        """[P][n_arow][n][6] float64 per assimilation slot and sensor: observed (0/1), observation, forecast mean and std
        of theta, posterior mean and std of theta over the resampled slots; NaN where the slot had no sensor value (and
        after observed = 0)."""
        return self.assim_table("filter_sm")

    def set_filter_sm_table(self, table):
        self.set_assim_table("filter_sm", table)

    def filter_sm_width(self):
        """m_s = the sensors present on the last assimilation (0: it took the bin path; test hook)."""
        w = np.zeros(1, dtype=np.int32)
        L.check(self.lib.hc_get_filter_sm_width(self.h, L.iptr(w)))
        return int(w[0])

    def filter_member_weights(self):
        """[N] int64: q_m of the last assimilation, with a record set (after a bin-path row q of the member's bin; test
        hook)."""
        out = np.zeros(self.N, dtype=np.int64)
        L.check(self.lib.hc_get_filter_member_weights(self.h, L.lptr(out)))
        return out

    def filter_loglik(self):
        """[N] l_m of the last assimilation, a sensor row (test hook)."""
        out = np.zeros(self.N)
        L.check(self.lib.hc_get_filter_loglik(self.h, L.dptr(out)))
        return out

    def filter_sm_theta(self):
        """[N][m_s] theta of every member's forecast at the nodes of the sensors present on the last assimilation (test
        hook)."""
        out = np.zeros((self.N, self.filter_sm_width()))
        L.check(self.lib.hc_get_filter_sm_theta(self.h, L.dptr(out)))
        return out

    # -- the well's record inside the window, particle filter (include/hydrocol.h hc_set_filter_window) ------------------
    def set_filter_window(self, offsets=()):
        """Every member's water-table index on the rows ``offsets`` before an assimilation row (integers in [1, stride),
        distinct, at most 8 together with the sensors) is recorded when the row is solved and joins that row's weight as a
        further well-type term: the weight is then the likelihood of everything the member's trajectory passed since the
        last resampling.  Empty or None turns it off.  The filter must be on (:meth:`set_filter` first; it turns the
        window off again) and not sharded."""
        off = filter_window_settings(offsets, self.filter_stride, self.filter_sm_n)
        self.filter_window_offsets = ()
        a = np.ascontiguousarray(off, dtype=np.int32)
        L.check(self.lib.hc_set_filter_window(self.h, a.size, L.iptr(a) if a.size else None))
        self.filter_window_offsets = off

    @property
    def filter_window_n(self):
        return len(self.filter_window_offsets)

    def filter_window_table(self):
        """[P][n_arow][n][4] float64 per assimilation slot and offset: observed (0/1), observation, forecast mean and std
        of the members' water-table depth on the lagged row (cm from the top node); NaN where the slot's assimilation had
        no lagged row (and after observed = 0)."""
        return self.assim_table("filter_window")

    def set_filter_window_table(self, table):
        self.set_assim_table("filter_window", table)

    def filter_window_capture(self):
        """(b [n][N] int32, rows [n] int64): the water-table indices the window holds for the coming assimilation (row
        -1: nothing; checkpoints)."""
        b = np.zeros((self.filter_window_n, self.N), dtype=np.int32)
        rows = np.zeros(self.filter_window_n, dtype=np.int64)
        L.check(self.lib.hc_get_filter_window_capture(self.h, L.iptr(b), L.lptr(rows)))
        return b, rows

    def set_filter_window_capture(self, b, rows):
        b = np.ascontiguousarray(b, dtype=np.int32)
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        if b.shape != (self.filter_window_n, self.N) or rows.size != self.filter_window_n:
            raise ValueError(f"the window's capture must be [{self.filter_window_n}, {self.N}] with as many rows")
        L.check(self.lib.hc_set_filter_window_capture(self.h, L.iptr(b), L.lptr(rows)))

    def filter_window_slots(self):
        """The indices into ``filter_window_offsets`` of the last assimilation's lagged columns, in column order (test
        hook)."""
        w, slots = np.zeros(1, dtype=np.int32), np.zeros(SM_MAX_SENSORS, dtype=np.int32)
        L.check(self.lib.hc_get_filter_window_width(self.h, L.iptr(w), L.iptr(slots)))
        return slots[:int(w[0])].copy()

    # -- fixed-lag smoother of the water table by ancestry (include/hydrocol.h hc_set_filter_smoother) -------------------
    def set_filter_smoother(self, stride, lag=0):
        """Carry every slot's water-table index of each ``stride``-th forcing row (the record rows) through the filter's
        resamplings and count it ``lag`` record rows later (0 <= lag <= 64): the distribution of that row given the
        observations up to the later one -- the one table that describes the posterior.  ``stride`` 0 turns it off.  The
        filter must be on (:meth:`set_filter` first; it removes the smoother again) and not sharded."""
        stride, lag = filter_smoother_settings(stride, lag)
        self.filter_smoother = (0, 0)
        L.check(self.lib.hc_set_filter_smoother(self.h, stride, lag))
        self.filter_smoother = (stride, lag)

    def filter_smoother_layout(self):
        """(stride, lag, n_srow) as the library holds them; zeros: off."""
        s, k, n = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
        L.check(self.lib.hc_get_filter_smoother_layout(self.h, L.iptr(s), L.iptr(k), L.lptr(n)))
        return int(s[0]), int(k[0]), int(n[0])

    def _smoother_rows(self):
        """n_srow (off: 1, and the library refuses the call)"""
        return stride_rows(self.T, self.filter_smoother[0]) if self.filter_smoother[0] else 1

    def filter_smoother_hist(self):
        """[P][n_srow][D] int32: the smoothed histograms (slot j <-> forcing row j stride; empty until emitted)."""
        t = np.zeros((self.P, self._smoother_rows(), self.D), dtype=np.int32)
        L.check(self.lib.hc_get_filter_smoother_hist(self.h, L.iptr(t), t.size))
        return t

    def set_filter_smoother_hist(self, table):
        t = np.asarray(table)
        if t.size and (t.min() < 0 or t.max() > INT32_MAX):
            raise ValueError("histogram counts must lie in [0, 2^31 - 1]")
        t = np.ascontiguousarray(t, dtype=np.int32).reshape(-1)
        L.check(self.lib.hc_set_filter_smoother_hist_table(self.h, L.iptr(t), t.size))

    def filter_smoother_paths(self):
        """[P][n_srow][2] int64: (distinct paths behind the slot's histogram, the row it is conditioned on); (0, -1) until
        emitted."""
        t = np.zeros((self.P, self._smoother_rows(), 2), dtype=np.int64)
        L.check(self.lib.hc_get_filter_smoother_paths(self.h, L.lptr(t), t.size))
        return t

    def set_filter_smoother_paths(self, table):
        t = np.ascontiguousarray(table, dtype=np.int64).reshape(-1)
        L.check(self.lib.hc_set_filter_smoother_paths(self.h, L.lptr(t), t.size))

    def filter_smoother_ring(self):
        """(w [K + 1][N] int32, id [K + 1][N] int64, rows [K + 1] int64, last row stepped): what the ring holds for the
        coming emissions (row -1: nothing, the plane reads 0; checkpoints)."""
        K1 = self.filter_smoother[1] + 1
        w, ids = np.zeros((K1, self.N), dtype=np.int32), np.zeros((K1, self.N), dtype=np.int64)
        rows, last = np.zeros(K1, dtype=np.int64), np.zeros(1, dtype=np.int64)
        L.check(self.lib.hc_get_filter_smoother_ring(self.h, L.iptr(w), L.lptr(ids), L.lptr(rows), L.lptr(last)))
        return w, ids, rows, int(last[0])

    def set_filter_smoother_ring(self, w, ids, rows, last_row=-1):
        K1 = self.filter_smoother[1] + 1
        w = np.ascontiguousarray(w, dtype=np.int32)
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        if w.shape != (K1, self.N) or ids.shape != (K1, self.N) or rows.size != K1:
            raise ValueError(f"the smoother's ring must be [{K1}, {self.N}] twice with as many rows")
        L.check(self.lib.hc_set_filter_smoother_ring(self.h, L.iptr(w), L.lptr(ids), L.lptr(rows), int(last_row)))

    def filter_smoother_flush(self):
        """Emit every pending plane, conditioned on the last row stepped (the end of a run)."""
        L.check(self.lib.hc_filter_smoother_flush(self.h))

    def reset_filter_smoother(self):
        L.check(self.lib.hc_reset_filter_smoother(self.h))

    # -- one point's members on several handles, particle filter (include/hydrocol.h hc_set_filter_shard) ----------------
    def filter_shard_words(self, bounds, index):
        """8-byte words the shard's buffer must hold: the index vector, the send and the receive region."""
        b = np.ascontiguousarray(bounds, dtype=np.int64)
        n = np.zeros(1, dtype=np.int64)
        L.check(self.lib.hc_get_filter_shard_words(self.h, b.size - 1, L.lptr(b), int(index), L.lptr(n)))
        return int(n[0])

    def set_filter_shard(self, bounds, index=0, exchange=None):
        """This handle is shard ``index`` of a point whose members are split at ``bounds`` (``[0, b_1, ..., n_global]``):
        the handles' assimilations together become the whole ensemble's, to the bit.  Per assimilation the library calls
        ``exchange(block, first_word, count_words)`` -- ``block`` a float64 device tensor of n_global words holding 8-byte
        integers, of which [first_word, first_word + count_words) are this handle's; on return everyone else's must be in
        place -- and then ``exchange.route(send, send_words, recv, recv_words)``: ``send`` holds the blocks for the other
        shards one after the other, ``send_words[s]`` words for shard s, and on return ``recv`` must hold the blocks from
        them, ``recv_words[s]`` words from shard s (:class:`multigpu.ShardExchange`; None: nothing to exchange, for a
        handle that holds every member).  The words are bit patterns: copy them, nothing else.  An exception either call
        raises fails the step.  ``bounds`` = None turns sharding off.  The particle filter comes first.  torch must have
        been imported before this process made its first handle (``_lib.load``)."""
        self._filter_shard_keep = None
        if bounds is None:
            L.check(self.lib.hc_set_filter_shard(self.h, 0, None, 0, None, 0, L.EXCHANGE_FN(), L.ROUTE_FN(), None))
            self.filter_shard = None
            return
        b = np.ascontiguousarray(bounds, dtype=np.int64).reshape(-1)
        n_shards, index = b.size - 1, int(index)
        L.load(with_torch=True)                    # the buffer is torch's: one HIP runtime must serve both
        import torch
        self.filter_shard = None
        buf = torch.zeros(max(self.filter_shard_words(b, index), 1), dtype=torch.float64,
                          device=torch.device("cuda", self.device))
        base = buf.data_ptr()

        def view(ptr, n_words):
            at = (int(ptr) - base) // 8
            return buf[at:at + n_words]

        def gather(_ctx, ptr, n_words, first_word, count_words):
            try:                                   # nothing may propagate through the C frames
                if exchange is not None:
                    exchange(view(ptr, n_words), int(first_word), int(count_words))
                return 0
            except BaseException as e:  # noqa: BLE001
                self._shard_error = e
                return 1

        def route(_ctx, send, send_words, recv, recv_words):
            try:
                if exchange is not None:
                    out, back = [int(send_words[s]) for s in range(n_shards)], [int(recv_words[s]) for s in range(n_shards)]
                    exchange.route(view(send, sum(out)), out, view(recv, sum(back)), back)
                return 0
            except BaseException as e:  # noqa: BLE001
                self._shard_error = e
                return 1

        fns = (L.EXCHANGE_FN(gather), L.ROUTE_FN(route))
        L.check(self.lib.hc_set_filter_shard(self.h, n_shards, L.lptr(b), index, C.c_void_p(base), buf.numel(), fns[0],
                                             fns[1], None))
        self._filter_shard_keep = (buf, fns, gather, route)        # alive as long as the handle may call them
        self.filter_shard = (tuple(int(v) for v in b), index)

    def get_filter_shard(self):
        """(n_shards, index, n_global) as the library holds them; (0, 0, 0): off."""
        n, i, g = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
        L.check(self.lib.hc_get_filter_shard(self.h, L.iptr(n), L.iptr(i), L.lptr(g)))
        return int(n[0]), int(i[0]), int(g[0])

    # -- ensemble Kalman filter on the well's water table (include/hydrocol.h hc_set_enkf) ------------------------------
    def set_enkf(self, stride, sigma_cm=None, localisation_cm=0.0, seed=0):
        """Update the members on every ``stride``-th forcing row that has an observation (0 = off): a stochastic EnKF on
        the continuous water table y (``sigma_cm``: the observation error; ``localisation_cm``: the Gaspari-Cohn half-width
        L, 0 = none).  The tables accumulate the forecast; the states after the call are the analysis.  Refused while the
        particle filter is on."""
        stride = int(stride)
        if stride < 0:
            raise ValueError(f"EnKF stride must be >= 0, got {stride}")
        sigma = float(sigma_cm) if stride else 0.0
        loc = float(localisation_cm) if stride else 0.0
        if stride and not (np.isfinite(sigma) and sigma > 0.0):
            raise ValueError(f"EnKF sigma_cm = {sigma_cm!r} must be finite and > 0")
        if stride and not (np.isfinite(loc) and loc >= 0.0):
            raise ValueError(f"EnKF localisation_cm = {localisation_cm!r} must be finite and >= 0")
        if stride and self.filter_stride:
            raise ValueError("the particle filter is on: the EnKF and the filter exclude each other")
        self.enkf_stride, self.enkf_sigma_cm, self.enkf_localisation_cm, self.enkf_seed = 0, 0.0, 0.0, 0
        self.enkf_sm_nodes = None                             # hc_set_enkf removes the sensor record
        self.enkf_method, self.enkf_relaxation = "stochastic", 0.0       # ... and resets the analysis scheme
        self.enkf_window_offsets = ()                         # ... and turns the window off
        self.enkf_shard = None                                # ... and the sharding
        self.enkf_noise_field, self.enkf_noise_relaxation = False, 0.0   # ... and the noise field
        self.enkf_forcing, self.enkf_forcing_relaxation = False, 0.0     # ... and the forcing state's analysis
        L.check(self.lib.hc_set_enkf(self.h, stride, sigma, loc, int(seed) & 0xFFFFFFFFFFFFFFFF))
        self.enkf_stride, self.enkf_sigma_cm, self.enkf_localisation_cm, self.enkf_seed = stride, sigma, loc, int(seed)

    def enkf_table(self):
        """[P][n_arow][8] float64 per analysis slot (slot j <-> row j stride): count, prior mean and std of y, innovation,
        log-likelihood increment, posterior mean and std of y, rejected members; count 0 and NaN where nothing was
        analysed.  Depths from the top node (z[i] - z[0])."""
        return self.assim_table("enkf")

    def set_enkf_table(self, table):
        self.set_assim_table("enkf", table)

    def enkf_gain(self):
        """[P][D] the gain K_d of the last analysis (test hook)."""
        out = np.zeros((self.P, self.D))
        L.check(self.lib.hc_get_enkf_gain(self.h, L.dptr(out)))
        return out

    def enkf_y(self):
        """[N] the forecast y_k of the last analysis, cm from the top node (test hook)."""
        out = np.zeros(self.N)
        L.check(self.lib.hc_get_enkf_y(self.h, L.dptr(out)))
        return out

    def enkf_eps(self):
        """[N] the observation perturbations eps_k of the last analysis (test hook)."""
        out = np.zeros(self.N)
        L.check(self.lib.hc_get_enkf_eps(self.h, L.dptr(out)))
        return out

    # -- the EnKF's analysis scheme and relaxation to prior spread (include/hydrocol.h hc_set_enkf_method) --------------
    def set_enkf_method(self, method="stochastic", relaxation=0.0):
        """``method``: "stochastic" (perturbed observations) or "sqrt" (the deterministic square-root analysis: nothing
        is drawn, the EnKF seed does not matter); ``relaxation``: the RTPS factor alpha in [0, 1] (0 = none): after each
        analysis every node's spread becomes (1 - alpha) sigma_a + alpha sigma_b.  The EnKF must be on (:meth:`set_enkf`
        first; it resets both)."""
        if method not in ENKF_METHODS:
            raise ValueError(f"EnKF method = {method!r} must be one of {list(ENKF_METHODS)}")
        alpha = float(relaxation)
        if not (np.isfinite(alpha) and 0.0 <= alpha <= 1.0):
            raise ValueError(f"EnKF relaxation = {relaxation!r} must be a finite number in [0, 1]")
        L.check(self.lib.hc_set_enkf_method(self.h, ENKF_METHODS.index(method), alpha))
        self.enkf_method, self.enkf_relaxation = method, alpha

    def get_enkf_method(self):
        """(method, relaxation) as the library holds them."""
        m, a = np.zeros(1, dtype=np.int32), np.zeros(1)
        L.check(self.lib.hc_get_enkf_method(self.h, L.iptr(m), L.dptr(a)))
        return ENKF_METHODS[int(m[0])], float(a[0])

    def enkf_width(self):
        """m' of the last analysis: 1 + the sensors and the lagged rows present on it."""
        w = np.zeros(1, dtype=np.int32)
        L.check(self.lib.hc_get_enkf_width(self.h, L.iptr(w)))
        return int(w[0]) or 1

    def enkf_sqrt_gain(self):
        """[P][D][m'] the reduced gain of the last analysis, a square-root one (test hook)."""
        out = np.zeros((self.P, self.D, self.enkf_width()))
        L.check(self.lib.hc_get_enkf_sqrt_gain(self.h, L.dptr(out)))
        return out

    def enkf_sqrt_shift(self):
        """[P][D] the mean's increment of the last analysis, a square-root one (test hook)."""
        out = np.zeros((self.P, self.D))
        L.check(self.lib.hc_get_enkf_sqrt_shift(self.h, L.dptr(out)))
        return out

    def enkf_relaxation_factors(self):
        """(sigma_b, sigma_a, f), [P][D] each, of the last analysis, a relaxed one (test hook)."""
        out = np.zeros((3, self.P, self.D))
        L.check(self.lib.hc_get_enkf_relaxation(self.h, L.dptr(out[0]), L.dptr(out[1]), L.dptr(out[2])))
        return out[0], out[1], out[2]

    # -- the noise field in the EnKF analysis (include/hydrocol.h hc_set_enkf_noise_field) ------------------------------
    def set_enkf_noise_field(self, on=True, relaxation=None):
        """Update every member's base noise vector -- its conductivity field -- together with its psi on every analysis
        row, from the same observations, draws and factor; ``relaxation``: the RTPS factor of the vectors' anomalies in
        [0, 1] (default: the one of :meth:`set_enkf_method`).  The EnKF must be on and not sharded.  In a Philox run the
        handle then feeds the step kernel its own normals as caller noise: set it after the spin-up, and
        :meth:`set_noise_scale` is refused while it is on."""
        on = bool(on)
        alpha = noise_field_relaxation(self.enkf_relaxation if relaxation is None else relaxation) if on else 0.0
        if on and not self.enkf_stride:
            raise ValueError("the noise field needs the EnKF on (set_enkf first)")
        if on and self.enkf_shard is not None:
            raise ValueError("the noise field with a sharded analysis: the exchanged partials cover psi only")
        L.check(self.lib.hc_set_enkf_noise_field(self.h, int(on), alpha))
        self.enkf_noise_field, self.enkf_noise_relaxation = on, alpha

    def get_enkf_noise_field(self):
        """(on, relaxation) as the library holds them."""
        m, a = np.zeros(1, dtype=np.int32), np.zeros(1)
        L.check(self.lib.hc_get_enkf_noise_field(self.h, L.iptr(m), L.dptr(a)))
        return bool(m[0]), float(a[0])

    def enkf_noise_table(self):
        """[P][n_arow][4 D + 1] float64 per analysis slot: the prior mean and std of every node's z, the mean and std
        after the relaxation, then the members whose updated vector was refused; NaN where nothing was analysed
        (:func:`split_enkf_noise_table`)."""
        return self.assim_table("enkf_noise")

    def set_enkf_noise_table(self, table):
        self.set_assim_table("enkf_noise", table)

    def enkf_noise_gain(self):
        """[P][m'][D] the vectors' gain of the last analysis (test hook)."""
        out = np.zeros((self.P, self.enkf_width(), self.D))
        L.check(self.lib.hc_get_enkf_noise_gain(self.h, L.dptr(out)))
        return out

    def enkf_noise_sqrt_gain(self):
        """[P][m'][D] the vectors' reduced gain of the last analysis, a square-root one (test hook)."""
        out = np.zeros((self.P, self.enkf_width(), self.D))
        L.check(self.lib.hc_get_enkf_noise_sqrt_gain(self.h, L.dptr(out)))
        return out

    def enkf_noise_sqrt_shift(self):
        """[P][D] the shift of the vectors' mean in the last analysis, a square-root one (test hook)."""
        out = np.zeros((self.P, self.D))
        L.check(self.lib.hc_get_enkf_noise_sqrt_shift(self.h, L.dptr(out)))
        return out

    def enkf_noise_base(self):
        """[N][D] the members' base noise vectors: a Philox run's with the noise field on, else the caller's
        (:meth:`get_noise_base`)."""
        if not self.philox:
            return self.get_noise_base()
        out = np.zeros((self.N, self.D))
        L.check(self.lib.hc_get_enkf_noise_base(self.h, L.dptr(out), 0, self.N))
        return out

    def set_enkf_noise_base(self, base):
        """Replace a Philox run's base noise vectors (a checkpoint taken with the noise field on)."""
        base = L.as_f64(base)
        if base.shape != (self.N, self.D):
            raise ValueError(f"base must be [{self.N}][{self.D}], got {base.shape}")
        L.check(self.lib.hc_set_enkf_noise_base(self.h, L.dptr(base)))

    # -- the members' forcing state in the EnKF analysis (include/hydrocol.h hc_set_enkf_forcing) ------------------------
    def set_enkf_forcing(self, on=True, relaxation=0.0):
        """Update every member's forcing state g -- the AR(1) behind its rainfall and demand factors
        (:meth:`set_forcing_perturbation`) -- together with its psi on every analysis row, from the same observations,
        draws and factor, without a taper on C_gY; ``relaxation``: the RTPS factor of g's anomalies in [0, 1] (g regains
        spread from its recursion, so 0 is a sound default).  The EnKF and the perturbation must be on, the analysis not
        sharded.  The analysed g is what the rest of the day and, through the recursion, every later day run with."""
        on = bool(on)
        alpha = forcing_enkf_relaxation(relaxation) if on else 0.0
        if on and not self.enkf_stride:
            raise ValueError("the forcing analysis needs the EnKF on (set_enkf first)")
        if on and self.enkf_shard is not None:
            raise ValueError("the forcing analysis with a sharded analysis: the exchanged partials cover psi only")
        L.check(self.lib.hc_set_enkf_forcing(self.h, int(on), alpha))
        self.enkf_forcing, self.enkf_forcing_relaxation = on, alpha

    def get_enkf_forcing(self):
        """(on, relaxation) as the library holds them."""
        m, a = np.zeros(1, dtype=np.int32), np.zeros(1)
        L.check(self.lib.hc_get_enkf_forcing(self.h, L.iptr(m), L.dptr(a)))
        return bool(m[0]), float(a[0])

    def enkf_forcing_table(self):
        """[P][n_arow][9] float64 per analysis slot: for stream s (0 precipitation, 1 demand) columns 4 s + (prior mean,
        prior std, mean and std after the relaxation) of g, then the members whose updated g was refused; NaN where
        nothing was analysed (:func:`split_enkf_forcing_table`)."""
        t = np.zeros((self.P, stride_rows(self.T, self.enkf_stride), ENKF_FORCING_WIDTH))
        L.check(self.lib.hc_get_enkf_g_table(self.h, L.dptr(t), t.size))
        return t

    def set_enkf_forcing_table(self, table):
        t = L.as_f64(table).reshape(-1)
        L.check(self.lib.hc_set_enkf_g_table(self.h, L.dptr(t), t.size))

    def enkf_forcing_gain(self):
        """[P][m'][2] the gain K^g of the last analysis (test hook)."""
        out = np.zeros((self.P, self.enkf_width(), 2))
        L.check(self.lib.hc_get_enkf_g_gain(self.h, L.dptr(out)))
        return out

    def enkf_forcing_sqrt_gain(self):
        """[P][m'][2] g's reduced gain of the last analysis, a square-root one (test hook)."""
        out = np.zeros((self.P, self.enkf_width(), 2))
        L.check(self.lib.hc_get_enkf_g_sqrt_gain(self.h, L.dptr(out)))
        return out

    def enkf_forcing_sqrt_shift(self):
        """[P][2] the shift of g's mean in the last analysis, a square-root one (test hook)."""
        out = np.zeros((self.P, 2))
        L.check(self.lib.hc_get_enkf_g_sqrt_shift(self.h, L.dptr(out)))
        return out

    # -- soil-moisture sensors in the EnKF analysis (include/hydrocol.h hc_set_enkf_soil_moisture) ----------------------
    def set_enkf_soil_moisture(self, nodes, values=None, sigma=None):
        """Add a record of volumetric water content at the depth nodes ``nodes`` (at most 8) to the EnKF's analyses:
        ``values`` [T][n] in [0, 1], NaN = no observation on that row; ``sigma`` the sensors' error (m^3/m^3), one number
        or one per sensor.  ``nodes`` empty or None removes the record.  The EnKF must be on (:meth:`set_enkf` first; it
        removes the record again)."""
        nodes, v, sg = self._sm_record(nodes, values, sigma)
        self.enkf_sm_nodes = None
        if nodes.size == 0:
            L.check(self.lib.hc_set_enkf_soil_moisture(self.h, 0, None, None, None))
            return
        L.check(self.lib.hc_set_enkf_soil_moisture(self.h, int(nodes.size), L.iptr(nodes), L.dptr(v), L.dptr(sg)))
        self.enkf_sm_nodes = nodes.copy()

    @property
    def enkf_sm_n(self):
        return 0 if self.enkf_sm_nodes is None else int(self.enkf_sm_nodes.size)

    def enkf_sm_table(self):
        """[P][n_arow][n][6] float64 per analysis slot and sensor: observed (0/1), observation, prior mean and std of
        theta, posterior mean and std of theta; NaN where the slot took no joint analysis (and after observed = 0)."""
        return self.assim_table("enkf_sm")

    def set_enkf_sm_table(self, table):
        self.set_assim_table("enkf_sm", table)

    def enkf_sm_width(self):
        """m' = 1 + the sensors present on the last analysis (0: it had none; test hook)."""
        w = np.zeros(1, dtype=np.int32)
        L.check(self.lib.hc_get_enkf_sm_width(self.h, L.iptr(w)))
        return int(w[0])

    def enkf_sm_y(self):
        """[N][m'] the observations Y_k of the last analysis: the well's y (cm from the top node), then theta (test hook)."""
        out = np.zeros((self.N, self.enkf_sm_width()))
        L.check(self.lib.hc_get_enkf_sm_y(self.h, L.dptr(out)))
        return out

    def enkf_sm_gain(self):
        """[P][D][m'] the gain K of the last analysis (test hook)."""
        out = np.zeros((self.P, self.D, self.enkf_sm_width()))
        L.check(self.lib.hc_get_enkf_sm_gain(self.h, L.dptr(out)))
        return out

    def enkf_sm_eps(self):
        """[N][n] the sensors' observation perturbations of the last analysis, every sensor of the record (test hook)."""
        out = np.zeros((self.N, self.enkf_sm_n))
        L.check(self.lib.hc_get_enkf_sm_eps(self.h, L.dptr(out)))
        return out

    # -- the well's record inside the window (include/hydrocol.h hc_set_enkf_window) -------------------------------------
    def set_enkf_window(self, offsets=()):
        """Asynchronous EnKF: every member's y on the rows ``offsets`` before an analysis row (integers in [1, stride),
        distinct, at most 8 together with the sensors) is recorded when the row is solved and joins that analysis as a
        further well-type observation.  Empty or None turns it off.  The EnKF must be on (:meth:`set_enkf` first; it
        turns the window off again)."""
        off = enkf_window_settings(offsets, self.enkf_stride, self.enkf_sm_n)
        self.enkf_window_offsets = ()
        a = np.ascontiguousarray(off, dtype=np.int32)
        L.check(self.lib.hc_set_enkf_window(self.h, a.size, L.iptr(a) if a.size else None))
        self.enkf_window_offsets = off

    @property
    def enkf_window_n(self):
        return len(self.enkf_window_offsets)

    def enkf_window_table(self):
        """[P][n_arow][n][4] float64 per analysis slot and offset: observed (0/1), observation, prior mean and std of the
        recorded y (cm from the top node); NaN where the slot's analysis had no lagged row (and after observed = 0)."""
        return self.assim_table("enkf_window")

    def set_enkf_window_table(self, table):
        self.set_assim_table("enkf_window", table)

    def enkf_window_capture(self):
        """(y [n][N], rows [n] int64): what the window holds for the coming analysis (row -1: nothing; checkpoints)."""
        y, rows = np.zeros((self.enkf_window_n, self.N)), np.zeros(self.enkf_window_n, dtype=np.int64)
        L.check(self.lib.hc_get_enkf_window_capture(self.h, L.dptr(y), L.lptr(rows)))
        return y, rows

    def set_enkf_window_capture(self, y, rows):
        y, rows = L.as_f64(y), np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        if y.shape != (self.enkf_window_n, self.N) or rows.size != self.enkf_window_n:
            raise ValueError(f"the window's capture must be [{self.enkf_window_n}, {self.N}] with as many rows")
        L.check(self.lib.hc_set_enkf_window_capture(self.h, L.dptr(y), L.lptr(rows)))

    def enkf_window_slots(self):
        """The indices into ``enkf_window_offsets`` of the last analysis's lagged columns, in column order (test hook)."""
        w, slots = np.zeros(1, dtype=np.int32), np.zeros(SM_MAX_SENSORS, dtype=np.int32)
        L.check(self.lib.hc_get_enkf_window_width(self.h, L.iptr(w), L.iptr(slots)))
        return slots[:int(w[0])].copy()

    def enkf_window_y(self):
        """[N][m_w] the recorded y of the last analysis's lagged columns, cm from the top node (test hook)."""
        out = np.zeros((self.N, self.enkf_window_slots().size))
        L.check(self.lib.hc_get_enkf_window_y(self.h, L.dptr(out)))
        return out

    def enkf_window_eps(self):
        """[N][m_w] the perturbations of the last analysis's lagged columns (test hook)."""
        out = np.zeros((self.N, self.enkf_window_slots().size))
        L.check(self.lib.hc_get_enkf_window_eps(self.h, L.dptr(out)))
        return out

    def enkf_full_gain(self):
        """[P][D][m'] the gain K of the last analysis, every column: well, sensors, lagged rows (test hook)."""
        out = np.zeros((self.P, self.D, self.enkf_width()))
        L.check(self.lib.hc_get_enkf_window_gain(self.h, L.dptr(out)))
        return out

    # -- one point's members on several handles (include/hydrocol.h hc_set_enkf_shard) ----------------------------------
    def enkf_shard_words(self, n_global):
        """Doubles the shard's exchange buffer must hold for ``n_global`` members, as the sensors and the window stand."""
        n = np.zeros(1, dtype=np.int64)
        L.check(self.lib.hc_get_enkf_shard_words(self.h, int(n_global), L.lptr(n)))
        return int(n[0])

    def set_enkf_shard(self, n_global, first_global=0, exchange=None):
        """This handle holds members [first_global, first_global + N) of a point with ``n_global`` members: its analyses
        become those of the whole ensemble, to the bit.  ``exchange(block, first_word, count_words)`` is called before
        each of the analysis's reductions with ``block``, a float64 device tensor (a view of the handle's exchange buffer)
        whose words [first_word, first_word + count_words) are this handle's; on return everyone else's must be in place
        (:class:`multigpu.ShardExchange`; None: nothing to gather, for a handle that holds every member).  An exception it
        raises fails the step.  ``n_global`` = 0 turns sharding off.  The EnKF, its sensors and its window come first.
        torch must have been imported before this process made its first handle (``_lib.load``)."""
        n_global, first = int(n_global), int(first_global)
        self._shard_keep = None
        if not n_global:
            L.check(self.lib.hc_set_enkf_shard(self.h, 0, 0, None, 0, L.EXCHANGE_FN(), None))
            self.enkf_shard = None
            return
        L.load(with_torch=True)                    # the buffer is torch's: one HIP runtime must serve both
        import torch
        buf = torch.zeros(max(self.enkf_shard_words(n_global), 1), dtype=torch.float64,
                          device=torch.device("cuda", self.device))
        base = buf.data_ptr()

        def call(_ctx, ptr, n_words, first_word, count_words):
            try:                                   # nothing may propagate through the C frames
                if exchange is not None:
                    at = (int(ptr) - base) // 8
                    exchange(buf[at:at + n_words], int(first_word), int(count_words))
                return 0
            except BaseException as e:  # noqa: BLE001
                self._shard_error = e
                return 1

        fn = L.EXCHANGE_FN(call)
        L.check(self.lib.hc_set_enkf_shard(self.h, n_global, first, C.c_void_p(base), buf.numel(), fn, None))
        self._shard_keep = (buf, fn, call)         # alive as long as the handle may call them
        self.enkf_shard = (n_global, first)

    def get_enkf_shard(self):
        """(n_global, first_global) as the library holds them; (0, 0): off."""
        n, f = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
        L.check(self.lib.hc_get_enkf_shard(self.h, L.lptr(n), L.lptr(f)))
        return int(n[0]), int(f[0])

    # -- hooks ----------------------------------------------------------------------
    def spinup(self, zwtd_cm, z0_cm, forcing_row=0, max_iterations=1500):
        """Per-member ``Simulation.initial_conditions`` (simulation.py:389-493) in one launch: every member
        iterates from its current state with its own noise vector until its own stop rule holds.
        Returns (iterations[N] -- negative where the cap was reached, kernel_ms)."""
        iters = np.zeros(self.N, dtype=np.int32)
        a = L.SpinupArgs()
        a.forcing_row, a.max_iterations = int(forcing_row), int(max_iterations)
        a.zwtd_cm, a.z0_cm = float(zwtd_cm), float(z0_cm)
        a.iterations_out = L.iptr(iters)
        L.check(self.lib.hc_spinup(self.h, C.byref(a)))
        return iters, a.kernel_ms

    def rhs(self, row, spinup=False, want_aux=False, variant="hook", want_diag=False):
        """dy/dt of every member's state on forcing row `row` (hc_rhs_ex).  `variant`: "hook" -- rhs_eval's plain
        instantiation; "step" -- the instantiation and wave layout of this handle's step kernel; "hook_layout" -- the
        plain instantiation on the step kernel's wave layout (include/hydrocol.h).  Returns dydt [N][D]; with `want_aux`
        also {"c", "s", "f": [N][D-1], "pL": [N]}; with `want_diag` that dict also holds "diag": [N][2] = transpiration,
        lateral flow of the evaluation."""
        out = np.empty((self.N, self.D))
        M = self.D - 1
        aux = np.empty((self.N, 3 * M + 1)) if want_aux else None
        diag = np.empty((self.N, 2)) if want_diag else None
        L.check(self.lib.hc_rhs_ex(self.h, int(row), int(spinup), L.RHS_VARIANTS[variant], L.dptr(out),
                                   L.dptr(aux) if want_aux else None, L.dptr(diag) if want_diag else None))
        if not (want_aux or want_diag):
            return out
        extra = {}
        if want_aux:
            extra.update(c=aux[:, :M], s=aux[:, M:2 * M], f=aux[:, 2 * M:3 * M], pL=aux[:, 3 * M])
        if want_diag:
            extra["diag"] = diag
        return out, extra

    def model_nodes(self):
        out = np.empty((4, self.N, self.D))
        qinf = np.empty(self.N)
        L.check(self.lib.hc_model_nodes(self.h, L.dptr(out), L.dptr(qinf)))
        return {"theta": out[0], "K": out[1], "C": out[2], "K_bkg": out[3], "q_inf_max": qinf}


def moments_to_mean_std(moments, dz, z0=0.0):
    """mu/sigma of the water-table depth [cm] per row from (count, sum idx, sum idx^2): the reference reports
    ``z[wtd_est]`` with ``z[i] = z0 + i dz`` (simulation.py:140,612; ``z0 = well["soil"]``).  Accepts [3][T] or [P][3][T]."""
    moments = np.asarray(moments)
    cnt = moments[..., 0, :].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_idx = moments[..., 1, :] / cnt
        var_idx = np.maximum(moments[..., 2, :] / cnt - mean_idx ** 2, 0.0)
    return z0 + dz * mean_idx, dz * np.sqrt(var_idx)


# ---- profile statistics on the host: layout, quantisation, limb normalisation (include/hydrocol.h) ----------------------
PROF_WORDS = 5
PROF_SCALE_PSI, PROF_SCALE_THETA, PROF_SCALE_FLUX = 16, 40, 32
PROF_Q_MAX = (1 << 40) - 1


def stride_rows(T, stride):
    """Rows of a table that samples every ``stride``-th of ``T`` forcing rows: rows 0, stride, 2 stride, ... < T."""
    return (int(T) - 1) // int(stride) + 1


def profile_layout(P, T, D, stride):
    """{part: (offset, shape)} of the int64 table: prof [P][T_out][D][2][5] (psi_press, theta_vol), pcnt [P][T_out],
    flux [P][T][2][5] (transpiration, lateral_flow), fcnt [P][T], aerr [P][T], ovf [1]; T_out = stride_rows(T, stride)."""
    return diag_layout("profile", diag_counts(P, T, D, profile_stride=stride))


def split_profile_table(table, P, T, D, stride):
    """Views of the parts of a flat table (see :func:`profile_layout`)."""
    return split_diag("profile", table, diag_counts(P, T, D, profile_stride=stride))


def join_profile_table(parts):
    """The flat table of ``split_profile_table`` parts (same order)."""
    return join_diag("profile", parts)


def profile_quantise(x, scale_bits):
    """q = rint(x 2^s) clamped to |q| <= 2^40 - 1 (NaN -> 0), as the device does; returns (q int64, values clamped)."""
    y = np.rint(np.asarray(x, dtype=np.float64) * 2.0 ** scale_bits)
    bad = ~(np.abs(y) <= PROF_Q_MAX)
    y = np.where(np.isnan(y), 0.0, np.clip(y, -PROF_Q_MAX, PROF_Q_MAX))
    return y.astype(np.int64), int(bad.sum())


def profile_words_of(q):
    """[..., 5] int64 words one member adds for quantised values q: q, then the 20-bit limbs of q^2."""
    q = np.asarray(q, dtype=np.int64)
    a = np.abs(q).astype(object)
    sq = a * a
    limbs = [np.asarray((sq >> (20 * k)) & ((1 << 20) - 1), dtype=np.int64) for k in range(4)]
    return np.stack([q] + limbs, axis=-1)


def limbs_to_mean_std(count, words, scale_bits):
    """Mean and population sigma from (count, [..., 5] words): the limbs are recombined with Python integers, the
    variance numerator n sum q^2 - (sum q)^2 is formed exactly and only then divided and rounded (no E[x^2] - E[x]^2
    cancellation).  Entries with count 0 are NaN.  Same convention as :func:`moments_to_mean_std`."""
    words = np.asarray(words, dtype=np.int64)
    n = np.broadcast_to(np.asarray(count, dtype=np.int64), words.shape[:-1])
    empty = n <= 0
    no = np.where(empty, 1, n).astype(object)
    s1 = words[..., 0].astype(object)
    s2 = sum(words[..., k + 1].astype(object) * (1 << (20 * k)) for k in range(4))
    var_num = no * s2 - s1 * s1
    scale = 2.0 ** -scale_bits
    mean = np.asarray(np.asarray(s1 / no, dtype=np.float64) * scale)
    std = np.asarray(np.sqrt(np.asarray(var_num / (no * no), dtype=np.float64)) * scale)
    return np.where(empty, np.nan, mean), np.where(empty, np.nan, std)


def profile_tables_to_stats(table, P, T, D, stride, porosity, dz):
    """The science arrays of a profile-statistics table: ``{theta_vol, psi_press, S_eff}_{mean,std}`` [P][T_out][D]
    (S_eff = theta_vol / porosity, simulation.py:658), ``{transpiration, lateral_flow}_{mean,std}`` and
    ``abs_error_mean`` [P][T] (NaN where no member was counted), ``rows`` [T_out], ``count`` [P][T_out] (members in each
    profile row), ``row_count`` [P][T] and ``overflow``.  The leading [P] axis is dropped for a single point."""
    parts = split_profile_table(table, P, T, D, stride)
    pcnt = parts["pcnt"][..., None]
    out = {}
    out["psi_press_mean"], out["psi_press_std"] = limbs_to_mean_std(pcnt, parts["prof"][..., 0, :], PROF_SCALE_PSI)
    out["theta_vol_mean"], out["theta_vol_std"] = limbs_to_mean_std(pcnt, parts["prof"][..., 1, :], PROF_SCALE_THETA)
    por = np.asarray(porosity, dtype=np.float64).reshape(P, 1, D)
    out["S_eff_mean"], out["S_eff_std"] = out["theta_vol_mean"] / por, out["theta_vol_std"] / por
    fcnt = parts["fcnt"]
    out["transpiration_mean"], out["transpiration_std"] = limbs_to_mean_std(fcnt, parts["flux"][..., 0, :], PROF_SCALE_FLUX)
    out["lateral_flow_mean"], out["lateral_flow_std"] = limbs_to_mean_std(fcnt, parts["flux"][..., 1, :], PROF_SCALE_FLUX)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["abs_error_mean"] = np.where(fcnt > 0, float(dz) * parts["aerr"] / np.maximum(fcnt, 1), np.nan)
    out["count"], out["row_count"] = parts["pcnt"].copy(), fcnt.copy()
    if P == 1:
        out = {k: v[0] for k, v in out.items()}
    out["rows"] = np.arange(parts["pcnt"].shape[1], dtype=np.int64) * int(stride)
    out["overflow"] = int(parts["ovf"][0])
    return out


# ---- water-table distributions (include/hydrocol.h hc_set_wtd_hist, hc_wtd_distribution) -------------------------------
WTD_MAX_LEVELS = 16
INT32_MAX = (1 << 31) - 1


wtd_hist_slots = stride_rows      # histogram rows of T forcing rows at a stride (the profile rows of the same stride)


def wtd_hist_rows(T, stride):
    """The forcing row of each slot: slot j <-> row j stride (the profile rows of the same stride)."""
    return np.arange(wtd_hist_slots(T, stride), dtype=np.int64) * int(stride)


def wtd_distribution(hist, obs_idx, levels, dz, z, device=0, stride=1):
    """Quantiles and CRPS of water-table histograms ``hist`` [..., n_hrow, D] (one table, or [P] of them) on the GPU
    (``hc_wtd_distribution``).  ``obs_idx`` is the forcing's observation index of every row (``forcing.wtd_obs``); slot j
    is row j ``stride``.  Returns ``rows`` [n_hrow], ``count`` [..., n_hrow], ``quantile_idx`` [..., n_hrow, L] (-1: no
    member), ``quantile_cm`` (``z[idx]``, NaN for -1), ``crps_cm`` [..., n_hrow] (NaN: no member) and ``crps_mean_cm``
    [...] (the mean over rows with members: the ensemble's analogue of the reference's MAE) and ``levels``."""
    lib = L.load()
    hist = np.asarray(hist)
    if hist.ndim < 2:
        raise ValueError(f"histograms must be [..., n_hrow, D], got shape {hist.shape}")
    if hist.size and (hist.min() < 0 or hist.max() > INT32_MAX):
        raise ValueError("histogram counts must lie in [0, 2^31 - 1]")
    lv = np.ascontiguousarray(np.asarray(levels, dtype=np.float64).reshape(-1))
    if lv.size > WTD_MAX_LEVELS or not np.all((lv >= 0.0) & (lv <= 1.0)):
        raise ValueError(f"at most {WTD_MAX_LEVELS} quantile levels, each in [0, 1]: got {lv.tolist()}")
    lead, n_hrow, D = hist.shape[:-2], hist.shape[-2], hist.shape[-1]
    rows = np.arange(n_hrow, dtype=np.int64) * int(stride)
    obs = np.asarray(obs_idx, dtype=np.int64).reshape(-1)
    if rows.size and rows[-1] >= obs.size:
        raise ValueError(f"{n_hrow} histogram rows at stride {stride} need {rows[-1] + 1} observations, got {obs.size}")
    obs = np.ascontiguousarray(np.broadcast_to(obs[rows].astype(np.int32), lead + (n_hrow,)).reshape(-1))
    h = np.ascontiguousarray(hist, dtype=np.int32).reshape(-1, D)
    R = h.shape[0]
    count = np.zeros(R, dtype=np.int64)
    qidx = np.zeros((R, lv.size), dtype=np.int32)
    crps = np.zeros(R, dtype=np.float64)
    L.check(lib.hc_wtd_distribution(int(device), L.iptr(h), L.iptr(obs), R, D, L.dptr(lv), lv.size, float(dz),
                                    L.lptr(count), L.iptr(qidx), L.dptr(crps)))
    z = np.asarray(z, dtype=np.float64)
    qcm = np.where(qidx >= 0, z[np.clip(qidx, 0, D - 1)], np.nan)
    count, crps = count.reshape(lead + (n_hrow,)), crps.reshape(lead + (n_hrow,))
    with np.errstate(invalid="ignore"):
        solved = count > 0
        crps_mean = np.where(solved.any(axis=-1), np.where(solved, crps, 0.0).sum(axis=-1) / np.maximum(solved.sum(axis=-1), 1),
                             np.nan)
    if not lead:
        crps_mean = float(crps_mean)
    return {"rows": rows, "count": count, "quantile_idx": qidx.reshape(lead + (n_hrow, lv.size)),
            "quantile_cm": qcm.reshape(lead + (n_hrow, lv.size)), "crps_cm": crps, "crps_mean_cm": crps_mean,
            "levels": lv}


# ---- soil-moisture distributions (include/hydrocol.h hc_set_theta_hist) ------------------------------------------------
THETA_HIST_BINS = (32, 64, 128)


def theta_hist_of(theta, bins):
    """The device's binning of one row restated: ``theta`` [N][D] -> (hist [D][bins] int64, outside).  A value goes to bin
    floor(theta bins) (theta bins is exact: bins is a power of two), 1.0 to the last bin; NaN, values below 0 and above 1
    go to no bin and are counted in ``outside``."""
    bins = int(bins)
    if bins not in THETA_HIST_BINS:
        raise ValueError(f"theta histograms have 32, 64 or 128 bins, not {bins}")
    th = np.asarray(theta, dtype=np.float64)
    th = th.reshape(-1, th.shape[-1])
    inside = (th >= 0.0) & (th <= 1.0)
    with np.errstate(invalid="ignore"):
        b = np.where(th == 1.0, bins - 1, np.floor(np.where(inside, th, 0.0) * bins)).astype(np.int64)
    hist = np.zeros((th.shape[1], bins), dtype=np.int64)
    node = np.broadcast_to(np.arange(th.shape[1]), th.shape)
    np.add.at(hist, (node[inside], b[inside]), 1)
    return hist, int((~inside).sum())


def theta_distribution(hist, levels, bins=None, stride=1):
    """Quantile bands of theta(z) from histograms ``hist`` [..., R, D, B] (one table, or [P] of them), in NumPy integers.
    Level p of a row and node is the centre (b + 0.5) / B of the first bin b whose cumulative count reaches
    k = max(1, ceil(n p)) in fp64 -- the rank of :func:`wtd_distribution`, numpy.quantile(..., method="inverted_cdf") on the
    bin index.  Returns ``rows`` [R], ``count`` [..., R] (members per row: every node holds as many, but for values outside
    the bins), ``quantiles`` [..., R, L, D] (NaN where a node counted nobody), ``levels`` and ``saturated_fraction``
    [..., R, D]: the share of the node's members in its highest bin occupied on any row of the table -- the bin that holds
    the node's porosity once any member has been saturated there."""
    hist = np.asarray(hist)
    if hist.ndim < 3:
        raise ValueError(f"histograms must be [..., R, D, B], got shape {hist.shape}")
    B = hist.shape[-1]
    if B not in THETA_HIST_BINS or (bins is not None and int(bins) != B):
        raise ValueError(f"histograms of {B} bins (32, 64 or 128{'' if bins is None else f'; {bins} were named'})")
    if hist.size and hist.min() < 0:
        raise ValueError("histogram counts must be >= 0")
    lv = np.asarray(levels, dtype=np.float64).reshape(-1)
    if lv.size > WTD_MAX_LEVELS or not np.all((lv >= 0.0) & (lv <= 1.0)):
        raise ValueError(f"at most {WTD_MAX_LEVELS} quantile levels, each in [0, 1]: got {lv.tolist()}")
    h = hist.astype(np.int64)
    cum = np.cumsum(h, axis=-1)                                     # [..., R, D, B]
    n = cum[..., -1]                                                # [..., R, D]
    k = np.maximum(1, np.ceil(n[..., None, :].astype(np.float64) * lv[:, None]).astype(np.int64))     # [..., R, L, D]
    idx = (cum[..., None, :, :] < k[..., None]).sum(axis=-1)        # bins whose cumulative count stays below k
    q = np.where(n[..., None, :] > 0, (np.minimum(idx, B - 1) + 0.5) / B, np.nan)
    occupied = h.sum(axis=-3) > 0                                   # [..., D, B] over the rows
    top = B - 1 - np.argmax(occupied[..., ::-1], axis=-1)           # [..., D]: highest occupied bin (B - 1 if none)
    in_top = np.take_along_axis(h, np.broadcast_to(top[..., None, :, None], h.shape[:-1] + (1,)), axis=-1)[..., 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        sat = np.where(n > 0, in_top / np.maximum(n, 1), np.nan)
    return {"rows": np.arange(hist.shape[-3], dtype=np.int64) * int(stride), "count": n.max(axis=-1), "quantiles": q,
            "levels": lv, "saturated_fraction": sat}


# ---- soil-water storage by depth layer (include/hydrocol.h hc_set_layer_storage) --------------------------------------
STORAGE_MAX_LAYERS = 8
STORAGE_BINS = (32, 64, 128, 256, 512, 1024)
STORAGE_MAX_CM = 4096.0
PROF_SCALE_STORAGE = 28


def layer_ranges(z, layers_cm):
    """Node ranges [L][2] = (i0, i1) of the depth layers ``layers_cm`` = [(top, bottom), ...] in cm on the grid ``z``
    (ascending): layer l holds the nodes with top <= z_i < bottom.  ValueError for more than 8 layers, for top >= bottom and
    for a layer that holds no node."""
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    layers = [tuple(float(v) for v in np.asarray(lay, dtype=np.float64).reshape(-1)) for lay in layers_cm]
    if not 1 <= len(layers) <= STORAGE_MAX_LAYERS:
        raise ValueError(f"1 to {STORAGE_MAX_LAYERS} storage layers, got {len(layers)}")
    out = []
    for lay in layers:
        if len(lay) != 2 or not all(np.isfinite(lay)) or lay[0] >= lay[1]:
            raise ValueError(f"a storage layer is (top, bottom) in cm with top < bottom, got {lay!r}")
        i0, i1 = int(np.searchsorted(z, lay[0], side="left")), int(np.searchsorted(z, lay[1], side="left"))
        if i0 >= i1:
            raise ValueError(f"storage layer {lay!r} cm holds no node of the column [{float(z[0])!r}, {float(z[-1])!r}] cm")
        out.append((i0, i1))
    return np.array(out, dtype=np.int32)


def _check_ranges(ranges, D):
    r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    if not 1 <= r.shape[0] <= STORAGE_MAX_LAYERS or np.any(r[:, 0] < 0) or np.any(r[:, 0] >= r[:, 1]) or np.any(r[:, 1] > D):
        raise ValueError(f"1 to {STORAGE_MAX_LAYERS} node ranges [i0, i1) with 0 <= i0 < i1 <= {D}, got {r.tolist()}")
    return r


def layer_storage_of(theta, ranges, dz):
    """The device's per-member reduction restated: ``theta`` [N][D] -> (S [N][L] in cm, u [N][L]).  T is summed in the
    order of include/hydrocol.h, fixed by (i0, i1) alone: x_j (j = 0..63) starts at 0.0 and adds theta_i of the layer's
    nodes with i mod 64 == j in ascending i; then x_j += x_{j+32}, x_j += x_{j+16}, ..., x_0 += x_1.  S = dz T,
    u = T / (i1 - i0).  Equal to the device's bits."""
    th = np.asarray(theta, dtype=np.float64)
    th = th.reshape(-1, th.shape[-1])
    r = _check_ranges(ranges, th.shape[1])
    S, u = np.zeros((th.shape[0], len(r))), np.zeros((th.shape[0], len(r)))
    for l, (i0, i1) in enumerate(r):
        x = np.zeros((th.shape[0], 64))
        for i in range(int(i0), int(i1)):
            x[:, i % 64] = x[:, i % 64] + th[:, i]
        s = 32
        while s:
            x[:, :s] = x[:, :s] + x[:, s:2 * s]
            s //= 2
        S[:, l], u[:, l] = float(dz) * x[:, 0], x[:, 0] / float(i1 - i0)
    return S, u


def layer_storage_hist_of(u, bins):
    """The device's binning of one row's layer means ``u`` [N][L] -> (hist [L][bins] int64, outside): bin floor(u bins)
    (exact: bins is a power of two), 1.0 to the last bin; NaN, values below 0 and above 1 go to no bin."""
    bins = int(bins)
    if bins not in STORAGE_BINS:
        raise ValueError(f"storage histograms have a power of two in 32 .. 1024 bins, not {bins}")
    u = np.asarray(u, dtype=np.float64)
    inside = (u >= 0.0) & (u <= 1.0)
    with np.errstate(invalid="ignore"):
        b = np.where(u == 1.0, bins - 1, np.floor(np.where(inside, u, 0.0) * bins)).astype(np.int64)
    hist = np.zeros((u.shape[1], bins), dtype=np.int64)
    layer = np.broadcast_to(np.arange(u.shape[1]), u.shape)
    np.add.at(hist, (layer[inside], b[inside]), 1)
    return hist, int((~inside).sum())


def layer_storage_table_layout(P, T, L, stride):
    """{part: (offset, shape)} of the int64 table: stor [P][T_out][L][5], scnt [P][T_out], ovf [1]."""
    return diag_layout("storage", diag_counts(P, T, profile_stride=stride, storage_layers=L))


def split_layer_storage_table(table, P, T, L, stride):
    """Views of the parts of a flat moments table (see :func:`layer_storage_table_layout`)."""
    return split_diag("storage", table, diag_counts(P, T, profile_stride=stride, storage_layers=L))


def layer_storage_tables_of(theta_rows, ranges, dz, bins=0, counted=None):
    """Both tables of one point from the members' theta on every profile row, ``theta_rows`` [R][N][D] (``counted`` [R]
    bool: rows that count their members; default all): the flat int64 moments table (stor [1][R][L][5], scnt, ovf) and,
    with ``bins``, (hist [R][L][bins] int32, outside) -- else (None, 0).  The device's tables, bit for bit."""
    th = np.asarray(theta_rows, dtype=np.float64)
    R, N, D = th.shape
    r = _check_ranges(ranges, D)
    counted = np.ones(R, dtype=bool) if counted is None else np.asarray(counted, dtype=bool)
    stor = np.zeros((1, R, len(r), PROF_WORDS), dtype=np.int64)
    scnt, ovf, outside = np.zeros((1, R), dtype=np.int64), 0, 0
    hist = np.zeros((R, len(r), int(bins)), dtype=np.int64) if bins else None
    for j in range(R):
        if not counted[j]:
            continue
        S, u = layer_storage_of(th[j], r, dz)
        q, bad = profile_quantise(S, PROF_SCALE_STORAGE)
        stor[0, j] = profile_words_of(q).astype(object).sum(axis=0).astype(np.int64)
        scnt[0, j], ovf = N, ovf + bad
        if bins:
            hist[j], out = layer_storage_hist_of(u, bins)
            outside += out
    table = np.concatenate([stor.reshape(-1), scnt.reshape(-1), np.array([ovf], dtype=np.int64)])
    return table, (hist.astype(np.int32) if bins else None, outside)


def layer_storage_stats(table, P, T, L, stride):
    """Mean and population sigma of the storage [cm] from a moments table, as :func:`profile_tables_to_stats` forms them
    (exact integers, rounded once): ``mean_cm``, ``std_cm`` [P][T_out][L] (NaN where no member was counted), ``count``
    [P][T_out], ``rows`` [T_out] and ``overflow``.  The leading [P] axis is dropped for a single point."""
    parts = split_layer_storage_table(table, P, T, L, stride)
    out = {}
    out["mean_cm"], out["std_cm"] = limbs_to_mean_std(parts["scnt"][..., None], parts["stor"], PROF_SCALE_STORAGE)
    out["count"] = parts["scnt"].copy()
    if P == 1:
        out = {k: v[0] for k, v in out.items()}
    out["rows"] = np.arange(parts["scnt"].shape[1], dtype=np.int64) * int(stride)
    out["overflow"] = int(parts["ovf"][0])
    return out


# ---- conductivity profiles (include/hydrocol.h hc_set_conductivity_stats) ------------------------------------------------
PROF_SCALE_LNK = 30


def conductivity_settings(value):
    """The run option ``conductivity`` normalised: None / False -> None (off); True -> {"layers_cm": None} (the node
    statistics alone); {"layers_cm": [(top, bottom), ...]} -> the same with the layers as float64 [L][2].  TypeError for any
    other value, ValueError for an unknown key or layers that are not 1 to 8 (top, bottom) pairs with top < bottom."""
    if value is None or value is False:
        return None
    if value is True:
        return {"layers_cm": None}
    if not isinstance(value, dict):
        raise TypeError(f"conductivity is None, True or {{'layers_cm': [(top, bottom), ...]}}, got {value!r}")
    unknown = sorted(set(value) - {"layers_cm"})
    if unknown:
        raise ValueError(f"conductivity has unknown keys {unknown} (known: ['layers_cm'])")
    layers = value.get("layers_cm")
    if layers is None or np.size(layers) == 0:
        return {"layers_cm": None}
    layers = np.asarray(layers, dtype=np.float64)
    if layers.ndim != 2 or layers.shape[1] != 2 or not 1 <= layers.shape[0] <= STORAGE_MAX_LAYERS:
        raise ValueError(f"conductivity.layers_cm holds 1 to {STORAGE_MAX_LAYERS} (top, bottom) pairs in cm, got {value['layers_cm']!r}")
    if not np.all(np.isfinite(layers)) or np.any(layers[:, 0] >= layers[:, 1]):
        raise ValueError(f"a conductivity layer is (top, bottom) in cm with top < bottom, got {layers.tolist()!r}")
    return {"layers_cm": layers}


def conductivity_ranges(z, dz, layers_cm):
    """Node ranges [L][2] of the conductivity layers on the grid ``z`` (:func:`layer_ranges`; no layers: [0][2]), with the
    layer storage's refusals: a layer that holds no node, and one of 4096 cm or more."""
    if layers_cm is None or np.size(layers_cm) == 0:
        return np.zeros((0, 2), dtype=np.int32)
    ranges = layer_ranges(z, layers_cm)
    for lay, (i0, i1) in zip(np.asarray(layers_cm, dtype=np.float64).reshape(-1, 2), ranges):
        if (int(i1) - int(i0)) * float(dz) >= STORAGE_MAX_CM:
            raise ValueError(f"conductivity layer {lay.tolist()!r} holds {(int(i1) - int(i0)) * float(dz):g} cm of column; "
                             f"a layer must stay below {STORAGE_MAX_CM:g} cm")
    return ranges


def conductivity_noise_of(base, fresh, refresh, failed, scale=None):
    """The noise vector the conductivity statistics use on each row of a batch: the vector the row's solve left behind
    (include/hydrocol.h).  One member: ``refresh`` / ``failed`` [n] are the rows' refresh flag and count of failed
    attempts, ``fresh`` [n_refresh][D] the vectors of the batch's refresh rows.  Returns [n][D].

    Vectors in memory (``scale`` None): ``base`` [D] is the base vector when the batch starts; a row that does not
    refresh damps it in place, x0.8 per failed attempt, for itself and every later row, and a refresh row damps its own
    copy only -- :func:`hydromodel_amd.simulation.rows_noise`.  In-kernel Philox (``scale``: the member's scale when the
    batch starts): ``base`` is the draw-0 normals xi; a row that does not refresh multiplies the SCALE by 0.8 per failed
    attempt and its vector is xi * scale, one product, as the step kernel rebuilds it; a refresh row as above."""
    from .simulation import rows_noise
    base = np.array(base, dtype=np.float64).reshape(-1)
    refresh, failed = np.asarray(refresh, dtype=bool).reshape(-1), np.asarray(failed, dtype=np.int64).reshape(-1)
    fresh = np.asarray(fresh, dtype=np.float64).reshape(-1, base.size)
    if scale is None:
        return rows_noise(base, fresh, refresh, failed)
    out, s, k = np.empty((refresh.size, base.size)), np.float64(scale), 0
    for i, (is_fresh, n_fail) in enumerate(zip(refresh, failed)):
        if is_fresh:
            out[i] = rows_noise(base, fresh[k:k + 1], [True], [n_fail])[0]
            k += 1
        else:
            for _ in range(int(n_fail)):
                s = s * 0.8
            out[i] = base * s
    return out


def conductivity_layer_of(k_hrc, ranges):
    """The device's per-member reduction restated: ``k_hrc`` [N][D] -> K_eff [N][L] = n / sum 1 / K_hrc,i over the layer's n
    nodes, the sum in :func:`layer_storage_of`'s order on 1 / K.  Equal to the device's bits."""
    with np.errstate(divide="ignore", invalid="ignore"):
        R, _ = layer_storage_of(1.0 / np.asarray(k_hrc, dtype=np.float64), ranges, 1.0)
        n = np.diff(_check_ranges(ranges, np.shape(k_hrc)[-1]), axis=1).reshape(-1).astype(np.float64)
        return n / R


def conductivity_table_layout(P, T, D, L, stride):
    """{part: (offset, shape)} of the int64 table: kmom [P][T_out][D][2][5] (K_hrc, K_bkg), kcnt [P][T_out][D][2],
    kmom_layer [P][T_out][L][5], kcnt_layer [P][T_out][L], ovf [1]."""
    return diag_layout("conductivity", diag_counts(P, T, D, profile_stride=stride, conductivity_layers=L))


def split_conductivity_table(table, P, T, D, L, stride):
    """Views of the parts of a flat table (see :func:`conductivity_table_layout`)."""
    return split_diag("conductivity", table, diag_counts(P, T, D, profile_stride=stride, conductivity_layers=L))


def _lnk_words(lnk):
    """(words [..., 5] summed over axis 0, members added [...], values clamped) of ln K [N][...]: a value that is not
    finite adds nothing."""
    lnk = np.asarray(lnk, dtype=np.float64)
    ok = np.isfinite(lnk)
    q, bad = profile_quantise(np.where(ok, lnk, 0.0), PROF_SCALE_LNK)
    words = np.where(ok[..., None], profile_words_of(q), 0)
    return words.astype(object).sum(axis=0).astype(np.int64), ok.sum(axis=0).astype(np.int64), bad


def conductivity_tables_of(lnk_rows, ranges=(), counted=None, k_rows=None):
    """The table of one point from the members' ln K on every profile row, ``lnk_rows`` [R][2][N][D] (ln K_hrc, ln K_bkg;
    ``counted`` [R] bool: rows that count their members, default all), with the layers ``ranges`` from ``k_rows`` [R][N][D]
    = K_hrc (default: exp of its ln): the flat int64 table (kmom [1][R][D][2][5], kcnt, kmom_layer, kcnt_layer, ovf).  A
    value that is not finite (K = 0, NaN, infinite) is left out and, through the count, visible; one beyond 2^10 is clamped
    and counted in ovf.  The device's table, bit for bit."""
    lnk = np.asarray(lnk_rows, dtype=np.float64)
    R, _, N, D = lnk.shape
    r = _check_ranges(ranges, D) if np.size(ranges) else np.zeros((0, 2), dtype=np.int64)
    counted = np.ones(R, dtype=bool) if counted is None else np.asarray(counted, dtype=bool)
    kmom, kcnt = np.zeros((1, R, D, 2, PROF_WORDS), dtype=np.int64), np.zeros((1, R, D, 2), dtype=np.int64)
    lmom, lcnt, ovf = np.zeros((1, R, len(r), PROF_WORDS), dtype=np.int64), np.zeros((1, R, len(r)), dtype=np.int64), 0
    for j in range(R):
        if not counted[j]:
            continue
        for q in range(2):
            kmom[0, j, :, q], kcnt[0, j, :, q], bad = _lnk_words(lnk[j, q])
            ovf += bad
        if len(r):
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                keff = conductivity_layer_of(np.exp(lnk[j, 0]) if k_rows is None else np.asarray(k_rows)[j], r)
                ln = np.log(np.where((keff > 0.0) & (keff < np.inf), keff, np.nan))
            lmom[0, j], lcnt[0, j], bad = _lnk_words(ln)
            ovf += bad
    return np.concatenate([kmom.reshape(-1), kcnt.reshape(-1), lmom.reshape(-1), lcnt.reshape(-1),
                           np.array([ovf], dtype=np.int64)])


def conductivity_stats(table, P, T, D, L, stride):
    """Mean and population sigma of ln K from a table, as :func:`profile_tables_to_stats` forms them (exact integers,
    rounded once), and the geometric mean K = exp(mean): ``lnK_{hrc,bkg}_{mean,std}``, ``K_{hrc,bkg}_geomean`` [P][T_out][D]
    (NaN where no member was added), ``count`` [P][T_out][D][2]; with layers ``lnK_eff_{mean,std}``, ``K_eff_geomean``
    and ``K_eff_count`` [P][T_out][L]; ``rows`` [T_out] and ``overflow``.  The leading [P] axis is dropped for a single
    point."""
    parts = split_conductivity_table(table, P, T, D, L, stride)
    out = {}
    moments = [(name, parts["kcnt"][..., q], parts["kmom"][..., q, :]) for q, name in enumerate(("hrc", "bkg"))]
    moments += [("eff", parts["kcnt_layer"], parts["kmom_layer"])] if L else []
    for name, count, words in moments:
        mean, std = limbs_to_mean_std(count, words, PROF_SCALE_LNK)
        with np.errstate(over="ignore"):                     # (a clamped ln K of 2^10: the geometric mean is inf)
            out[f"lnK_{name}_mean"], out[f"lnK_{name}_std"], out[f"K_{name}_geomean"] = mean, std, np.exp(mean)
    out["count"] = parts["kcnt"].copy()
    if L:
        out["K_eff_count"] = parts["kcnt_layer"].copy()
    if P == 1:
        out = {k: v[0] for k, v in out.items()}
    out["rows"] = np.arange(parts["kcnt"].shape[1], dtype=np.int64) * int(stride)
    out["overflow"] = int(parts["ovf"][0])
    return out


def layer_storage_distribution(hist, ranges, dz, levels, stride=1):
    """Quantile bands of the storage from histograms ``hist`` [..., R, L, B] of the layers' mean theta, in NumPy integers.
    Level p of a row and layer is the centre (b + 0.5) / B of the first bin b whose cumulative count reaches
    k = max(1, ceil(n p)) in fp64 -- the rank of :func:`theta_distribution`, numpy.quantile(..., method="inverted_cdf") on
    the bin index -- times the layer's thickness (i1 - i0) dz: ``quantiles_cm`` [..., R, Lv, L] (NaN where nobody was
    counted), with ``rows`` [R], ``count`` [..., R, L], ``levels`` and ``thickness_cm`` [L]."""
    hist = np.asarray(hist)
    if hist.ndim < 3:
        raise ValueError(f"histograms must be [..., R, L, B], got shape {hist.shape}")
    B = hist.shape[-1]
    r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    if B not in STORAGE_BINS or r.shape[0] != hist.shape[-2]:
        raise ValueError(f"histograms of {hist.shape[-2]} layers and {B} bins for {r.shape[0]} ranges (a power of two in 32 .. 1024 bins)")
    if hist.size and hist.min() < 0:
        raise ValueError("histogram counts must be >= 0")
    lv = np.asarray(levels, dtype=np.float64).reshape(-1)
    if lv.size > WTD_MAX_LEVELS or not np.all((lv >= 0.0) & (lv <= 1.0)):
        raise ValueError(f"at most {WTD_MAX_LEVELS} quantile levels, each in [0, 1]: got {lv.tolist()}")
    thick = (r[:, 1] - r[:, 0]).astype(np.float64) * float(dz)
    cum = np.cumsum(hist.astype(np.int64), axis=-1)                 # [..., R, L, B]
    n = cum[..., -1]                                                # [..., R, L]
    k = np.maximum(1, np.ceil(n[..., None, :].astype(np.float64) * lv[:, None]).astype(np.int64))     # [..., R, Lv, L]
    idx = (cum[..., None, :, :] < k[..., None]).sum(axis=-1)        # bins whose cumulative count stays below k
    q = np.where(n[..., None, :] > 0, (np.minimum(idx, B - 1) + 0.5) / B * thick, np.nan)
    return {"rows": np.arange(hist.shape[-3], dtype=np.int64) * int(stride), "count": n, "quantiles_cm": q, "levels": lv,
            "thickness_cm": thick}


# ---- covariance of theta(z) and the water table (include/hydrocol.h hc_set_theta_cov) ---------------------------------
THETA_COV_SCALE = 20
THETA_COV_MAX_MEMBERS = 1 << 22
THETA_COV_MAX_WORDS = 1 << 30


def theta_cov_shape(D, stride):
    """(n, E, W) of a table at node stride ``stride`` on ``D`` nodes: n = ceil(D / stride) selected nodes, E = n + 1
    columns (the last is the water table), W = 1 + E + E (E + 1) / 2 words a row."""
    D, s = int(D), int(stride)
    if not 1 <= s <= D:
        raise ValueError(f"the node stride must lie in 1 .. {D}, got {s}")
    n = (D + s - 1) // s
    E = n + 1
    return n, E, 1 + E + E * (E + 1) // 2


def theta_cov_index(a, b, E):
    """Offset of entry (a, b), a <= b < E, in the packed upper triangle: a E - a (a - 1) / 2 + (b - a)."""
    return a * E - a * (a - 1) // 2 + (b - a)


def theta_cov_of(theta, wtd_idx, stride):
    """The device's table of one row restated in exact integers: ``theta`` [N][D], ``wtd_idx`` [N] -> (words [W] int64,
    outside).  q_k = rint(theta_{k s} 2^20) for the selected nodes, q_n = the water-table index; a member with a selected
    theta that is NaN, below 0 or above 1 adds nothing and is counted in ``outside``.  words = count, S1 [E], S2 packed by
    rows (:func:`theta_cov_index`)."""
    th = np.asarray(theta, dtype=np.float64)
    th = th.reshape(-1, th.shape[-1])
    n, E, W = theta_cov_shape(th.shape[1], stride)
    sel = th[:, ::int(stride)]
    with np.errstate(invalid="ignore"):
        ok = np.all((sel >= 0.0) & (sel <= 1.0), axis=1)
    q = np.empty((int(ok.sum()), E), dtype=np.int64)
    q[:, :n] = np.rint(sel[ok] * float(1 << THETA_COV_SCALE)).astype(np.int64)
    q[:, n] = np.asarray(wtd_idx, dtype=np.int64).reshape(-1)[ok]
    if q.shape[0] > THETA_COV_MAX_MEMBERS:
        raise ValueError(f"{q.shape[0]} members exceed 2^22: the sums of products would leave an int64")
    words = np.zeros(W, dtype=np.int64)
    words[0] = q.shape[0]
    words[1:1 + E] = q.sum(axis=0)
    S2 = q.T @ q                             # int64 matmul: exact, every sum is below 2^62
    iu = np.triu_indices(E)
    words[1 + E:] = S2[iu]                   # row-major upper triangle = the packed order
    return words, int((~ok).sum())


def theta_cov_finish(table, dz, stride, D):
    """Population covariances from table rows ``table`` [..., W] (:func:`theta_cov_of`'s words): for a row of count c >= 1,
    cov_ab = (c S2_ab - S1_a S1_b) / c^2 with the numerator formed in exact integers, scaled by 2^-20 per theta factor and
    ``dz`` per water-table factor.  Returns ``count`` [...], ``theta_mean`` [..., n], ``wtd_mean_idx`` [...] (node units),
    ``theta_cov`` [..., n, n] (symmetric), ``wtd_theta_cov_cm`` [..., n], ``wtd_var_cm2`` [...], ``theta_wtd_corr`` [..., n]
    and ``theta_corr`` [..., n, n]; NaN where c = 0, correlations NaN where a variance is 0.

    The numerator: with the integer r_a = S1_a mod c (0 <= r_a < c <= 2^22) and m_a = S1_a div c,
    c S2_ab - S1_a S1_b = c (S2_ab - m_a S1_b - r_a m_b) - r_a r_b: the sum of squares about the integer mean.  It is
    below 2^63 in magnitude (c^2 times a covariance of at most 2^40), so the wrap-around int64 products give it exactly."""
    t = np.asarray(table, dtype=np.int64)
    n, E, W = theta_cov_shape(D, stride)
    if t.shape[-1] != W:
        raise ValueError(f"theta covariance rows of {t.shape[-1]} words, the layout has {W}")
    lead = t.shape[:-1]
    t = t.reshape(-1, W)
    c = t[:, 0]
    S1 = t[:, 1:1 + E]
    iu = np.triu_indices(E)
    cs = np.maximum(c, 1)[:, None]
    m, r = S1 // cs, S1 % cs
    with np.errstate(over="ignore"):
        z = t[:, 1 + E:] - m[:, iu[0]] * S1[:, iu[1]] - r[:, iu[0]] * m[:, iu[1]]      # (wraps cancel: |z| < 2^62 + 2^42)
    lo = z & 0xFFFFFFFF
    low = cs * lo - r[:, iu[0]] * r[:, iu[1]]                  # |low| < 2^54
    hi = cs * (z >> 32) + (low >> 32)                         # |hi| < 2^53: exact as a double
    num = hi.astype(np.float64) * 4294967296.0 + (low & 0xFFFFFFFF).astype(np.float64)     # two exact terms: one rounding
    scale = np.full(E, 2.0 ** -THETA_COV_SCALE)
    scale[n] = float(dz)
    cf = c.astype(np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        packed = np.where(cf > 0, num / (cf * cf), np.nan) * (scale[iu[0]] * scale[iu[1]])
        mean = np.where(cf > 0, S1 / cf, np.nan)
    full = np.empty((t.shape[0], E, E))
    full[:, iu[0], iu[1]] = packed
    full[:, iu[1], iu[0]] = packed
    var = np.einsum("rii->ri", full)
    with np.errstate(divide="ignore", invalid="ignore"):
        vv = var[:, :, None] * var[:, None, :]                 # (the root of a square is exact: a diagonal of ones)
        corr = np.where((var[:, :, None] > 0) & (var[:, None, :] > 0), full / np.sqrt(vv), np.nan)
    out = {"count": c.copy(), "theta_mean": mean[:, :n] * 2.0 ** -THETA_COV_SCALE, "wtd_mean_idx": mean[:, n],
           "theta_cov": full[:, :n, :n], "wtd_theta_cov_cm": full[:, :n, n], "wtd_var_cm2": full[:, n, n],
           "theta_wtd_corr": corr[:, :n, n], "theta_corr": corr[:, :n, :n]}
    return {k: v.reshape(lead + v.shape[1:]) for k, v in out.items()}


def theta_sensor_gain(fin, sigma):
    """cov(theta_i, wtd)^2 / ((var theta_i + sigma^2) var wtd) per row and selected node from :func:`theta_cov_finish`'s
    arrays: the fraction of the water table's variance one probe of error ``sigma`` [m3/m3] at that node removes in a linear
    update.  NaN where var wtd = 0."""
    var_t = np.einsum("...ii->...i", fin["theta_cov"])
    vw = fin["wtd_var_cm2"][..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(vw > 0, fin["wtd_theta_cov_cm"] ** 2 / ((var_t + float(sigma) ** 2) * vw), np.nan)


# ---- period totals per member (include/hydrocol.h hc_set_period_totals) ------------------------------------------------
PERIOD_MAX_PERIODS = 4096
PERIOD_MAX_ROWS = 1 << 20
PERIOD_MAX_THRESHOLDS = 4
PERIOD_WTD_NONE = 65535
PERIOD_FLUX_SHIFT = 12                   # flux totals enter the moments as A >> 12: units of 2^-20 cm
PERIOD_SCALE_TOTAL = PROF_SCALE_FLUX - PERIOD_FLUX_SHIFT


def flux_max_log2_of(max_cm):
    """e of a flux histogram's upper end ``max_cm`` = 2^e cm, e an integer in -8 .. 12; anything else is a ValueError."""
    v = float(max_cm)
    m, e = np.frexp(v) if np.isfinite(v) and v > 0 else (0.0, 0)
    if m != 0.5 or not -8 <= int(e) - 1 <= 12:
        raise ValueError(f"a flux histogram's upper end is a power of two in 2^-8 .. 2^12 cm, got {max_cm!r}")
    return int(e) - 1


def period_ends(T, rows=None, datenum=None, calendar=None):
    """The inclusive end rows of the periods of a record of ``T`` forcing rows (row 0 is the initial state; period 0
    starts at row 1).  ``rows=n``: every n-th row, n, 2 n, ... below T (rows after the last end belong to no period).
    ``datenum=`` the record's Datenum [T] (days, 719529 = 1970-01-01) with ``calendar="month"`` or ``"year"``: the last
    row of every calendar month or year -- row r >= 1 whose successor lies in another one; the record's last row counts
    when one more time step would leave its month or year."""
    T = int(T)
    if (rows is None) == (calendar is None):
        raise ValueError("exactly one of rows= and calendar=")
    if rows is not None:
        rows = int(rows)
        if not 1 <= rows <= PERIOD_MAX_ROWS:
            raise ValueError(f"a period holds 1 to {PERIOD_MAX_ROWS} rows, got {rows}")
        return np.arange(rows, T, rows, dtype=np.int64)
    if calendar not in ("month", "year"):
        raise ValueError(f"calendar is \"month\" or \"year\", got {calendar!r}")
    dn = np.asarray(datenum, dtype=np.float64).reshape(-1)
    if dn.size != T or T < 2 or not np.all(np.isfinite(dn)) or np.any(np.diff(dn) <= 0):
        raise ValueError(f"calendar periods need the record's {T} ascending Datenum values")
    dn = np.append(dn, dn[-1] + (dn[-1] - dn[-2]))
    days = np.floor(dn + 1e-6).astype(np.int64) - 719529
    key = days.astype("datetime64[D]").astype("datetime64[M]" if calendar == "month" else "datetime64[Y]").astype(np.int64)
    r = np.flatnonzero(key[:-1] != key[1:])
    return r[r >= 1].astype(np.int64)


def _check_period_ends(ends, T=None):
    e = np.asarray(ends, dtype=np.int64).reshape(-1)
    if not 1 <= e.size <= PERIOD_MAX_PERIODS:
        raise ValueError(f"1 to {PERIOD_MAX_PERIODS} periods, got {e.size}")
    if e[0] < 1 or np.any(np.diff(e) <= 0) or (T is not None and e[-1] >= T):
        raise ValueError("period end rows ascend strictly within [1, n_rows)")
    if np.any(np.diff(np.concatenate([[0], e])) > PERIOD_MAX_ROWS):
        raise ValueError(f"a period holds at most {PERIOD_MAX_ROWS} rows")
    return e


def period_solved_rows(wtd_obs, ends):
    """Rows of every period that are solved (wtd_obs >= 0): [n_period] int64."""
    e = _check_period_ends(ends)
    solved = np.concatenate([[0], np.cumsum(np.asarray(wtd_obs)[1:e[-1] + 1] >= 0)]).astype(np.int64)     # solved rows in [1, r]
    return np.diff(np.concatenate([[0], solved[e]]))


def period_totals_table_layout(P, n_period, K):
    """{part: (offset, shape)} of the int64 table: pmom [P][n_period][K][5], pcnt [P][n_period], ovf [1]."""
    return diag_layout("period", diag_counts(P, periods=n_period, thresholds=K - 4))


def split_period_totals_table(table, P, n_period, K):
    """Views of the parts of a flat moments table (see :func:`period_totals_table_layout`)."""
    return split_diag("period", table, diag_counts(P, periods=n_period, thresholds=K - 4))


def split_period_hist(entries, P, n_period, B, D):
    """(phist_flux [P][n_period][2][B], phist_wtd [P][n_period][2][D]) of the histogram table without its two last entries."""
    parts = _diag_views("period_hist", entries, diag_counts(P, D=D, periods=n_period, period_bins=B))
    return parts["flux"], parts["wtd"]


def period_totals_of(diag_rows, wtd_rows, wtd_obs, ends, threshold_nodes=(), bins=0, flux_max_log2=(0, 0), ancestors=None,
                     D=None, row_begin=1, acc=None):
    """The device's period totals of one point restated in NumPy integers.  ``diag_rows`` [R][N][2] and ``wtd_rows``
    [R][N] are what the launches stored for forcing rows row_begin ... row_begin + R - 1, ``wtd_obs`` [T] the forcing's.
    ``ancestors`` {row: anc [N]}: the particle filter's resampling after that row (after the row's reduction).  ``acc``
    [K][N]: the accumulators to start from (default: reset).  Returns ``acc`` [K][N] as they stand after the last row,
    ``acc_at_end`` [n_period][K][N] (each period's before its reset; reset values where the end was not reached),
    ``table`` (flat int64: pmom [1][n_period][K][5], pcnt, ovf), ``hist_flux`` [n_period][2][bins] and ``hist_wtd``
    [n_period][2][D] int32 (None without bins), ``outside``, ``overflow``.  The device's tables, bit for bit."""
    diag = np.asarray(diag_rows, dtype=np.float64)
    wtd = np.asarray(wtd_rows, dtype=np.int64)
    R, N = wtd.shape
    e = _check_period_ends(ends)
    thr = np.asarray(threshold_nodes, dtype=np.int64).reshape(-1)
    if thr.size > PERIOD_MAX_THRESHOLDS:
        raise ValueError(f"at most {PERIOD_MAX_THRESHOLDS} thresholds")
    bins = int(bins)
    if bins and (bins not in STORAGE_BINS or D is None):
        raise ValueError("period histograms have a power of two in 32 .. 1024 bins and need the depth D")
    K, n_period = 4 + thr.size, e.size

    def fresh():
        a = np.zeros((K, N), dtype=np.int64)
        a[2] = PERIOD_WTD_NONE
        return a

    acc = fresh() if acc is None else np.array(acc, dtype=np.int64).reshape(K, N)
    acc_at_end = np.stack([fresh() for _ in range(n_period)])
    pmom = np.zeros((1, n_period, K, PROF_WORDS), dtype=np.int64)
    pcnt = np.zeros((1, n_period), dtype=np.int64)
    hist_flux = np.zeros((n_period, 2, bins), dtype=np.int64) if bins else None
    hist_wtd = np.zeros((n_period, 2, int(D)), dtype=np.int64) if bins else None
    ovf = outside = 0
    for r in range(R):
        row = int(row_begin) + r
        p = int(np.searchsorted(e, row, side="left"))
        if p >= n_period:
            break
        if wtd_obs[row] >= 0:
            q, bad = profile_quantise(diag[r], PROF_SCALE_FLUX)
            ovf += bad
            acc[0] += q[:, 0]
            acc[1] += q[:, 1]
            acc[2] = np.minimum(acc[2], wtd[r])
            acc[3] = np.maximum(acc[3], wtd[r])
            for j, t in enumerate(thr):
                acc[4 + j] += wtd[r] <= t
        if row == e[p]:
            acc_at_end[p] = acc
            inn = acc[2] != PERIOD_WTD_NONE
            v = acc[:, inn].copy()
            v[:2] >>= PERIOD_FLUX_SHIFT                        # floor(A / 4096): an arithmetic shift
            ovf += int((np.abs(v[:2]) > PROF_Q_MAX).sum())
            v[:2] = np.clip(v[:2], -PROF_Q_MAX, PROF_Q_MAX)
            pmom[0, p] = profile_words_of(v).astype(object).sum(axis=1).astype(np.int64) if v.shape[1] else 0
            pcnt[0, p] = v.shape[1]
            if bins:
                for q in range(2):
                    sh = 20 + int(flux_max_log2[q])
                    ok = (v[q] >= 0) & (v[q] < (1 << sh))
                    np.add.at(hist_flux[p, q], (v[q][ok] * bins) >> sh, 1)
                    okw = (v[2 + q] >= 0) & (v[2 + q] < int(D))
                    np.add.at(hist_wtd[p, q], v[2 + q][okw], 1)
                    outside += int((~ok).sum()) + int((~okw).sum())
            acc = fresh()
        if ancestors is not None and row in ancestors:
            acc = acc[:, np.asarray(ancestors[row], dtype=np.int64)]
    table = np.concatenate([pmom.reshape(-1), pcnt.reshape(-1), np.array([ovf], dtype=np.int64)])
    return {"acc": acc, "acc_at_end": acc_at_end, "table": table, "overflow": ovf, "outside": outside,
            "hist_flux": hist_flux.astype(np.int32) if bins else None, "hist_wtd": hist_wtd.astype(np.int32) if bins else None}


def period_totals_stats(table, P, ends, n_thresholds, z0, dz, wtd_obs=None):
    """The science arrays of a period-totals moments table, formed as :func:`limbs_to_mean_std` forms them (exact
    integers, rounded once): ``transpiration_{mean,std}_cm``, ``lateral_flow_{mean,std}_cm`` [P][n_period] (the members'
    totals over the period), ``wtd_shallowest_{mean,std}_cm`` and ``wtd_deepest_{mean,std}_cm`` (depth z0 + dz idx; the
    sigma is dz times the index's), ``below_rows_{mean,std}`` [P][n_period][n_thresholds] (rows with the water table at
    or above the threshold node) and, with ``wtd_obs``, ``below_fraction_mean`` (of the period's solved rows) and
    ``solved_rows`` [n_period]; ``count`` [P][n_period], ``end_rows`` and ``overflow``.  NaN where nobody was counted.
    The leading [P] axis is dropped for a single point."""
    e = _check_period_ends(ends)
    parts = split_period_totals_table(table, P, e.size, 4 + int(n_thresholds))
    cnt, w = parts["pcnt"], parts["pmom"]
    out = {}
    for k, name in enumerate(("transpiration", "lateral_flow")):
        out[name + "_mean_cm"], out[name + "_std_cm"] = limbs_to_mean_std(cnt, w[:, :, k], PERIOD_SCALE_TOTAL)
    for k, name in ((2, "wtd_shallowest"), (3, "wtd_deepest")):
        m, sd = limbs_to_mean_std(cnt, w[:, :, k], 0)
        out[name + "_mean_cm"], out[name + "_std_cm"] = float(z0) + float(dz) * m, float(dz) * sd
    out["below_rows_mean"], out["below_rows_std"] = limbs_to_mean_std(cnt[..., None], w[:, :, 4:], 0)
    solved = None if wtd_obs is None else period_solved_rows(wtd_obs, e)
    if solved is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            out["below_fraction_mean"] = np.where(solved[None, :, None] > 0,
                                                  out["below_rows_mean"] / np.maximum(solved, 1)[None, :, None], np.nan)
    out["count"] = cnt.copy()
    if P == 1:
        out = {k: v[0] for k, v in out.items()}
    if solved is not None:
        out["solved_rows"] = solved
    out["end_rows"] = e.copy()
    out["overflow"] = int(parts["ovf"][0])
    return out


def _rank_bins(hist, lv):
    """First bin whose cumulative count reaches k = max(1, ceil(n p)): hist [..., B], lv [Lv] -> (idx [..., Lv], n [...])."""
    cum = np.cumsum(np.asarray(hist).astype(np.int64), axis=-1)
    n = cum[..., -1]
    k = np.maximum(1, np.ceil(n[..., None].astype(np.float64) * lv).astype(np.int64))
    idx = (cum[..., None, :] < k[..., None]).sum(axis=-1)
    return np.minimum(idx, cum.shape[-1] - 1), n


def period_totals_distribution(hist_flux, hist_wtd, levels, flux_max_log2, z0, dz):
    """Quantiles of the members' period totals from the histograms ``hist_flux`` [..., n_period, 2, B] and ``hist_wtd``
    [..., n_period, 2, D], in NumPy integers.  Level p is the first bin b whose cumulative count reaches
    k = max(1, ceil(n p)) in fp64 -- the rank of :func:`theta_distribution`, numpy.quantile(..., method="inverted_cdf")
    on the bin index: the bin centre (b + 0.5) 2^e / B cm for the fluxes, the node depth z0 + dz b for the extremes.
    ``transpiration_quantile_cm``, ``lateral_flow_quantile_cm``, ``wtd_shallowest_quantile_cm``, ``wtd_deepest_quantile_cm``
    [..., n_period, Lv] (NaN where nobody was binned), ``count`` [..., n_period] (of the shallowest index) and ``levels``."""
    hf, hw = np.asarray(hist_flux), np.asarray(hist_wtd)
    if hf.ndim < 3 or hw.ndim < 3 or hf.shape[-2] != 2 or hw.shape[-2] != 2 or hf.shape[:-1] != hw.shape[:-1]:
        raise ValueError(f"histograms must be [..., n_period, 2, B] and [..., n_period, 2, D], got {hf.shape} and {hw.shape}")
    B = hf.shape[-1]
    if B not in STORAGE_BINS:
        raise ValueError(f"period histograms have a power of two in 32 .. 1024 bins, not {B}")
    if (hf.size and hf.min() < 0) or (hw.size and hw.min() < 0):
        raise ValueError("histogram counts must be >= 0")
    lv = np.asarray(levels, dtype=np.float64).reshape(-1)
    if lv.size > WTD_MAX_LEVELS or not np.all((lv >= 0.0) & (lv <= 1.0)):
        raise ValueError(f"at most {WTD_MAX_LEVELS} quantile levels, each in [0, 1]: got {lv.tolist()}")
    out = {"levels": lv}
    idx, n = _rank_bins(hf, lv)                                        # [..., n_period, 2, Lv]
    for q, name in enumerate(("transpiration", "lateral_flow")):
        width = 2.0 ** int(flux_max_log2[q]) / B
        out[name + "_quantile_cm"] = np.where(n[..., q, None] > 0, (idx[..., q, :] + 0.5) * width, np.nan)
    idx, n = _rank_bins(hw, lv)
    for q, name in enumerate(("wtd_shallowest", "wtd_deepest")):
        out[name + "_quantile_cm"] = np.where(n[..., q, None] > 0, float(z0) + float(dz) * idx[..., q, :], np.nan)
    out["count"] = n[..., 0]
    return out


# ---- root-water uptake by depth (include/hydrocol.h hc_set_root_uptake) -------------------------------------------------
UPTAKE_MAX_LAYERS = 8
UPTAKE_SCALE_PROFILE = 44                # u_i enters the depth profile as rint(u 2^44), in two 20-bit limbs
UPTAKE_LIMB = 20


def layer_cells(z, layers_cm):
    """Midpoint-cell ranges [L][2] = (lo, hi) of the depth layers ``layers_cm`` = [(top, bottom), ...] in cm on the node
    grid ``z`` (ascending, evenly spaced): layer l holds the midpoints i with top <= z_i + dz / 2 < bottom.  ValueError for
    more than 8 layers, for top >= bottom and for a layer that holds no midpoint."""
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    if z.size < 2:
        raise ValueError("the node grid has at least two nodes")
    zm = z[:-1] + 0.5 * (z[1] - z[0])
    layers = [tuple(float(v) for v in np.asarray(lay, dtype=np.float64).reshape(-1)) for lay in layers_cm]
    if not 1 <= len(layers) <= UPTAKE_MAX_LAYERS:
        raise ValueError(f"1 to {UPTAKE_MAX_LAYERS} uptake layers, got {len(layers)}")
    out = []
    for lay in layers:
        if len(lay) != 2 or not all(np.isfinite(lay)) or lay[0] >= lay[1]:
            raise ValueError(f"an uptake layer is (top, bottom) in cm with top < bottom, got {lay!r}")
        lo, hi = int(np.searchsorted(zm, lay[0], side="left")), int(np.searchsorted(zm, lay[1], side="left"))
        if lo >= hi:
            raise ValueError(f"uptake layer {lay!r} cm holds no midpoint of the column [{float(zm[0])!r}, {float(zm[-1])!r}] cm")
        out.append((lo, hi))
    return np.array(out, dtype=np.int32)


def _check_cells(cells, M):
    r = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
    if not 1 <= r.shape[0] <= UPTAKE_MAX_LAYERS or np.any(r[:, 0] < 0) or np.any(r[:, 0] >= r[:, 1]) or np.any(r[:, 1] > M):
        raise ValueError(f"1 to {UPTAKE_MAX_LAYERS} cell ranges [lo, hi) with 0 <= lo < hi <= {M}, got {r.tolist()}")
    return r


def root_uptake_mid_tables(cols):
    """[5][D - 1]: midpoint porosity, field capacity, wilting point, 1 / (por - wlt) (a zero denominator counts as 1) and
    root density of a ``digest.ColumnTables``, as the device holds them."""
    por, fc, wlt, root = (np.asarray(v, dtype=np.float64) for v in (cols.por_mid, cols.fc_mid, cols.wlt_mid, cols.root_mid))
    d1 = por - wlt
    return np.stack([por, fc, wlt, 1.0 / np.where(d1 == 0.0, 1.0, d1), root])


def _uptake_sum(v):
    """S of include/hydrocol.h over [N][64 R]: lane partials by ascending round from 0.0, then halving strides."""
    p = np.zeros((v.shape[0], 64))
    for r in range(v.shape[1] // 64):
        p = p + v[:, 64 * r:64 * (r + 1)]
    s = 32
    while s:
        p[:, :s] = p[:, :s] + p[:, s:2 * s]
        s //= 2
    return p[:, 0]


def _uptake_scan(v):
    """C of include/hydrocol.h over [N][64 R]: (c [N][64 R], the carry after the last round)."""
    c, carry = np.zeros_like(v), np.zeros(v.shape[0])
    for r in range(v.shape[1] // 64):
        t = v[:, 64 * r:64 * (r + 1)].copy()
        o = 1
        while o < 64:
            nxt = t.copy()
            nxt[:, o:] = t[:, o:] + t[:, :-o]
            t = nxt
            o *= 2
        c[:, 64 * r:64 * (r + 1)] = carry[:, None] + t
        carry = carry + t[:, 63]
    return c, carry


def _uptake_pad(a, C):
    a = np.asarray(a, dtype=np.float64)
    out = np.zeros(a.shape[:-1] + (C,))
    n = min(C, a.shape[-1])
    out[..., :n] = a[..., :n]
    return out


def root_uptake_of(theta_mid, tables, atm, daylight, n_root_first, n_root_int, dz, flag_et=True):
    """The device's u restated in NumPy, in its order (include/hydrocol.h hc_set_root_uptake): ``theta_mid`` [N][D - 1] (or
    [D - 1]) at the midpoints, ``tables`` [5][D - 1] (:func:`root_uptake_mid_tables`), the row's ``atm`` and ``daylight``.
    Returns u [N][D - 1] >= 0, the uptake the RHS applies (its sink is -u): cells 1 .. n_root_int normalised together, cell 0
    on its own when ``n_root_first``; zeros at night or with ET off.  Equal to the device's bits from the same theta."""
    th = np.asarray(theta_mid, dtype=np.float64)
    th = th.reshape(-1, th.shape[-1])
    N, M = th.shape
    tabs = np.asarray(tables, dtype=np.float64).reshape(5, M)
    n, dz, atm = int(n_root_int), np.float64(dz), np.float64(atm)
    u = np.zeros((N, M))
    if not (int(daylight) & 1) or not flag_et:
        return u
    with np.errstate(all="ignore"):
        if n > 0:
            C = (n + 1 + 63) // 64 * 64
            t = _uptake_pad(th, C)
            por, fc, wlt, invd1, root = _uptake_pad(tabs, C)
            i = np.arange(C)
            inn = (i >= 1) & (i <= n)
            water_k = _uptake_sum(np.where(inn, t - wlt, 0.0)) * dz
            c, carry = _uptake_scan(np.where(inn, t, 0.0))
            total = carry * dz
            total = np.where(total == 0.0, 1.0, total)
            g = np.where(np.all(~inn | (t > fc), axis=1), 0.1, 1.0)
            a1 = np.maximum(t * invd1, (c * dz) / total[:, None])
            rho = np.where(inn & (t > fc), np.abs(a1 * g[:, None]), 0.0)
            tot = _uptake_sum(rho) * dz
            tot = np.where(tot == 0.0, 1.0, tot)
            x = (rho / tot[:, None]) * root
            tot_x = _uptake_sum(x) * dz
            big = tot_x > 1.0
            xb = x / np.where(big, tot_x, 1.0)[:, None]
            x = np.where(big[:, None], xb, x)
            tot_x = np.where(big, _uptake_sum(xb) * dz, tot_x)
            ok = (water_k > 0.0) & (tot_x > 0.0)
            tr = np.where(ok, np.minimum(atm, water_k) / np.where(ok, tot_x, 1.0), 0.0)
            ui = np.where((ok & (tr != 0.0))[:, None] & inn, tr[:, None] * x, 0.0)
            u[:, :min(C, M)] = ui[:, :min(C, M)]
        if int(n_root_first) > 0:
            por, fc, wlt, invd1, root = tabs[:, 0]
            t0 = th[:, 0]
            water_k = (t0 - wlt) * dz
            local = t0 * dz
            total = np.where(local == 0.0, 1.0, local)
            a1 = np.maximum(t0 * invd1, local / total)
            rho = np.where(t0 > fc, np.abs(a1 * 0.1), 0.0)
            tot = rho * dz
            tot = np.where(tot == 0.0, 1.0, tot)
            x0 = (rho / tot) * root
            tot_x = x0 * dz
            big = tot_x > 1.0
            x0 = np.where(big, x0 / np.where(big, tot_x, 1.0), x0)
            tot_x = np.where(big, x0 * dz, tot_x)
            ok = (water_k > 0.0) & (tot_x > 0.0)
            u[:, 0] = np.where(ok, (np.minimum(atm, water_k) / np.where(ok, tot_x, 1.0)) * x0, 0.0)
    return u


def root_uptake_layer_totals(u, cells, n_root_int, dz):
    """U [N][L + 1] in cm per row from u [N][D - 1]: plane 0 every cell, plane l the cells [lo_l, hi_l), each dz times the
    sum over the cells 0 .. n_root_int in the device's order (lane partials by ascending round, halving strides)."""
    u = np.asarray(u, dtype=np.float64)
    u = u.reshape(-1, u.shape[-1])
    r = _check_cells(cells, u.shape[1])
    C = (int(n_root_int) + 1 + 63) // 64 * 64
    i = np.arange(C)
    v = np.where(i <= int(n_root_int), _uptake_pad(u, C), 0.0)
    planes = [_uptake_sum(v)] + [_uptake_sum(np.where((i >= lo) & (i < hi), v, 0.0)) for lo, hi in r]
    return np.float64(dz) * np.stack(planes, axis=1)


def root_uptake_table_layout(P, n_period, L, D):
    """{part: (offset, shape)} of the int64 table: umom [P][n_period][L + 1][5], ucnt [P][n_period], uprof
    [P][n_period][D - 1][2], ovf [1]."""
    return diag_layout("uptake", diag_counts(P, D=D, periods=n_period, uptake_layers=L))


def split_root_uptake_table(table, P, n_period, L, D):
    """Views of the parts of a flat table (see :func:`root_uptake_table_layout`)."""
    return split_diag("uptake", table, diag_counts(P, D=D, periods=n_period, uptake_layers=L))


def root_uptake_tables_of(u_rows, wtd_obs, ends, cells, n_root_int, dz, bins=0, ancestors=None, row_begin=1, acc=None,
                          solved=False, daylight=None):
    """The device's root-uptake tables of one point restated in NumPy integers.  ``u_rows`` [R][N][D - 1] is the uptake at
    the end states of forcing rows row_begin ... row_begin + R - 1 (:func:`root_uptake_of`; zeros on a night row),
    ``wtd_obs`` [T] the forcing's (a skipped row adds nothing), ``daylight`` [T] if given drops the night rows as the
    device does.  ``ancestors`` {row: anc [N]}: the particle filter's resampling after that row.  ``acc`` [L + 1][N] and
    ``solved``: the accumulators to start from and whether the running period has had a solved row (default: reset).
    Returns ``acc`` as they stand after the last row, ``solved``, ``acc_at_end`` [n_period][L + 1][N], ``table`` (flat
    int64: umom [1][n_period][L + 1][5], ucnt, uprof, ovf), ``hist`` [n_period][L][bins] int32 (None without bins),
    ``outside`` and ``overflow``.  The device's tables, bit for bit."""
    u_rows = np.asarray(u_rows, dtype=np.float64)
    R, N, M = u_rows.shape
    e = _check_period_ends(ends)
    r = _check_cells(cells, M)
    bins, n = int(bins), int(n_root_int)
    if bins and bins not in STORAGE_BINS:
        raise ValueError("share histograms have a power of two in 32 .. 1024 bins")
    L_, n_period = r.shape[0], e.size
    acc = np.zeros((L_ + 1, N), dtype=np.int64) if acc is None else np.array(acc, dtype=np.int64).reshape(L_ + 1, N)
    acc_at_end = np.zeros((n_period, L_ + 1, N), dtype=np.int64)
    umom = np.zeros((1, n_period, L_ + 1, PROF_WORDS), dtype=np.int64)
    ucnt = np.zeros((1, n_period), dtype=np.int64)
    uprof = np.zeros((1, n_period, M, 2), dtype=np.int64)
    hist = np.zeros((n_period, L_, bins), dtype=np.int64) if bins else None
    ovf = outside = 0
    solved = bool(solved)
    for k in range(R):
        row = int(row_begin) + k
        p = int(np.searchsorted(e, row, side="left"))
        if p >= n_period:
            break
        if wtd_obs[row] >= 0:
            solved = True
            if daylight is None or (int(daylight[row]) & 1):
                q, bad = profile_quantise(root_uptake_layer_totals(u_rows[k], r, n, dz), PROF_SCALE_FLUX)
                acc += q.T
                qi, bad_i = profile_quantise(u_rows[k][:, :n + 1], UPTAKE_SCALE_PROFILE)
                neg = qi < 0
                ovf += bad + bad_i + int(neg.sum())
                qi = np.where(neg, 0, qi)
                uprof[0, p, :n + 1, 0] += (qi & ((1 << UPTAKE_LIMB) - 1)).sum(axis=0)
                uprof[0, p, :n + 1, 1] += (qi >> UPTAKE_LIMB).sum(axis=0)
        if row == e[p]:
            acc_at_end[p] = acc
            if solved:
                v = acc >> PERIOD_FLUX_SHIFT                      # floor(A / 4096): an arithmetic shift
                ovf += int((np.abs(v) > PROF_Q_MAX).sum())
                v = np.clip(v, -PROF_Q_MAX, PROF_Q_MAX)
                umom[0, p] = profile_words_of(v).astype(object).sum(axis=1).astype(np.int64)
                ucnt[0, p] = N
                if bins:
                    has = v[0] > 0
                    outside += int((~has).sum())
                    for l in range(L_):
                        share = np.minimum(bins - 1, (np.maximum(v[l + 1][has], 0) * bins) // v[0][has])
                        np.add.at(hist[p, l], share, 1)
            acc = np.zeros_like(acc)
            solved = False
        if ancestors is not None and row in ancestors:
            acc = acc[:, np.asarray(ancestors[row], dtype=np.int64)]
    table = np.concatenate([umom.reshape(-1), ucnt.reshape(-1), uprof.reshape(-1), np.array([ovf], dtype=np.int64)])
    return {"acc": acc, "solved": solved, "acc_at_end": acc_at_end, "table": table, "overflow": ovf, "outside": outside,
            "hist": hist.astype(np.int32) if bins else None}


def root_uptake_stats(table, P, ends, L, D):
    """The science arrays of a root-uptake table, formed as :func:`limbs_to_mean_std` forms them (exact integers, rounded
    once): ``total_mean_cm`` / ``total_std_cm`` [P][n_period] (the members' uptake over the period, every cell),
    ``layer_mean_cm`` / ``layer_std_cm`` [P][n_period][L], ``share_of_mean`` [P][n_period][L] (layer mean over total mean;
    NaN where the total is 0), ``count`` [P][n_period]; ``end_rows`` and ``overflow``.  NaN where nobody was counted.  The
    leading [P] axis is dropped for a single point."""
    e = _check_period_ends(ends)
    parts = split_root_uptake_table(table, P, e.size, int(L), int(D))
    cnt, w = parts["ucnt"], parts["umom"]
    mean, std = limbs_to_mean_std(cnt[..., None], w, PERIOD_SCALE_TOTAL)
    out = {"total_mean_cm": mean[..., 0], "total_std_cm": std[..., 0], "layer_mean_cm": mean[..., 1:],
           "layer_std_cm": std[..., 1:], "count": cnt.copy()}
    with np.errstate(divide="ignore", invalid="ignore"):
        out["share_of_mean"] = np.where(mean[..., :1] > 0, mean[..., 1:] / mean[..., :1], np.nan)
    if P == 1:
        out = {k: v[0] for k, v in out.items()}
    out["end_rows"] = e.copy()
    out["overflow"] = int(parts["ovf"][0])
    return out


def root_uptake_profile(table, P, ends, L, D, z, fractions=(0.5, 0.9)):
    """The depth profile of a root-uptake table: ``profile`` [P][n_period][D - 1], the period's uptake per cm of depth as
    the mean over the members counted (the two limbs recombined with Python integers, divided once; NaN where nobody was
    counted), ``depth_cm`` [D - 1] the midpoints, and ``depth_quantile_cm`` [P][n_period][len(fractions)]: the depth of
    the bottom of the first cell at which the cumulative profile reaches that fraction of the period's uptake (NaN when
    there was none).  The leading [P] axis is dropped for a single point."""
    e = _check_period_ends(ends)
    parts = split_root_uptake_table(table, P, e.size, int(L), int(D))
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    dz = z[1] - z[0]
    lim = parts["uprof"].astype(object)
    s = lim[..., 0] + lim[..., 1] * (1 << UPTAKE_LIMB)                        # [P][n_period][M] exact
    cnt = parts["ucnt"]
    no = np.where(cnt > 0, cnt, 1).astype(object)[..., None]
    prof = np.asarray(s / no, dtype=np.float64) * 2.0 ** -UPTAKE_SCALE_PROFILE
    prof = np.where(cnt[..., None] > 0, prof, np.nan)
    cum = np.cumsum(s, axis=-1)                                              # Python integers: exact
    tot = cum[..., -1]
    fr = np.asarray(fractions, dtype=np.float64).reshape(-1)
    dq = np.full(cnt.shape + (fr.size,), np.nan)
    for idx in np.ndindex(*cnt.shape):
        if int(tot[idx]) > 0:
            c = np.asarray(cum[idx] / int(tot[idx]), dtype=np.float64)
            for j, f in enumerate(fr):
                dq[idx + (j,)] = z[int(np.argmax(c >= f))] + dz
    out = {"profile": prof, "depth_quantile_cm": dq}
    if P == 1:
        out = {k: v[0] for k, v in out.items()}
    out["depth_cm"] = z[:-1] + 0.5 * dz
    return out


def root_uptake_distribution(hist, levels):
    """Quantiles of each layer's share of a member's period total from the histograms ``hist`` [..., n_period, L, B], in
    NumPy integers: level p is the first bin b whose cumulative count reaches k = max(1, ceil(n p)) in fp64 -- the rank of
    :func:`theta_distribution`, numpy.quantile(..., method="inverted_cdf") on the bin index -- reported as the bin centre
    (b + 0.5) / B.  ``share_quantile`` [..., n_period, Lv, L] (NaN where nobody was binned), ``count`` [..., n_period]
    and ``levels``."""
    h = np.asarray(hist)
    if h.ndim < 3:
        raise ValueError(f"share histograms must be [..., n_period, L, B], got {h.shape}")
    B = h.shape[-1]
    if B not in STORAGE_BINS:
        raise ValueError(f"share histograms have a power of two in 32 .. 1024 bins, not {B}")
    if h.size and h.min() < 0:
        raise ValueError("histogram counts must be >= 0")
    lv = np.asarray(levels, dtype=np.float64).reshape(-1)
    if lv.size > WTD_MAX_LEVELS or not np.all((lv >= 0.0) & (lv <= 1.0)):
        raise ValueError(f"at most {WTD_MAX_LEVELS} quantile levels, each in [0, 1]: got {lv.tolist()}")
    idx, n = _rank_bins(h, lv)                                            # [..., n_period, L, Lv]
    q = np.where(n[..., None] > 0, (idx + 0.5) / B, np.nan)
    return {"levels": lv, "share_quantile": np.swapaxes(q, -1, -2), "count": n[..., 0]}


# ---- particle filter on the host (include/hydrocol.h hc_set_filter) ----------------------------------------------------
FILTER_Q_ONE = 1 << 31


def filter_slot_ranges(q_members, r):
    """[N_p] (k0, k1) slot ranges of systematic resampling with Python integers: member m (C_m = exclusive prefix sum of
    q in member order, Q = sum q) fills k in [ceil((C_m N_p - r) / Q), ceil(((C_m + q_m) N_p - r) / Q))."""
    q = [int(v) for v in q_members]
    n, Q, r = len(q), sum(q), int(r)
    out, c = [], 0
    for qm in q:
        out.append((-((r - c * n) // Q), -((r - (c + qm) * n) // Q)))
        c += qm
    return out


def filter_ancestors_of(q_members, r):
    """[N_p] ancestor of every slot (point-local member index) from :func:`filter_slot_ranges`."""
    anc = np.full(len(q_members), -1, dtype=np.int64)
    for m, (k0, k1) in enumerate(filter_slot_ranges(q_members, r)):
        anc[k0:k1] = m
    return anc


def filter_member_loglik(w, theta, obs_idx, theta_obs, dz, sigma_cm, sigma, lag_w=None, lag_obs_idx=None):
    """[N] l_m of a sensor row (include/hydrocol.h hc_set_filter_soil_moisture), the device's IEEE operations in its order:
    ``w`` [N] water-table indices, ``theta`` [N][m_s] at the present sensors' nodes, ``obs_idx`` the well's index,
    ``theta_obs`` and ``sigma`` [m_s] the present sensors' values and errors in record order.  With a window
    (hc_set_filter_window) ``lag_w`` [N][m_w] the members' indices on the present lagged rows by ascending offset and
    ``lag_obs_idx`` [m_w] the indices observed there: their terms follow the sensors'."""
    w = np.asarray(w, dtype=np.int64)
    theta = np.asarray(theta, dtype=np.float64).reshape(w.size, -1)
    theta_obs, sigma = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (theta_obs, sigma))
    t = np.float64(dz) * (w - int(obs_idx)).astype(np.float64) / np.float64(sigma_cm)
    a = t * t
    with np.errstate(under="ignore", over="ignore"):
        for i in range(theta.shape[1]):
            u = (theta[:, i] - theta_obs[i]) / sigma[i]
            a = a + u * u
        if lag_w is not None:
            lag_w = np.asarray(lag_w, dtype=np.int64).reshape(w.size, -1)
            lag_obs = np.asarray(lag_obs_idx, dtype=np.int64).reshape(-1)
            if lag_obs.size != lag_w.shape[1]:
                raise ValueError(f"{lag_w.shape[1]} lagged columns, {lag_obs.size} observed indices")
            for j in range(lag_w.shape[1]):
                tj = np.float64(dz) * (lag_w[:, j] - int(lag_obs[j])).astype(np.float64) / np.float64(sigma_cm)
                a = a + tj * tj
    return -0.5 * a


def filter_tile_sum(x):
    """The sum of ``x`` [N_p] (or of every column of [N_p][c]) in the order of the filter's sensor rows (include/hydrocol.h
    hc_set_filter_soil_moisture): tiles of 1024 consecutive members, 256 threads with 4 consecutive members each from 0.0,
    a tree of halving strides over the threads, the tiles ascending from 0.0; members past N_p add 0.0."""
    x = np.asarray(x, dtype=np.float64)
    cols = x.reshape(x.shape[0], -1)
    n_tiles = -(-cols.shape[0] // 1024)
    pad = np.zeros((n_tiles * 1024, cols.shape[1]))
    pad[:cols.shape[0]] = cols
    per = pad.reshape(n_tiles, 256, 4, -1)
    th = np.zeros((n_tiles, 256, cols.shape[1]))
    for j in range(4):
        th = th + per[:, :, j]
    o = 128
    while o:
        th[:, :o] = th[:, :o] + th[:, o:2 * o]
        o //= 2
    total = np.zeros(cols.shape[1])
    for t in range(n_tiles):
        total = total + th[t, 0]
    return total.reshape(x.shape[1:]) if x.ndim > 1 else float(total[0])


def filter_routes(ancestors, bounds):
    """The columns a sharded resampling moves (include/hydrocol.h hc_set_filter_shard), restated with NumPy:
    ``(send, recv)`` with ``send[s][d]`` = the global ids of the members shard s sends to shard d -- the distinct ancestors
    of d's slots [bounds[d], bounds[d + 1]) that lie in s's range, ascending; empty for d = s -- and ``recv[d][s]`` the
    same list seen from the receiver.  ``ancestors`` [n_global]: the global ancestor of every slot."""
    anc = np.asarray(ancestors, dtype=np.int64)
    b = [int(v) for v in bounds]
    S = len(b) - 1
    send = [[np.zeros(0, dtype=np.int64) for _ in range(S)] for _ in range(S)]
    for d in range(S):
        mine = np.unique(anc[b[d]:b[d + 1]])
        for s in range(S):
            if s != d:
                send[s][d] = mine[(mine >= b[s]) & (mine < b[s + 1])]
    recv = [[send[s][d] for s in range(S)] for d in range(S)]
    return send, recv


# ---- tempered weights on the host (include/hydrocol.h hc_set_filter_tempering) -----------------------------------------
TEMPER_STEPS = 1024
TEMPER_TRIALS = 11
TEMPER_WIDTH = 4


def filter_temper_target(ess_floor, n):
    """T = min(n, max(1, ceil(f n))), the product in fp64 as the device forms it."""
    n = int(n)
    return min(n, max(1, int(np.ceil(np.float64(ess_floor) * np.float64(n)))))


def filter_temper_ok(Q, S, T):
    """Q^2 >= T S in Python integers."""
    return int(Q) * int(Q) >= int(T) * int(S)


def filter_temper_weights(l, counted, k):
    """[n] int64 q(k) = floor(2^31 exp((k / 1024) (l - s))) of the counted entries (s = their largest l), 0 elsewhere:
    the difference and the product rounded once each."""
    l = np.asarray(l, dtype=np.float64).reshape(-1)
    counted = np.asarray(counted, dtype=bool).reshape(-1)
    q = np.zeros(l.size, dtype=np.int64)
    if counted.any():
        d = l[counted] - l[counted].max()
        a = np.float64(int(k) / TEMPER_STEPS) * d
        with np.errstate(under="ignore"):
            q[counted] = np.floor(np.float64(FILTER_Q_ONE) * np.exp(a)).astype(np.int64)
    return q


def filter_temper_of(l, counted, ess_floor, n_b=None):
    """The tempering of one point's weights restated with NumPy and Python integers: ``l`` the log-likelihoods (per
    member, or per bin with the bin counts ``n_b``), ``counted`` which of them count (a bin: n_b > 0).  Returns
    ``(k, trials, q)``: the procedure's k (beta = k / 1024), its trials ``[(k, Q_k, S_k), ...]`` in order and the weights
    q(k) [n] int64; ``(None, [], zeros)`` when nothing is counted (the row is not tempered)."""
    l = np.asarray(l, dtype=np.float64).reshape(-1)
    counted = np.asarray(counted, dtype=bool).reshape(-1)
    mult = [1] * l.size if n_b is None else [int(v) for v in np.asarray(n_b).reshape(-1)]
    n = sum(m for m, c in zip(mult, counted) if c)
    if n == 0:
        return None, [], np.zeros(l.size, dtype=np.int64)
    T = filter_temper_target(ess_floor, n)
    trials = []

    def ok(k):
        q = [int(v) for v in filter_temper_weights(l, counted, k)]
        Q = sum(m * v for m, v in zip(mult, q))
        S = sum(m * v * v for m, v in zip(mult, q))
        trials.append((k, Q, S))
        return filter_temper_ok(Q, S, T)

    k = TEMPER_STEPS
    if not ok(TEMPER_STEPS):
        lo, hi = 0, TEMPER_STEPS
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if ok(mid):
                lo = mid
            else:
                hi = mid
        k = lo
    return k, trials, filter_temper_weights(l, counted, k)


# ---- rejuvenated base vectors on the host (include/hydrocol.h hc_set_filter_rejuvenation) ------------------------------
REJUV_WIDTH = 4


def rejuvenation_discount(discount):
    """Liu & West's discount as a float: 0 (off; None too) or finite with 0.5 <= delta < 1; anything else, a bool
    included, is a ValueError."""
    from numbers import Real
    if discount is None:
        return 0.0
    if isinstance(discount, (bool, np.bool_)) or not isinstance(discount, (Real, np.floating, np.integer)):
        raise ValueError(f"filter rejuvenation = {discount!r} must be a number: 0 (off) or 0.5 <= discount < 1")
    d = float(discount)
    if d != 0.0 and not (np.isfinite(d) and 0.5 <= d < 1.0):
        raise ValueError(f"filter rejuvenation = {discount!r} must be 0 (off) or finite with 0.5 <= discount < 1")
    return d


def rejuvenation_shrinkage(discount):
    """(a, h) = ((3 delta - 1) / (2 delta), sqrt(1 - a a)) in float64, every operation rounded once."""
    d = np.float64(rejuvenation_discount(discount))
    if d == 0.0:
        raise ValueError("filter rejuvenation is off (discount 0): no shrinkage")
    a = (np.float64(3.0) * d - np.float64(1.0)) / (np.float64(2.0) * d)
    return float(a), float(np.sqrt(np.float64(1.0) - a * a))


def filter_rejuvenation_of(z, eps, discount, survivors=None):
    """The rejuvenation of ONE point's resampled base vectors ``z`` [N][D] restated in float64 NumPy (include/hydrocol.h
    hc_set_filter_rejuvenation), with the standard normals ``eps`` [N][D].  ``survivors``: the resampling's count; None
    counts the distinct rows of ``z``.  The point is rejuvenated iff 0 < survivors < N.

    Moments as differences from the first member: mean_d = z_0d + S1_d / N, s_d = sqrt(S2_d / (N - 1)) (N = 1: 0); the
    update z' = (mean + a (z - mean)) + (h s) eps; a member whose new vector has a non-finite entry keeps its vector and
    is refused.  Returns ``z`` [N][D], ``applied``, ``refused`` [N] bool, ``mean``, ``s``, ``s_after`` [D] and ``row``
    [4] = the table's entries (applied, members refused, sqrt(mean_d s_d^2) before and after; NaN when not applied)."""
    z = np.asarray(z, dtype=np.float64)
    eps = np.asarray(eps, dtype=np.float64)
    N, D = z.shape
    a, h = rejuvenation_shrinkage(discount)

    def moments(x):
        d0 = x - x[0][None, :]
        s1 = d0.sum(axis=0)
        mean = x[0] + s1 / N
        if N == 1:
            return mean, np.zeros(D)
        an = d0 - (s1 / N)[None, :]
        return mean, np.sqrt((an * an).sum(axis=0) / (N - 1))

    with np.errstate(all="ignore"):
        mean, s = moments(z)
        if survivors is None:
            survivors = np.unique(z, axis=0).shape[0]
        applied = 0 < int(survivors) < N
        refused = np.zeros(N, dtype=bool)
        out = z.copy()
        if applied:
            cand = (mean[None, :] + a * (z - mean[None, :])) + (h * s)[None, :] * eps
            refused = ~np.isfinite(cand).all(axis=1)
            out = np.where(refused[:, None], z, cand)
        s_after = moments(out)[1]
        nan = float("nan")
        row = np.array([1.0 if applied else 0.0, float(refused.sum()),
                        np.sqrt((s * s).sum() / D) if applied else nan,
                        np.sqrt((s_after * s_after).sum() / D) if applied else nan])
    return {"z": out, "applied": applied, "refused": refused, "mean": mean, "s": s, "s_after": s_after, "row": row,
            "a": a, "h": h}


def filter_summary(table, stride, sigma_cm, temper_table=None, rejuvenation_table=None):
    """The filter's record from its [..., n_arow, 4] table: ``rows`` (forcing row of every assimilated slot), ``count``,
    ``ess``, ``loglik_rows`` (the increments), ``survivors`` [..., R] over the slots any point assimilated, and ``loglik``
    [...] = the sum of the increments in row order; ``stride``, ``sigma_cm``.  With the tempering's table
    (``temper_table`` [..., n_arow, 4]) also ``beta``, ``ess_tempered``, ``ess_target`` [..., R] and ``tempered_rows``
    [...] = the rows resampled with beta < 1.  With the rejuvenation's (``rejuvenation_table`` [..., n_arow, 4]) also
    ``rejuvenated`` (0 / 1), ``rejuvenation_refused``, ``noise_std_resampled``, ``noise_std_rejuvenated`` [..., R] and
    ``rejuvenated_rows`` [...] = the rows on which the base vectors were moved."""
    t = np.asarray(table, dtype=np.float64)
    used = (t[..., 0] > 0).reshape(-1, t.shape[-2]).any(axis=0)
    slots = np.flatnonzero(used)
    sel = t[..., slots, :]
    inc = sel[..., 2]
    loglik = np.zeros(inc.shape[:-1])
    for j in range(inc.shape[-1]):                      # row order
        loglik = loglik + np.where(sel[..., j, 0] > 0, inc[..., j], 0.0)
    out = {"rows": slots.astype(np.int64) * int(stride), "count": sel[..., 0].astype(np.int64), "ess": sel[..., 1],
           "loglik_rows": inc, "survivors": np.nan_to_num(sel[..., 3]).astype(np.int64),
           "loglik": loglik if loglik.ndim else float(loglik), "stride": int(stride), "sigma_cm": float(sigma_cm)}
    if temper_table is not None:
        tt = np.asarray(temper_table, dtype=np.float64)[..., slots, :]
        tempered = (tt[..., 0] < 1.0).sum(axis=-1)
        out.update(beta=tt[..., 0], ess_tempered=tt[..., 1], ess_target=tt[..., 2],
                   tempered_rows=tempered if tempered.ndim else int(tempered))
    if rejuvenation_table is not None:
        rt = np.asarray(rejuvenation_table, dtype=np.float64)[..., slots, :]
        moved = (rt[..., 0] > 0).sum(axis=-1)
        out.update(rejuvenated=np.nan_to_num(rt[..., 0]).astype(np.int64),
                   rejuvenation_refused=np.nan_to_num(rt[..., 1]).astype(np.int64),
                   noise_std_resampled=rt[..., 2], noise_std_rejuvenated=rt[..., 3],
                   rejuvenated_rows=moved if moved.ndim else int(moved))
    return out


# ---- ensemble Kalman filter on the host (include/hydrocol.h hc_set_enkf) -----------------------------------------------
ENKF_WIDTH = 8
FILTER_WIDTH = 4                           # the particle filter's own table: count, ESS, log-likelihood increment, survivors
ENKF_METHODS = ("stochastic", "sqrt")      # hc_set_enkf_method's 0 and 1


def gaspari_cohn(r):
    """The Gaspari & Cohn (1999, eq. 4.10) fifth-order taper of r = distance / L: 1 at 0, 0 from r = 2 on, continuous
    with continuous derivatives (the device's evaluation order, float64)."""
    r = np.asarray(r, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        inner = (((-0.25 * r + 0.5) * r + 0.625) * r - 5.0 / 3.0) * r * r + 1.0
        outer = ((((r / 12.0 - 0.5) * r + 0.625) * r + 5.0 / 3.0) * r - 5.0) * r + 4.0 - 2.0 / (3.0 * r)
    out = np.where(r <= 1.0, inner, np.where(r <= 2.0, outer, 0.0))
    return out if out.ndim else float(out)


def enkf_summary(table, stride, sigma_cm, z0_cm=0.0):
    """The EnKF's record from its [..., n_arow, 8] table: ``rows`` (forcing row of every analysed slot), ``count``,
    ``prior_mean_cm``, ``prior_std_cm``, ``innovation_cm``, ``loglik_rows`` (the increments), ``post_mean_cm``,
    ``post_std_cm``, ``rejected`` [..., R] over the slots any point analysed, and ``loglik`` [...] = the sum of the
    increments in row order; the means are moved from the top node to ``z0_cm`` (the well's z[0])."""
    t = np.asarray(table, dtype=np.float64)
    used = (t[..., 0] > 0).reshape(-1, t.shape[-2]).any(axis=0)
    slots = np.flatnonzero(used)
    sel = t[..., slots, :]
    inc = sel[..., 4]
    loglik = np.zeros(inc.shape[:-1])
    for j in range(inc.shape[-1]):                      # row order
        loglik = loglik + np.where(sel[..., j, 0] > 0, inc[..., j], 0.0)
    return {"rows": slots.astype(np.int64) * int(stride), "count": sel[..., 0].astype(np.int64),
            "prior_mean_cm": sel[..., 1] + z0_cm, "prior_std_cm": sel[..., 2], "innovation_cm": sel[..., 3],
            "loglik_rows": inc, "post_mean_cm": sel[..., 5] + z0_cm, "post_std_cm": sel[..., 6],
            "rejected": np.nan_to_num(sel[..., 7]).astype(np.int64), "loglik": loglik if loglik.ndim else float(loglik),
            "stride": int(stride), "sigma_cm": float(sigma_cm)}


# ---- the noise field in the EnKF (include/hydrocol.h hc_set_enkf_noise_field) ------------------------------------------
def noise_field_relaxation(value):
    """The noise field's relaxation: a finite number in [0, 1], not a bool."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"Noise_Field relaxation = {value!r} must be a number in [0, 1]")
    a = float(value)
    if not (np.isfinite(a) and 0.0 <= a <= 1.0):
        raise ValueError(f"Noise_Field relaxation = {value!r} must be a finite number in [0, 1]")
    return a


def noise_field_settings(value, block_relaxation=0.0):
    """The ``Noise_Field`` key of an EnKF block / the ``enkf_noise_field=`` argument: None or False -> None (off); True
    -> the block's relaxation; {"Relaxation": a} (or "relaxation") -> a.  Anything else is a ValueError."""
    if value is None or value is False:
        return None
    if value is True:
        return noise_field_relaxation(block_relaxation)
    if isinstance(value, dict) and len(value) == 1 and next(iter(value)) in ("Relaxation", "relaxation"):
        return noise_field_relaxation(next(iter(value.values())))
    raise ValueError(f"Noise_Field = {value!r} must be true, false or {{\"Relaxation\": a}}")


def split_enkf_noise_table(table, D):
    """[..., n_arow, 4 D + 1] -> (stats [..., n_arow, 4, D]: prior mean, prior std, posterior mean, posterior std of
    every node's z; rejected [..., n_arow])."""
    t = np.asarray(table, dtype=np.float64)
    return t[..., :4 * D].reshape(t.shape[:-1] + (4, D)), t[..., 4 * D]


def _enkf_gains_of(x, Y, obs, sigma, zeta, dz, loc, want_sqrt, taper_x=True):
    """One point: K [D][m'] = (rho o C_xY)(rho o C_YY + R)^-1 of the columns x [N][D] against Y [N][m'], and for the
    square-root scheme the reduced gain and the mean's shift.  ``taper_x`` False: rho on C_xY is all ones (columns
    without a depth, :func:`enkf_forcing_analysis_of`); S keeps its taper."""
    N, D = x.shape
    W = Y.shape[1]
    yb = Y.mean(axis=0)
    A = Y - yb
    n1 = N - 1
    cyy = A.T @ A / n1 if N > 1 else np.zeros((W, W))
    cxy = (x - x.mean(axis=0)).T @ A / n1 if N > 1 else np.zeros((D, W))
    zt = np.concatenate([[yb[0]], np.asarray(zeta, dtype=np.float64).reshape(-1)])
    depth = np.arange(D) * float(dz)
    if loc > 0:
        rho_yy = gaspari_cohn(np.abs(zt[:, None] - zt[None, :]) / loc)
        rho_xy = gaspari_cohn(np.abs(depth[:, None] - zt[None, :]) / loc) if taper_x else np.ones((D, W))
    else:
        rho_yy, rho_xy = np.ones((W, W)), np.ones((D, W))
    R = np.asarray(sigma, dtype=np.float64) ** 2
    Lc = np.linalg.cholesky(rho_yy * cyy + np.diag(R))
    u = np.linalg.solve(Lc, (rho_xy * cxy).T)
    K = np.linalg.solve(Lc.T, u).T
    if not want_sqrt:
        return K, None, None, yb
    Kr = np.linalg.solve((Lc + np.diag(np.sqrt(R))).T, u).T
    return K, Kr, K @ (np.asarray(obs, dtype=np.float64) - yb), yb


def enkf_noise_analysis_of(psi_f, z_f, Y, obs, sigma, eps=None, zeta=(), dz=1.0, localisation_cm=0.0,
                           method="stochastic", relaxation=0.0):
    """The noise field's analysis for ONE point in float64 NumPy (include/hydrocol.h hc_set_enkf_noise_field): from the
    forecast states ``psi_f`` [N][D], base vectors ``z_f`` [N][D], observations of the members ``Y`` [N][m'] (the well's
    y first), the observed values ``obs`` and their errors ``sigma`` [m'], and for the stochastic scheme the draws ``eps``
    [N][m']; ``zeta`` [m' - 1]: the taper centres of the columns beyond the well's, cm from the top node.

    K^z = (rho o C_zY)(rho o C_YY + R)^-1; z + (obs + sigma eps - Y) K^z^T, or with "sqrt" z + shift + (Ybar - Y) Kr^T.
    A member whose psi analysis (the same formula on psi_f) has a non-finite entry keeps its z; one whose updated z has
    a non-finite entry keeps its old z and is ``rejected``.  Then the anomalies are relaxed: f_d = 1 + a (sigma_b -
    sigma_a) / sigma_a (1 where sigma_a is 0 or not finite), over every member (those that kept their z included), and
    applied to the members that took their update.

    Returns ``K`` [m'][D] (and ``Kr``, ``shift`` with "sqrt"), ``z`` [N][D] the analysed vectors, ``rejected`` and
    ``psi_rejected`` [N] bool, ``sigma_b``, ``sigma_a``, ``factor`` [D], and ``stats`` [4][D]: prior mean and std,
    posterior (relaxed) mean and std."""
    if method not in ENKF_METHODS:
        raise ValueError(f"EnKF method = {method!r} must be one of {list(ENKF_METHODS)}")
    psi_f, z_f, Y = (np.asarray(a, dtype=np.float64) for a in (psi_f, z_f, Y))
    obs, sigma = np.asarray(obs, dtype=np.float64).reshape(-1), np.asarray(sigma, dtype=np.float64).reshape(-1)
    alpha = noise_field_relaxation(relaxation)
    N, D = z_f.shape
    root = method == "sqrt"
    with np.errstate(all="ignore"):
        def increments(x):
            K, Kr, shift, yb = _enkf_gains_of(x, Y, obs, sigma, zeta, dz, float(localisation_cm), root)
            if root:
                return K, Kr, shift, shift[None, :] + (yb[None, :] - Y) @ Kr.T
            return K, None, None, ((obs[None, :] + sigma[None, :] * np.asarray(eps, dtype=np.float64)) - Y) @ K.T
        psi_rej = ~np.isfinite(psi_f + increments(psi_f)[3]).all(axis=1)
        K, Kr, shift, inc = increments(z_f)
        cand = z_f + inc
        rej = ~np.isfinite(cand).all(axis=1) & ~psi_rej
        z = np.where((rej | psi_rej)[:, None], z_f, cand)
        sb = z_f.std(axis=0, ddof=1) if N > 1 else np.zeros(D)
        sa = z.std(axis=0, ddof=1) if N > 1 else np.zeros(D)
        f = np.ones(D)
        if alpha > 0.0:
            good = (sa > 0) & np.isfinite(sa) & np.isfinite(K[0, 0])
            f = np.where(good, 1.0 + alpha * (sb - sa) / np.where(good, sa, 1.0), 1.0)
            mean = z.mean(axis=0)
            relaxed = np.where(f[None, :] == 1.0, z, mean[None, :] + f[None, :] * (z - mean[None, :]))
            keep = np.isfinite(relaxed).all(axis=1) & ~psi_rej & ~rej
            z = np.where(keep[:, None], relaxed, z)
        stats = np.stack([z_f.mean(axis=0), sb, z.mean(axis=0), z.std(axis=0, ddof=1) if N > 1 else np.zeros(D)])
    out = {"K": K.T.copy(), "z": z, "rejected": rej, "psi_rejected": psi_rej, "sigma_b": sb, "sigma_a": sa, "factor": f,
           "stats": stats}
    if root:
        out["Kr"], out["shift"] = Kr.T.copy(), shift
    return out


def enkf_noise_summary(table, stride, relaxation, D=None):
    """The noise field's record from its [..., n_arow, 4 D + 1] table, over the slots any point analysed: ``rows`` [R],
    ``noise_prior_mean``, ``noise_prior_std``, ``noise_post_mean``, ``noise_post_std`` [..., R, D], ``noise_rejected``
    [..., R], ``noise_spread_ratio`` = the mean over nodes and rows of sigma_post / sigma_prior (nodes with sigma_prior
    = 0 left out; NaN with no row), ``noise_relaxation``."""
    t = np.asarray(table, dtype=np.float64)
    D = (t.shape[-1] - 1) // 4 if D is None else int(D)
    stats, rej = split_enkf_noise_table(t, D)
    used = np.isfinite(rej).reshape(-1, t.shape[-2]).any(axis=0) if t.size else np.zeros(t.shape[-2], bool)
    slots = np.flatnonzero(used)
    sel = stats[..., slots, :, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = sel[..., 3, :] / sel[..., 1, :]
    ok = np.isfinite(ratio) & (sel[..., 1, :] > 0)
    return {"rows": slots.astype(np.int64) * int(stride), "noise_prior_mean": sel[..., 0, :],
            "noise_prior_std": sel[..., 1, :], "noise_post_mean": sel[..., 2, :], "noise_post_std": sel[..., 3, :],
            "noise_rejected": np.nan_to_num(rej[..., slots]).astype(np.int64),
            "noise_spread_ratio": float(ratio[ok].mean()) if ok.any() else float("nan"),
            "noise_relaxation": float(relaxation)}


# ---- correlated noise fields (include/hydrocol.h hc_set_noise_correlation) ---------------------------------------------
def noise_correlation_length(length_cm):
    """The correlation length as a float; a ValueError unless it is a finite number > 0 (a bool is none)."""
    if isinstance(length_cm, (bool, np.bool_)) or not isinstance(length_cm, (int, float, np.integer, np.floating)):
        raise ValueError(f"noise correlation length_cm = {length_cm!r} must be a finite number > 0")
    length = float(length_cm)
    if not (np.isfinite(length) and length > 0.0):
        raise ValueError(f"noise correlation length_cm = {length_cm!r} must be a finite number > 0")
    return length


def noise_correlation_tables(z, length_cm, breaks_cm=()):
    """(a, b), each [D]: the recursion's coefficients for the exponential covariance exp(-|z_i - z_j| / length_cm) on
    the grid ``z`` -- a_i = rho_i = exp(-(z_i - z_{i-1}) / length_cm), b_i = sqrt(1 - rho_i rho_i) -- with a_0 = 0 and a
    break (a_i = 0, b_i = 1) at node i >= 1 wherever z[i-1] < L <= z[i] for an L of ``breaks_cm``: the first node at or
    below the depth, the rule of :func:`sensor_nodes`.  A break outside (z[0], z[-1]] falls on no node."""
    length = noise_correlation_length(length_cm)
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    if z.size < 1 or not np.all(np.isfinite(z)) or np.any(np.diff(z) <= 0.0):
        raise ValueError("noise correlation: z must be finite and strictly increasing")
    a, b = np.zeros(z.size), np.ones(z.size)
    rho = np.exp(-np.diff(z) / length)
    a[1:], b[1:] = rho, np.sqrt(1.0 - rho * rho)
    if np.any(a[1:] >= 1.0) or np.any(b[1:] <= 0.0):
        raise ValueError(f"noise correlation length_cm = {length_cm!r} is too long for this grid: rho rounds to 1")
    for lv in np.asarray(breaks_cm, dtype=np.float64).reshape(-1):
        if not np.isfinite(lv):
            raise ValueError(f"noise correlation break {float(lv)!r} cm is not finite")
        i = np.flatnonzero((z[:-1] < lv) & (lv <= z[1:])) + 1
        a[i], b[i] = 0.0, 1.0
    return a, b


def noise_correlate(xi, a, b):
    """The field of the white vectors ``xi`` [..., D] under the tables ``a``, ``b`` [D] (or broadcastable to xi), the
    library's recursion to the bit: z_0 = xi_0; z_i = xi_i where a_i == 0 (copied, not computed), else
    (a_i z_{i-1}) + (b_i xi_i), sequentially along the last axis."""
    xi = np.asarray(xi, dtype=np.float64)
    a = np.broadcast_to(np.asarray(a, dtype=np.float64), xi.shape)
    b = np.broadcast_to(np.asarray(b, dtype=np.float64), xi.shape)
    z = xi.copy()
    for i in range(1, xi.shape[-1]):
        step = (a[..., i] * z[..., i - 1]) + (b[..., i] * xi[..., i])
        z[..., i] = np.where(a[..., i] == 0.0, xi[..., i], step)
    return z


# ---- perturbed forcing (include/hydrocol.h hc_set_forcing_perturbation) --------------------------------------------------
FORCING_DAY_ROWS = 48


def forcing_day_of_row(row):
    """The day of forcing row ``row``: row // 48, the model's daily clock."""
    return np.asarray(row) // FORCING_DAY_ROWS


def forcing_coefficients(correlation_days):
    """(phi, c) of the AR(1) with e-folding time ``correlation_days``: phi = exp(-1 / tau), c = sqrt(1 - phi phi);
    tau = 0 gives (0, 1), white in time."""
    if isinstance(correlation_days, (bool, np.bool_)) or not isinstance(correlation_days, (int, float, np.integer, np.floating)):
        raise ValueError(f"forcing perturbation: correlation_days = {correlation_days!r} must be a finite number >= 0")
    tau = float(correlation_days)
    if not (np.isfinite(tau) and tau >= 0.0):
        raise ValueError(f"forcing perturbation: correlation_days = {correlation_days!r} must be a finite number >= 0")
    if tau == 0.0:
        return 0.0, 1.0
    phi = float(np.exp(-1.0 / tau))
    c = float(np.sqrt(1.0 - phi * phi))
    if not (phi < 1.0 and c > 0.0):
        raise ValueError(f"forcing perturbation: correlation_days = {correlation_days!r} is too long: phi rounds to 1")
    return phi, c


def forcing_recursion_of(xi, phi, c):
    """g of the normals ``xi`` [n_days, ...] (days along the FIRST axis), the library's recursion to the bit:
    g_0 = xi_0, g_k = (phi g_{k-1}) + (c xi_k)."""
    xi = np.asarray(xi, dtype=np.float64)
    phi, c = np.float64(phi), np.float64(c)
    g = xi.copy()
    for k in range(1, xi.shape[0]):
        g[k] = (phi * g[k - 1]) + (c * xi[k])
    return g


def forcing_factors_of(g, sigma):
    """exp((sigma g) - sigma^2 / 2) as NumPy evaluates it, exactly 1.0 where sigma == 0 (the library's rule; its exp may
    differ from NumPy's in the last bits)."""
    g = np.asarray(g, dtype=np.float64)
    sigma = np.float64(sigma)
    if sigma == 0.0:
        return np.ones_like(g)
    return np.exp((sigma * g) - (sigma * sigma / 2.0))


def forcing_perturbation_settings(value):
    """The ``forcing_perturbation=`` argument of EnsembleSimulation / SweepSimulation: ``None`` or
    ``{"precipitation_sigma": .., "demand_sigma": .., "correlation_days": .., "seed": ..}`` -> ``None`` or the dict
    with every key present (seed ``None``: the ensemble's).  ``"enkf_relaxation": a`` has the EnKF analyse the members'
    forcing state with relaxation ``a`` (:meth:`EnsembleStepper.set_enkf_forcing`); the key comes back only when it is
    given and not ``None``."""
    if value is None:
        return None
    if not isinstance(value, dict):
        raise ValueError(f"forcing_perturbation = {value!r} must be a dict")
    known = {"precipitation_sigma", "demand_sigma", "correlation_days", "seed", "enkf_relaxation"}
    if set(value) - known:
        raise ValueError(f"forcing_perturbation: unknown key(s) {sorted(set(value) - known)}; known: {sorted(known)}")
    if "precipitation_sigma" not in value and "demand_sigma" not in value:
        raise ValueError("forcing_perturbation needs precipitation_sigma or demand_sigma")
    out = {}
    for key in ("precipitation_sigma", "demand_sigma"):
        v = value.get(key, 0.0)
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) \
                or not np.isfinite(float(v)) or not 0.0 <= float(v) <= 1.0:
            raise ValueError(f"forcing_perturbation: {key} = {v!r} must be a finite number in [0, 1]")
        out[key] = float(v)
    tau = value.get("correlation_days", 0.0)
    forcing_coefficients(tau)
    if float(tau) > 365.0:
        raise ValueError(f"forcing_perturbation: correlation_days = {tau!r} must lie in [0, 365]")
    out["correlation_days"] = float(tau)
    seed = value.get("seed")
    if seed is not None and (isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)) or seed < 0):
        raise ValueError(f"forcing_perturbation: seed = {seed!r} must be an integer >= 0")
    out["seed"] = None if seed is None else int(seed)
    if value.get("enkf_relaxation") is not None:
        out["enkf_relaxation"] = forcing_enkf_relaxation(value["enkf_relaxation"])
    return out


# ---- the members' forcing state in the EnKF (include/hydrocol.h hc_set_enkf_forcing) --------------------------------------
ENKF_FORCING_WIDTH = 9
FORCING_STREAMS = ("precipitation", "demand")


def forcing_enkf_relaxation(value):
    """The relaxation of the forcing state's anomalies: a finite number in [0, 1], not a bool."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"the forcing analysis's relaxation = {value!r} must be a number in [0, 1]")
    a = float(value)
    if not (np.isfinite(a) and 0.0 <= a <= 1.0):
        raise ValueError(f"the forcing analysis's relaxation = {value!r} must be a finite number in [0, 1]")
    return a


def forcing_enkf_settings(value, block_relaxation=0.0):
    """The ``EnKF`` key of a ``Forcing_Perturbation`` block: None or False -> None (off); True -> the EnKF block's
    relaxation; {"Relaxation": a} -> a.  Anything else is a ValueError."""
    if value is None or value is False:
        return None
    if value is True:
        return forcing_enkf_relaxation(block_relaxation)
    if isinstance(value, dict) and set(value) - {"Relaxation"}:
        raise ValueError(f"Forcing_Perturbation.EnKF has unknown keys {sorted(set(value) - {'Relaxation'}, key=str)} "
                         f"(known: ['Relaxation'])")
    if isinstance(value, dict) and value:
        return forcing_enkf_relaxation(value["Relaxation"])
    raise ValueError(f"Forcing_Perturbation.EnKF = {value!r} must be true, false or {{\"Relaxation\": a}}")


def split_enkf_forcing_table(table):
    """[..., n_arow, 9] -> (stats [..., n_arow, 4, 2]: prior mean, prior std, posterior mean, posterior std of the two
    streams' g; rejected [..., n_arow])."""
    t = np.asarray(table, dtype=np.float64)
    return np.swapaxes(t[..., :8].reshape(t.shape[:-1] + (2, 4)), -1, -2), t[..., 8]


def enkf_forcing_analysis_of(psi_f, g_f, Y, obs, sigma, eps=None, active=(True, True), zeta=(), dz=1.0, localisation_cm=0.0,
                             method="stochastic", relaxation=0.0):
    """The forcing state's analysis for ONE point in float64 NumPy (include/hydrocol.h hc_set_enkf_forcing): from the
    forecast states ``psi_f`` [N][D], forcing states ``g_f`` [N][2] (precipitation, demand), observations of the members
    ``Y`` [N][m'] (the well's y first), the observed values ``obs`` and their errors ``sigma`` [m'], and for the stochastic
    scheme the draws ``eps`` [N][m']; ``zeta`` [m' - 1]: the taper centres of the columns beyond the well's (they shape S
    alone: C_gY is not tapered); ``active`` [2]: whether the stream is analysed (sigma_s > 0).

    K^g = C_gY (rho o C_YY + R)^-1; g + (obs + sigma eps - Y) K^g^T, or with "sqrt" g + shift + (Ybar - Y) Kr^T.  A member
    whose psi analysis has a non-finite entry keeps its g; one whose updated (g_0, g_1) has a non-finite entry keeps its
    old g and is ``rejected``.  Then the anomalies are relaxed by the noise field's rules
    (:func:`enkf_noise_analysis_of`).  A stream that is not active goes through the same arithmetic and is then put
    back: its g keeps every bit and its posterior statistics repeat the prior's.

    Returns ``K`` [m'][2] (and ``Kr``, ``shift`` with "sqrt"), ``g`` [N][2], ``rejected`` and ``psi_rejected`` [N] bool,
    ``sigma_b``, ``sigma_a``, ``factor`` [2], and ``stats`` [4][2]: prior mean and std, posterior (relaxed) mean and
    std."""
    if method not in ENKF_METHODS:
        raise ValueError(f"EnKF method = {method!r} must be one of {list(ENKF_METHODS)}")
    psi_f, g_f, Y = (np.asarray(a, dtype=np.float64) for a in (psi_f, g_f, Y))
    obs, sigma = np.asarray(obs, dtype=np.float64).reshape(-1), np.asarray(sigma, dtype=np.float64).reshape(-1)
    alpha = forcing_enkf_relaxation(relaxation)
    act = np.asarray(active, dtype=bool).reshape(2)
    N = g_f.shape[0]
    if g_f.shape != (N, 2):
        raise ValueError(f"g_f must be [N][2], got {g_f.shape}")
    root = method == "sqrt"
    with np.errstate(all="ignore"):
        def increments(x, taper_x):
            K, Kr, shift, yb = _enkf_gains_of(x, Y, obs, sigma, zeta, dz, float(localisation_cm), root, taper_x)
            if root:
                return K, Kr, shift, shift[None, :] + (yb[None, :] - Y) @ Kr.T
            return K, None, None, ((obs[None, :] + sigma[None, :] * np.asarray(eps, dtype=np.float64)) - Y) @ K.T
        psi_rej = ~np.isfinite(psi_f + increments(psi_f, True)[3]).all(axis=1)
        K, Kr, shift, inc = increments(g_f, False)
        cand = g_f + inc
        rej = ~np.isfinite(cand).all(axis=1) & ~psi_rej
        g = np.where((rej | psi_rej)[:, None], g_f, cand)
        std = (lambda a: a.std(axis=0, ddof=1)) if N > 1 else (lambda a: np.zeros(2))
        sb, sa = std(g_f), std(g)
        f = np.ones(2)
        if alpha > 0.0:
            good = (sa > 0) & np.isfinite(sa) & np.isfinite(K[0, 0])
            f = np.where(good, 1.0 + alpha * (sb - sa) / np.where(good, sa, 1.0), 1.0)
            mean = g.mean(axis=0)
            relaxed = np.where(f[None, :] == 1.0, g, mean[None, :] + f[None, :] * (g - mean[None, :]))
            keep = np.isfinite(relaxed).all(axis=1) & ~psi_rej & ~rej
            g = np.where(keep[:, None], relaxed, g)
        g = np.where(act[None, :], g, g_f)
        stats = np.stack([g_f.mean(axis=0), sb, g.mean(axis=0), std(g)])
        stats[2:] = np.where(act[None, :], stats[2:], stats[:2])
    out = {"K": K.T.copy(), "g": g, "rejected": rej, "psi_rejected": psi_rej, "sigma_b": sb, "sigma_a": sa, "factor": f,
           "stats": stats}
    if root:
        out["Kr"], out["shift"] = Kr.T.copy(), shift
    return out


def enkf_forcing_summary(table, stride, relaxation):
    """The forcing analysis's record from its [..., n_arow, 9] table, over the slots any point analysed: ``rows`` [R],
    ``forcing_prior_mean``, ``forcing_prior_std``, ``forcing_post_mean``, ``forcing_post_std`` [..., R, 2] (precipitation,
    demand), ``forcing_rejected`` [..., R], ``forcing_spread_ratio`` [2] = per stream the mean over rows (and points) of
    sigma_post / sigma_prior (entries with sigma_prior = 0 left out; NaN with none), ``forcing_relaxation``."""
    t = np.asarray(table, dtype=np.float64)
    stats, rej = split_enkf_forcing_table(t)
    used = np.isfinite(rej).reshape(-1, t.shape[-2]).any(axis=0) if t.size else np.zeros(t.shape[-2], bool)
    slots = np.flatnonzero(used)
    sel = stats[..., slots, :, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = sel[..., 3, :] / sel[..., 1, :]
    ok = np.isfinite(ratio) & (sel[..., 1, :] > 0)
    spread = np.array([float(ratio[..., s][ok[..., s]].mean()) if ok[..., s].any() else float("nan") for s in range(2)])
    return {"rows": slots.astype(np.int64) * int(stride), "forcing_prior_mean": sel[..., 0, :],
            "forcing_prior_std": sel[..., 1, :], "forcing_post_mean": sel[..., 2, :], "forcing_post_std": sel[..., 3, :],
            "forcing_rejected": np.nan_to_num(rej[..., slots]).astype(np.int64), "forcing_spread_ratio": spread,
            "forcing_relaxation": float(relaxation)}


def noise_correlation_breaks(layers, z):
    """The interfaces of ``cols.layers`` (soil, saprolite, weathered, fresh: cm) that lie inside the column ``z``: the
    saprolite's and the weathered bedrock's tops, and the soil's if it is > 0."""
    z = np.asarray(z, dtype=np.float64)
    tops = [float(layers[0]), float(layers[1]), float(layers[2])]
    return tuple(t for k, t in enumerate(tops) if (k > 0 or t > 0.0) and z[0] < t <= z[-1])


def noise_correlation_settings(value):
    """The ``noise_correlation=`` argument of EnsembleSimulation / SweepSimulation: ``None`` or
    ``{"length_cm": l, "layers": bool}`` -> ``None`` or (length_cm, layers)."""
    if value is None:
        return None
    if not isinstance(value, dict):
        raise ValueError(f"noise_correlation must be a dict {{'length_cm': ..., 'layers': ...}} or None, got {value!r}")
    unknown = sorted(set(value) - {"length_cm", "layers"})
    if unknown:
        raise ValueError(f"noise_correlation: unknown key(s) {unknown} (known: 'length_cm', 'layers')")
    if "length_cm" not in value:
        raise ValueError("noise_correlation needs 'length_cm'")
    layers = value.get("layers", False)
    if not isinstance(layers, (bool, np.bool_)):
        raise ValueError(f"noise_correlation 'layers' = {layers!r} must be true or false")
    return noise_correlation_length(value["length_cm"]), bool(layers)


# ---- soil-moisture sensors in the EnKF (include/hydrocol.h hc_set_enkf_soil_moisture) ----------------------------------
SM_WIDTH = 6
SM_MAX_SENSORS = 8


def sensor_nodes(z, depths_cm):
    """The node of every sensor depth by the reference's rule for the well (src/simulation.py:255): the first z >= depth.
    A depth outside [z[0], z[D-1]] is a ValueError."""
    z = np.asarray(z, dtype=np.float64)
    out = []
    for d in depths_cm:
        d = float(d)
        if not (np.isfinite(d) and z[0] <= d <= z[-1]):
            raise ValueError(f"sensor depth {d!r} cm lies outside the column [{float(z[0])!r}, {float(z[-1])!r}] cm")
        out.append(int(np.flatnonzero(z >= d)[0]))
    return np.array(out, dtype=np.int32)


def soil_moisture_record(z, depths_cm, values, sigma):
    """The ``enkf_soil_moisture=`` / ``filter_soil_moisture=`` argument of EnsembleSimulation / SweepSimulation: ``depths_cm`` [n] (mapped to nodes
    by :func:`sensor_nodes`), ``values`` [T][n] (NaN = none), ``sigma`` one number or [n]."""
    depths = np.asarray(depths_cm, dtype=np.float64).reshape(-1)
    sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), depths.shape).copy()
    return {"depths_cm": depths, "nodes": sensor_nodes(z, depths), "sigma": sg,
            "values": np.asarray(values, dtype=np.float64).reshape(-1, depths.size)}


def enkf_sm_summary(table, stride, sigma):
    """The sensors' record from the [..., n_arow, n, 6] table, over the slots that took a
    joint analysis at any point: ``rows`` [R], ``observed`` [..., R, n] (bool), ``obs``, ``prior_mean``, ``prior_std``,
    ``post_mean``, ``post_std`` [..., R, n]; per sensor [..., n]: ``rmse`` (forecast: the prior mean against the
    observation over the rows it was observed; NaN if never), ``mean_innovation`` (observation - prior mean), ``n_obs``;
    ``rmse_all`` [...] over every (row, sensor) observed."""
    t = np.asarray(table, dtype=np.float64)
    n = t.shape[-2]
    used = np.isfinite(t[..., 0]).reshape(-1, t.shape[-3], n).any(axis=(0, 2)) if t.size else np.zeros(t.shape[-3], bool)
    slots = np.flatnonzero(used)
    sel = t[..., slots, :, :]
    observed = sel[..., 0] == 1.0
    innov = np.where(observed, sel[..., 1] - sel[..., 2], 0.0)
    cnt = observed.sum(axis=-2)
    with np.errstate(invalid="ignore", divide="ignore"):
        rmse = np.sqrt((innov * innov).sum(axis=-2) / cnt)
        mean_innov = innov.sum(axis=-2) / cnt
        rmse_all = np.sqrt((innov * innov).sum(axis=(-2, -1)) / cnt.sum(axis=-1))
    return {"rows": slots.astype(np.int64) * int(stride), "observed": observed, "obs": sel[..., 1],
            "prior_mean": sel[..., 2], "prior_std": sel[..., 3], "post_mean": sel[..., 4], "post_std": sel[..., 5],
            "rmse": rmse, "mean_innovation": mean_innov, "n_obs": cnt.astype(np.int64),
            "rmse_all": rmse_all if np.ndim(rmse_all) else float(rmse_all), "stride": int(stride),
            "sigma": np.asarray(sigma, dtype=np.float64)}


def filter_sm_summary(table, stride, sigma):
    """The particle filter's sensor record (include/hydrocol.h hc_set_filter_soil_moisture) from its [..., n_arow, n, 6]
    table: the keys of :func:`enkf_sm_summary`, the layout being the same -- ``prior_*`` the forecast ensemble,
    ``post_*`` the resampled one, the RMSE the forecast mean's over the observed rows."""
    return enkf_sm_summary(table, stride, sigma)


# ---- the well's record inside the window (include/hydrocol.h hc_set_enkf_window) ---------------------------------------
WINDOW_WIDTH = 4


def enkf_window_settings(offsets, stride, n_sensors=0, who="EnKF", filt="the EnKF"):
    """The window's offsets as a tuple in ascending order (``()``: off).  A ValueError unless ``offsets`` is a list or
    tuple of distinct integers in [1, stride) -- no booleans, no floats -- of at most 8 entries, at most 8 together with
    ``n_sensors`` soil-moisture sensors; any offset needs the EnKF (stride > 0).  ``who`` and ``filt`` name the block and
    the filter in the messages (:func:`filter_window_settings`: the particle filter's window, the same rules)."""
    if offsets is None:
        return ()
    if not isinstance(offsets, (list, tuple)):
        raise ValueError(f"{who} Window_Offsets = {offsets!r} must be a list of integers")
    for o in offsets:
        if isinstance(o, (bool, np.bool_)) or not isinstance(o, (int, np.integer)):
            raise ValueError(f"{who} Window_Offsets: {o!r} is not an integer")
    off = tuple(sorted(int(o) for o in offsets))
    if not off:
        return ()
    stride = int(stride or 0)
    if stride <= 0:
        raise ValueError(f"{who} Window_Offsets need {filt} (Stride > 0)")
    for o in off:
        if not 1 <= o < stride:
            raise ValueError(f"{who} Window_Offsets: {o} lies outside [1, {stride}) (rows before the analysis row, below Stride)")
    if len(set(off)) != len(off):
        raise ValueError(f"{who} Window_Offsets = {list(off)} repeats an offset")
    if len(off) > SM_MAX_SENSORS:
        raise ValueError(f"{who} Window_Offsets: {len(off)} offsets, at most {SM_MAX_SENSORS}")
    if len(off) + int(n_sensors) > SM_MAX_SENSORS:
        raise ValueError(f"{who} Window_Offsets: {len(off)} offsets and {int(n_sensors)} soil-moisture sensors, at most "
                         f"{SM_MAX_SENSORS} together")
    return off


def filter_window_settings(offsets, stride, n_sensors=0):
    """:func:`enkf_window_settings` for the particle filter's window (include/hydrocol.h hc_set_filter_window)."""
    return enkf_window_settings(offsets, stride, n_sensors, who="Filter", filt="the particle filter")


def enkf_window_summary(table, stride, offsets, z0_cm=0.0):
    """The window's record from the [..., n_arow, n, 4] table, over the slots whose analysis had a lagged row at any
    point: ``rows`` [R] (the analysis rows), ``offsets`` [n], ``observed`` [..., R, n] (bool), ``obs_cm``,
    ``prior_mean_cm`` (both moved from the top node to ``z0_cm``), ``prior_std_cm``, ``innovation_cm`` [..., R, n];
    ``n_obs`` = the lagged observations assimilated (at any one point), ``n_rows`` = the analysis rows that took any."""
    t = np.asarray(table, dtype=np.float64)
    n = t.shape[-2]
    used = np.isfinite(t[..., 0]).reshape(-1, t.shape[-3], n).any(axis=(0, 2)) if t.size else np.zeros(t.shape[-3], bool)
    slots = np.flatnonzero(used)
    sel = t[..., slots, :, :]
    observed = sel[..., 0] == 1.0
    first = observed.reshape((-1,) + observed.shape[-2:])[0] if observed.size else observed.reshape(0, n)
    return {"rows": slots.astype(np.int64) * int(stride), "offsets": np.asarray(offsets, dtype=np.int64),
            "observed": observed, "obs_cm": sel[..., 1] + z0_cm, "prior_mean_cm": sel[..., 2] + z0_cm,
            "prior_std_cm": sel[..., 3], "innovation_cm": sel[..., 1] - sel[..., 2],
            "n_obs": int(first.sum()), "n_rows": int(first.any(axis=-1).sum())}


def filter_window_summary(table, stride, offsets, z0_cm=0.0):
    """The particle filter's window record from its [..., n_arow, n, 4] table: the keys of :func:`enkf_window_summary`, the
    layout being the same -- ``prior_*`` the forecast ensemble's water-table depth on the lagged row, ``n_obs`` the lagged
    observations weighed, ``n_rows`` the assimilation rows that took any."""
    return enkf_window_summary(table, stride, offsets, z0_cm)


# ---- fixed-lag smoother of the water table by ancestry (include/hydrocol.h hc_set_filter_smoother) ---------------------
SMOOTHER_MAX_LAG = 64


def filter_smoother_settings(stride, lag=0):
    """(stride, lag) of :meth:`EnsembleStepper.set_filter_smoother`, checked: integers, stride >= 0, lag in [0, 64]
    record rows."""
    for name, v in (("stride", stride), ("lag", lag)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"the smoother's {name} must be an integer, got {v!r}")
    stride, lag = int(stride), int(lag)
    if stride < 0:
        raise ValueError(f"the smoother's stride must be >= 0, got {stride}")
    if stride and not 0 <= lag <= SMOOTHER_MAX_LAG:
        raise ValueError(f"the smoother's lag must lie in [0, {SMOOTHER_MAX_LAG}] record rows, got {lag}")
    return stride, (lag if stride else 0)


def filter_smoother_config(cfg, who="filter_smoother"):
    """``{"stride": s, "lag_rows": L}`` -> (s, K = L / s), checked (L a multiple of s, K <= 64); None or stride 0: None."""
    if cfg is None:
        return None
    if not isinstance(cfg, dict) or set(cfg) - {"stride", "lag_rows"} or "stride" not in cfg:
        raise ValueError(f"{who} must be {{'stride': s, 'lag_rows': L}}, got {cfg!r}")
    stride, lag_rows = cfg["stride"], cfg.get("lag_rows", 0)
    for name, v in (("stride", stride), ("lag_rows", lag_rows)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError(f"{who}: {name} must be an integer >= 0, got {v!r}")
    stride, lag_rows = int(stride), int(lag_rows)
    if stride == 0:
        return None
    if lag_rows % stride:
        raise ValueError(f"{who}: lag_rows = {lag_rows} is not a multiple of the stride {stride}")
    return filter_smoother_settings(stride, lag_rows // stride)


def filter_smoother_of(w_rows, ancestors_by_row, stride, lag, members_per_point, D, wtd_obs, last_row):
    """The smoother's tables restated in NumPy: store, gather, emit and flush of include/hydrocol.h
    hc_set_filter_smoother, one row at a time (a launch ends on every assimilation row, so that is what the library's
    order amounts to).  ``w_rows[r]`` [N] are the members' water-table indices of forcing row r (what ``want_wtd``
    returns; read on record rows only), ``ancestors_by_row`` maps each row the filter resampled on to its ancestor table
    [N], ``wtd_obs`` [T] is the forcing's, rows 1 ... ``last_row`` have been stepped.  The distinct paths are counted
    with ``np.unique``, not by the neighbour rule the kernel relies on.  Returns ``hist`` [P][n_srow][D] int32 and
    ``paths`` [P][n_srow][2] int64 before the flush, ``hist_flushed`` and ``paths_flushed`` after it, and the ring before
    it: ``ring_w`` [K + 1][N] int32, ``ring_id`` [K + 1][N] int64, ``ring_rows`` [K + 1] (an empty plane reads 0)."""
    s, K, Np, D = int(stride), int(lag), int(members_per_point), int(D)
    obs = np.asarray(wtd_obs).reshape(-1)
    T, last_row = obs.size, int(last_row)
    N = int(np.asarray(w_rows[s]).size)                   # (the first record row)
    P, n_srow = N // Np, (T - 1) // s + 1
    hist = np.zeros((P, n_srow, D), dtype=np.int32)
    paths = np.zeros((P, n_srow, 2), dtype=np.int64)
    paths[..., 1] = -1
    ring_w, ring_id = np.zeros((K + 1, N), dtype=np.int32), np.zeros((K + 1, N), dtype=np.int64)
    ring_rows = np.full(K + 1, -1, dtype=np.int64)

    def gather(anc):
        anc = np.asarray(anc, dtype=np.int64)
        for k in np.flatnonzero(ring_rows >= 0):
            ring_w[k], ring_id[k] = ring_w[k][anc], ring_id[k][anc]

    def emit(j, cond, hist, paths, rows):
        k = j % (K + 1)
        for p in range(P):
            w, ids = ring_w[k, p * Np:(p + 1) * Np], ring_id[k, p * Np:(p + 1) * Np]
            hist[p, j] += np.bincount(w[w < D], minlength=D).astype(np.int32)
            paths[p, j] = (np.unique(ids).size, cond)
        rows[k] = -1

    for r in range(1, last_row + 1):
        anc = ancestors_by_row.get(r)
        if r % s:
            if anc is not None:
                gather(anc)
            continue
        j = r // s
        k = j % (K + 1)
        if obs[r] >= 0:
            ring_w[k] = np.asarray(w_rows[r], dtype=np.int32)
            ring_id[k] = np.arange(N, dtype=np.int64) % Np
            ring_rows[k] = r
        else:
            ring_rows[k] = -1
        if anc is not None:
            gather(anc)
        if j - K >= 1 and ring_rows[(j - K) % (K + 1)] >= 0:
            emit(j - K, r, hist, paths, ring_rows)
    live = (ring_rows >= 0)[:, None]
    out = {"hist": hist.copy(), "paths": paths.copy(), "ring_w": np.where(live, ring_w, 0),
           "ring_id": np.where(live, ring_id, 0), "ring_rows": ring_rows.copy()}
    pending = ring_rows.copy()
    for r in np.sort(pending[pending >= 0]):
        emit(int(r) // s, max(last_row, int(r)), hist, paths, pending)
    out["hist_flushed"], out["paths_flushed"] = hist, paths
    return out


def filter_smoother_summary(hist, paths, obs_idx, levels, dz, z, stride, device=0):
    """The smoothed distributions from the tables ``hist`` [..., n_srow, D] and ``paths`` [..., n_srow, 2]
    (:func:`wtd_distribution` on the histograms): its keys -- ``rows``, ``count``, ``quantile_idx``, ``quantile_cm``,
    ``crps_cm``, ``crps_mean_cm``, ``levels`` -- and ``hist``, ``lag_rows`` [..., n_srow] (the conditioning row minus the
    row: the lag the slot really got, -1 where nothing was emitted) and ``unique_paths`` [..., n_srow] (the distinct
    paths behind the histogram: towards 1 it is one trajectory, not a distribution)."""
    hist, paths = np.asarray(hist), np.asarray(paths)
    out = wtd_distribution(hist, obs_idx, levels, dz, z, device=device, stride=stride)
    emitted = paths[..., 1] >= 0
    out["hist"] = hist
    out["lag_rows"] = np.where(emitted, paths[..., 1] - out["rows"], -1).astype(np.int64)
    out["unique_paths"] = np.where(emitted, paths[..., 0], 0).astype(np.int64)
    return out


# ---- the assimilation tables (include/hydrocol.h hc_get_<key>_stats / hc_set_<key>_stats) ------------------------------
# key -> (owner, the trailing shape of one point's assimilation slot).  The key names the C entry points, the accessors
# (<key>_table / set_<key>_table), the checkpoint's dataset (<key>_table) and the CLI's placed table; "sensors", "offsets"
# and "4D+1" stand for the run's counts (:func:`assim_table_shape`).  A new table is one entry here, its two C entry
# points in _lib.EXPORTS, and the named accessors that document its columns.
ASSIM_TABLES = {
    "filter": ("filter", (FILTER_WIDTH,)),
    "filter_sm": ("filter", ("sensors", SM_WIDTH)),
    "filter_temper": ("filter", (TEMPER_WIDTH,)),
    "filter_rejuvenation": ("filter", (REJUV_WIDTH,)),
    "filter_window": ("filter", ("offsets", WINDOW_WIDTH)),
    "enkf": ("enkf", (ENKF_WIDTH,)),
    "enkf_sm": ("enkf", ("sensors", SM_WIDTH)),
    "enkf_window": ("enkf", ("offsets", WINDOW_WIDTH)),
    "enkf_noise": ("enkf", ("4D+1",)),
}


def assim_table_shape(key, D, n_sensors=0, n_offsets=0):
    """The trailing shape of the table ``key`` of ASSIM_TABLES -- what follows [P][n_arow] -- for ``D`` depth nodes and
    the owner's ``n_sensors`` soil-moisture sensors and ``n_offsets`` window offsets.  Needs no handle."""
    sizes = {"sensors": int(n_sensors), "offsets": int(n_offsets), "4D+1": 4 * int(D) + 1}
    return tuple(sizes.get(n, n) for n in ASSIM_TABLES[key][1])


# ---- the diagnostic tables (include/hydrocol.h: the accumulated integer tables of the handle) ---------------------------
# key -> one raw device table, in the order a checkpoint installs them:
#   stem     names hc_get_<stem> and, where _lib.EXPORTS has them, hc_get_<stem>_words and hc_export_<stem>
#   set      the setter (the suffixes differ: _tables, _table, none); reset: the family's reset, which zeroes all its tables
#   dtype    the element type of the raw table
#   parts    (name, shape) in table order, the shapes in the run's counts (:func:`diag_counts`).  The parts that lead with
#            "P" belong to the points: a sum over ranks places them at the points (:func:`diag_placed`).  The others are
#            global words (ovf [1]: values clamped) and are summed as they are -- or, the members' accumulators, per
#            member and not summed at all.
#   outside  how the count of values that fell in no bin follows the parts: None, "int64" (one word) or "uint64" (in the
#            last two int32 entries)
#   stored   the checkpoint's (dataset, dataset of the outside count or None, shaped): the parts flat in table order, or
#            the one part shaped, both without the outside count
# A new table is one entry here, its C entry points in _lib.EXPORTS, its counts in diag_counts, and the named accessors
# that document its columns; EnsembleStepper.diag_*, the checkpoint (_Run.diag_tables_on) and the CLI's placed table follow.
_T = namedtuple("DiagTable", "stem set reset dtype parts outside stored")
_PR, _PER = ("P", "prows"), ("P", "periods")
DIAG_TABLES = {
    "profile": _T("profile_stats", "hc_set_profile_stats_tables", "hc_reset_profile_stats", np.int64,
                  (("prof", _PR + ("D", 2, PROF_WORDS)), ("pcnt", _PR), ("flux", ("P", "T", 2, PROF_WORDS)),
                   ("fcnt", ("P", "T")), ("aerr", ("P", "T")), ("ovf", (1,))), None, ("profile_table", None, False)),
    "theta_hist": _T("theta_hist", "hc_set_theta_hist_table", "hc_reset_theta_hist", np.int32,
                     (("hist", _PR + ("D", "theta_bins")),), "uint64", ("theta_hist", "theta_hist_outside", True)),
    "storage": _T("layer_storage", "hc_set_layer_storage_tables", "hc_reset_layer_storage", np.int64,
                  (("stor", _PR + ("storage_layers", PROF_WORDS)), ("scnt", _PR), ("ovf", (1,))), None,
                  ("storage_table", None, False)),
    "storage_hist": _T("layer_storage_hist", "hc_set_layer_storage_hist_table", "hc_reset_layer_storage", np.int32,
                       (("hist", _PR + ("storage_layers", "storage_bins")),), "uint64",
                       ("storage_hist", "storage_hist_outside", True)),
    "theta_cov": _T("theta_cov", "hc_set_theta_cov_tables", "hc_reset_theta_cov", np.int64,
                    (("cov", _PR + ("cov_words",)),), "int64", ("theta_cov_table", "theta_cov_outside", True)),
    "period": _T("period_totals", "hc_set_period_totals_tables", "hc_reset_period_totals", np.int64,
                 (("pmom", _PER + ("K", PROF_WORDS)), ("pcnt", _PER), ("ovf", (1,))), None, ("period_table", None, False)),
    "period_acc": _T("period_totals_acc", "hc_set_period_totals_acc", "hc_reset_period_totals", np.int64,
                     (("acc", ("K", "N")),), None, ("period_acc", None, True)),
    "period_hist": _T("period_totals_hist", "hc_set_period_totals_hist_table", "hc_reset_period_totals", np.int32,
                      (("flux", _PER + (2, "period_bins")), ("wtd", _PER + (2, "D"))), "uint64",
                      ("period_hist", "period_hist_outside", False)),
    "uptake": _T("root_uptake", "hc_set_root_uptake_tables", "hc_reset_root_uptake", np.int64,
                 (("umom", _PER + ("uptake_layers+1", PROF_WORDS)), ("ucnt", _PER), ("uprof", _PER + ("D-1", 2)),
                  ("ovf", (1,))), None, ("uptake_table", None, False)),
    "uptake_acc": _T("root_uptake_acc", "hc_set_root_uptake_acc", "hc_reset_root_uptake", np.int64,
                     (("acc", ("uptake_layers+1", "N")),), None, ("uptake_acc", None, True)),
    "uptake_hist": _T("root_uptake_hist", "hc_set_root_uptake_hist_table", "hc_reset_root_uptake", np.int32,
                      (("hist", _PER + ("uptake_layers", "uptake_bins")),), "uint64",
                      ("uptake_hist", "uptake_hist_outside", False)),
    "wtd_hist": _T("wtd_hist", "hc_set_wtd_hist_table", "hc_reset_wtd_hist", np.int32,
                   (("hist", ("P", "hslots", "D")),), None, ("wtd_hist", None, True)),
}
# ... and the tables that joined the registry after those twelve: the same record, found by the same functions
# (:func:`diag_entry`), carried by the same path.  They stand apart because "every entry of DIAG_TABLES on at once" is the
# configuration the registry's fixtures and recorded call sequences were written for.
MORE_DIAG_TABLES = {
    "conductivity": _T("conductivity_stats", "hc_set_conductivity_stats_tables", "hc_reset_conductivity_stats", np.int64,
                       (("kmom", _PR + ("D", 2, PROF_WORDS)), ("kcnt", _PR + ("D", 2)),
                        ("kmom_layer", _PR + ("conductivity_layers", PROF_WORDS)),
                        ("kcnt_layer", _PR + ("conductivity_layers",)), ("ovf", (1,))), None,
                       ("conductivity_table", None, False)),
}


def diag_entry(key):
    """The record of the diagnostic table ``key``, of DIAG_TABLES or MORE_DIAG_TABLES (KeyError: no such table)."""
    return DIAG_TABLES[key] if key in DIAG_TABLES else MORE_DIAG_TABLES[key]


def diag_keys():
    """Every diagnostic table's key, in the order a checkpoint installs them."""
    return tuple(DIAG_TABLES) + tuple(MORE_DIAG_TABLES)


def diag_counts(P, T=1, D=1, N=0, profile_stride=0, wtd_hist_stride=0, theta_bins=0, storage_layers=0, storage_bins=0,
                cov_stride=0, periods=0, thresholds=0, period_bins=0, uptake_layers=0, uptake_bins=0, conductivity_layers=0):
    """The counts the shapes of DIAG_TABLES are written in, from a run's settings (a rank without points: ``P`` = 0).
    Needs no handle; a family that is off has no rows."""
    T, D = int(T), int(D)
    return {"P": int(P), "T": T, "D": D, "D-1": D - 1, "N": int(N),
            "prows": stride_rows(T, profile_stride) if profile_stride else 0,
            "hslots": wtd_hist_slots(T, wtd_hist_stride) if wtd_hist_stride else 0,
            "theta_bins": int(theta_bins), "storage_layers": int(storage_layers), "storage_bins": int(storage_bins),
            "cov_words": theta_cov_shape(D, cov_stride)[2] if cov_stride else 0,
            "periods": int(periods), "K": 4 + int(thresholds), "period_bins": int(period_bins),
            "uptake_layers": int(uptake_layers), "uptake_layers+1": int(uptake_layers) + 1, "uptake_bins": int(uptake_bins),
            **({"conductivity_layers": int(conductivity_layers)} if conductivity_layers else {})}


_COUNTS_ABSENT = {"conductivity_layers": 0}       # the counts :func:`diag_counts` leaves out when their option is off


def diag_placed(key):
    """The names of the table's parts that lead with [P]: what a sum over ranks places at the points."""
    return tuple(name for name, shape in diag_entry(key).parts if shape[0] == "P")


def diag_layout(key, counts, wide=False):
    """{part: (offset, shape)} of the raw table ``key`` at ``counts`` (:func:`diag_counts`), and ``words``: its elements
    with the entries the outside count takes.  ``wide``: the table as it is summed over ranks -- every element int64,
    the outside count in one word whatever its carrier.  The one place the tables' offsets come from."""
    e = diag_entry(key)
    out, off = {}, 0
    for name, shape in e.parts:
        shape = tuple((counts[n] if n in counts else _COUNTS_ABSENT[n]) if isinstance(n, str) else n for n in shape)
        out[name] = (off, shape)
        off += int(np.prod(shape))
    out["words"] = (off + (0 if e.outside is None else 1 if wide or e.outside == "int64" else 2), ())
    return out


def pack_diag(key, body, outside=0, wide=False):
    """The flat raw table of its parts' elements ``body`` and its outside count, of the entry's element type (``wide``:
    as :func:`diag_layout`).  Every table that is installed passes here: int32 counts outside [0, 2^31 - 1] and an
    outside count outside its carrier's range are refused."""
    e = diag_entry(key)
    body = np.asarray(body).reshape(-1)
    dtype = np.int64 if wide else e.dtype
    if dtype == np.int32 and body.size and (body.min() < 0 or body.max() > INT32_MAX):
        raise ValueError("histogram counts must lie in [0, 2^31 - 1]")
    if e.outside is None:
        return np.ascontiguousarray(body, dtype=dtype)
    bits = 63 if e.outside == "int64" else 64
    if not 0 <= int(outside) < 1 << bits:
        raise ValueError(f"the outside count must lie in [0, 2^{bits})")
    tail = np.array([int(outside)], dtype=np.uint64).view(np.int32)         # (the low half first, as the device holds it)
    return np.concatenate([np.ascontiguousarray(body, dtype=dtype), tail.view(dtype)])


def unpack_diag(key, raw, wide=False):
    """(the parts' elements, the outside count or None) of a flat raw table: the inverse of :func:`pack_diag`."""
    e = diag_entry(key)
    t = np.asarray(raw).reshape(-1)
    if e.outside is None:
        return t, None
    n = 1 if wide or e.dtype == np.int64 else 2
    tail = np.ascontiguousarray(t[t.size - n:], dtype=np.int64 if n == 1 else np.int32)
    return t[:t.size - n], int(tail.view(np.uint64)[0])


def _diag_views(key, body, counts):
    """{part: shaped view} of the parts' elements ``body`` (a table without its outside count)."""
    lay = diag_layout(key, counts, wide=True)
    t, n = np.asarray(body).reshape(-1), lay.pop("words")[0] - (diag_entry(key).outside is not None)
    if t.size != n:
        what = "words" if diag_entry(key).dtype == np.int64 else "entries"
        raise ValueError(f"{key} table of {t.size} {what}, the layout has {n}")
    return {k: t[o:o + int(np.prod(sh))].reshape(sh) for k, (o, sh) in lay.items()}


def split_diag(key, raw, counts, wide=False):
    """{part: shaped view} of the raw table ``key`` (the overflow word of an int64 table is its part ``ovf`` [1]), with
    ``outside`` as an integer where the entry carries one; ``wide`` as :func:`diag_layout`."""
    body, outside = unpack_diag(key, np.asarray(raw, dtype=np.int64 if wide else diag_entry(key).dtype), wide)
    out = _diag_views(key, body, counts)
    if outside is not None:
        out["outside"] = outside
    return out


def join_diag(key, parts, wide=False):
    """The flat raw table of :func:`split_diag`'s parts (``outside`` defaults to 0): its inverse."""
    body = np.concatenate([np.asarray(parts[name]).reshape(-1) for name, _ in diag_entry(key).parts])
    return pack_diag(key, body, parts.get("outside", 0), wide)


def diag_checkpoint(key, raw, counts):
    """{dataset: array} a checkpoint holds of the raw table ``key`` (the entry's ``stored``)."""
    e = diag_entry(key)
    name, outside_name, shaped = e.stored
    body, outside = unpack_diag(key, raw)
    out = {name: body.reshape(diag_layout(key, counts)[e.parts[0][0]][1]) if shaped else body}
    if outside_name is not None:
        out[outside_name] = np.array(outside, dtype=np.uint64)
    return out


def diag_from_checkpoint(key, data):
    """The raw table ``key`` of a checkpoint's datasets ``data``: the inverse of :func:`diag_checkpoint`."""
    name, outside_name, _ = diag_entry(key).stored
    return pack_diag(key, data[name], 0 if outside_name is None else int(data[outside_name]))


def _diag_ptr(t):
    return L.lptr(t) if t.dtype == np.int64 else L.iptr(t)


def allreduce_handles(steppers):
    """``hc_allreduce_moments``: one process, several devices, one stepper each -- every stepper's moment table becomes
    the sum over all of them (RCCL inside the library, no torch involved)."""
    lib = L.load()
    arr = (C.c_void_p * len(steppers))(*[st.h for st in steppers])
    L.check(lib.hc_allreduce_moments(arr, len(steppers)))

