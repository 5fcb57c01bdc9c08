"""The state bank of the "RHS as stepped" tests: named pressure-head profiles, noise vectors and forcing rows that reach
every branch on which the two instantiations of ``rhs_eval`` (include/hydrocol.h, ``hc_rhs_ex``) are written differently.

Plain NumPy, importable without a GPU.  tests/test_rhs_states_cpu.py proves on the CPU, with the oracle, that the bank
reaches what it claims to reach (a state that misses its branch hides a failure there); tests/test_gpu_rhs_as_stepped.py
runs it on the GPU.

What the states are for (csrc/hc_device.h):

* ``wt@j``  -- the deepest unsaturated midpoint is j.  The two-waves-per-SIMD kernels find it with ONE ballot: the highest
  lane that holds an unsaturated cell, then that lane's deepest cell.  j runs over lanes 0, 1, 62, 63 of every cell slot
  of every layout that serves the depth (one wave, and the two halves of a split column), the last midpoint D - 2, and
  the four nodes around a split column's cut.
* ``saturated`` (no unsaturated midpoint: the index is -1), ``unsaturated``, ``perched`` (a saturated lens over an
  unsaturated band: the deepest unsaturated cell is not the first saturated cell's neighbour).
* ``thr_exact`` / ``thr_below`` -- one midpoint at exactly psi_sat (saturated: the test is >=) and one ulp below (not).
* ``range_down`` / ``range_up`` -- |psi| log-spaced over 1e-3 ... 1e5 cm: t = 1 + sigma (1 - S_e) / m^2 of the cell model
  crosses a mantissa of 1/sqrt(2) (the log's range reduction, written as a select in one instantiation and as ldexp in
  the other) many times, and C falls below epsilon at unsaturated cells.
* ``wet_roots`` -- theta above field capacity in the whole root zone (pressure_head of the tables): transpiration with
  the "roots drowning" guard.  ``wet_top`` -- above field capacity in the top twelve cells only.
* the reference's constructed states (tests/golden/g34_states_<D>.npz) where a fixture exists.

Noise: every state has its own vector; ``range_*`` carry entries of +-6 (K_bkg = exp(sig n - ...) over its whole range).
The ``thr_*`` states keep the noise off the cells around the threshold: an unsaturated cell one ulp from saturation has
1 - S_e ~ 1e-9, known to ~1e-7 of itself, and the noise term sig n = sqrt(log t) n of K_bkg carries that into K as
~7e-12 |n| -- with it the states would test the conditioning of the formula, not the classification they are for.  ``crafted_column`` returns a copy of a column whose tables hold what no well of the site offers: cells
outside every layer (noisec < 0: K_bkg is the saturated soil's) and a root density large enough for the tot_x > 1
renormalisation of the uptake (tree_roots: the rho-weighted mean root density exceeds 1 / cm).  No well's tables hold a
zero layer-mean K, and none is crafted: the digest replaces it before the tables are made.

FINITE STATES ONLY.  One instantiation adds the root-zone terms of the evapo-transpiration sums under a mask
(``s += in_root ? x : 0``), the other as ``fma(m, x, s)`` with m = 0 / 1.  For finite x the two round alike; for a
non-finite psi OUTSIDE the root zone the masked add skips x while fma(0, inf, s) is NaN -- they legitimately differ, the
solver never hands the RHS such a state (hc_set_state refuses it), and the bank holds none.
"""
import copy

import numpy as np

WAVE = 64
PAIR_CPL = 5                      # cells per lane and half of the split column (csrc/hc_launch.h)
SPLIT_FROM = 8 * WAVE + 1         # the first depth the split-column kernel serves
LANES = (0, 1, 62, 63)


def cells_per_lane(D):
    return -(-D // WAVE)


def is_split(D):
    return D >= SPLIT_FROM


def ballot_targets(D):
    """Midpoint indices j in [1, D - 2] at which the deepest unsaturated midpoint is put (module docstring)."""
    layouts = [(cells_per_lane(D), 0)]                       # the one-wave kernel (a split column with the split off, too)
    cut = WAVE * PAIR_CPL
    if is_split(D):
        layouts += [(PAIR_CPL, 0), (PAIR_CPL, cut)]
    t = {D - 2}
    for cpl, first in layouts:
        t.update(first + lane * cpl + c for lane in LANES for c in range(cpl))
    if is_split(D):
        t.update(range(cut - 2, cut + 2))
    return sorted(j for j in t if 1 <= j <= D - 2)


def water_table_at(cols, j):
    """Deepest unsaturated midpoint exactly j: a profile that rises through zero between midpoints j and j + 1, its
    gradient away from the hydrostatic 1 (a flux K (dpsi/dz - 1) of exactly zero would hide K) and not constant."""
    i = np.arange(cols.dim_d, dtype=float)
    return cols.dz * (1.3 * (i - j - 0.75) + 0.2 * np.sin(0.37 * i))


def midpoints(y):
    return 0.5 * (y[..., :-1] + y[..., 1:])


def deepest_unsaturated(cols, y):
    """The index the kernels' water-table search returns: the deepest midpoint in [1, D - 2] below psi_sat, or -1."""
    unsat = ~(midpoints(y)[1:cols.dim_d - 1] >= cols.soil.psi_sat)
    idx = np.nonzero(unsat)[0]
    return int(idx[-1]) + 1 if idx.size else -1


def conductivity_uncertainty(cols, y, z):
    """[D - 1], per midpoint: the relative uncertainty of K that ONE rounding (2^-53) of each of its two cancelling
    intermediates leaves -- how well ANY double-precision evaluation of the formula as the reference writes it, the
    oracle's included, determines K.  Next to saturation S_e is 1 - 1e-9 or so; 1 - S_e is then known to 1e-7 of itself,
    and so is what the conductivity makes of it:
      vrettas_fung   K = S_e^lambda exp(sqrt(L) n - L / 2 + ...),  L = log(t),  t = 1 + sigma (1 - S_e) / m^2:  t is rounded
                     next to 1 as well, so dL = (1 + (sigma / m^2) / t) 2^-53 and d ln K = |n / (2 sqrt(L)) - 1/2| dL + lambda 2^-53 / S_e;
      van Genuchten  K = sqrt(S_e) (1 - u^m)^n,  u = 1 - S_e^(1/m):  du = (1 + 1/m) 2^-53 and
                     d ln K = n m u^m / (1 - u^m) du / u + 2^-53 / (2 S_e).
    First-order, with 1 - S_e evaluated without the cancellation (expm1 / log1p); 0 at saturated cells (K is the table's
    there).  `z`: the state's noise vector (midpoint j reads entry max(j - 1, 0))."""
    D, eps = cols.dim_d, 2.0 ** -53
    ym = midpoints(np.asarray(y, dtype=float))
    n_eff = np.where(cols.noisec_mid < 0.0, 0.0, cols.noisec_mid * np.asarray(z)[np.maximum(np.arange(D - 1) - 1, 0)])
    al, n, m = cols.soil.alpha, cols.soil.n, cols.soil.m
    one_minus_s = -np.expm1(-m * np.log1p((al * np.abs(ym)) ** n))
    se = 1.0 - one_minus_s
    with np.errstate(all="ignore"):
        if cols.model != 0:                                   # van Genuchten (digest.MODEL_VAN_GENUCHTEN)
            u_ = -np.expm1(np.log1p(-one_minus_s) / m)
            g = u_ ** m
            u = n * m * g / (1.0 - g) * (1.0 + 1.0 / m) * eps / u_ + 0.5 * eps / se
        else:
            mk = np.where(cols.meank_mid == 0.0, 1.0e-7, cols.meank_mid)
            x = cols.k_hc.sigma_noise / (mk * mk)
            lt = np.log1p(x * one_minus_s)
            u = np.abs(n_eff / (2.0 * np.sqrt(lt)) - 0.5) * (1.0 + x / (1.0 + x * one_minus_s)) * eps \
                + cols.k_hc.lambda_exponent * eps / se
            u = np.where(cols.noisec_mid < 0.0, cols.k_hc.lambda_exponent * eps / se, u)     # (K_bkg is the saturated soil's)
    u[~np.isfinite(u)] = np.inf                                # (S_e of exactly 1 or 0: nothing is determined)
    u[ym >= cols.soil.psi_sat] = 0.0
    return u


def threshold_node(cols):
    """Node a of the thr_* states: midpoint a is the one at the threshold, inside the root zone."""
    return max(2, min(cols.n_root_int, cols.dim_d - 4) // 2)


def state_bank(cols, golden_states=None, seed=0):
    """-> (names, Y [n][D], noise [n][D]).  `golden_states`: the arrays of g34_states_<D>.npz, where the depth has one."""
    from hydromodel_amd.ensemble import pressure_head
    D, dz, psi_sat = cols.dim_d, cols.dz, cols.soil.psi_sat
    rng = np.random.default_rng(1000 + D + seed)
    names, Y, Z = [], [], []

    def add(name, y, noise=None):
        names.append(name)
        Y.append(np.asarray(y, dtype=float))
        Z.append(rng.standard_normal(D) if noise is None else np.asarray(noise, dtype=float))

    if golden_states is not None:
        for n in golden_states["names"]:
            add(f"g34:{n}", golden_states[f"{n}_y"], golden_states["n_rnd"])
    for j in ballot_targets(D):
        add(f"wt@{j}", water_table_at(cols, j))
    add("saturated", 10.0 + 0.1 * dz * np.arange(D))
    fc_psi, _ = pressure_head(cols, 0.5 * (cols.wlt_node + cols.fc_node))
    add("unsaturated", fc_psi)
    wet_psi, _ = pressure_head(cols, np.minimum(cols.fc_node + 0.5 * (cols.por_node - cols.fc_node), 0.999 * cols.por_node))
    add("wet_roots", wet_psi)
    # wet above field capacity in the top twelve cells only, far below it underneath: the uptake weights sit where the root
    # density is largest (on crafted_column their weighted mean exceeds 1 / cm: the tot_x > 1 renormalisation)
    add("wet_top", np.where(np.arange(D) < 12, -20.0, -5000.0) - 0.5 * dz * np.arange(D))
    # perched: saturated lens at nodes [p0, p1), unsaturated band below it down to node q, saturated from there on
    p0, p1, q = D // 8, D // 8 + max(3, D // 16), (5 * D) // 8
    y = np.full(D, -80.0) - 0.3 * dz * np.arange(D)
    y[p0:p1] = 5.0 + 0.2 * dz * np.arange(p1 - p0)
    y[q:] = 2.0 + 1.2 * dz * np.arange(D - q)
    add("perched", y)
    # the threshold: nodes a and a + 1 at psi_sat -> midpoint a == psi_sat exactly (0.5 (x + x) is exact); one ulp lower next
    a = threshold_node(cols)
    pm6 = np.where(np.arange(D) % 2 == 0, 6.0, -6.0)
    for name, v in (("thr_exact", psi_sat), ("thr_below", np.nextafter(psi_sat, -np.inf))):
        y = np.full(D, -40.0) - 0.1 * dz * np.arange(D)
        y[a:a + 2] = v
        y[a + 2:] = 3.0 + 1.1 * dz * np.arange(D - a - 2)
        noise = rng.standard_normal(D)
        noise[max(a - 3, 0):a + 4] = 0.0      # (module docstring: the noise term next to saturation)
        add(name, y, noise)
    mag = np.logspace(-3.0, 5.0, D)
    add("range_down", -mag, pm6 * (np.arange(D) % 3 != 0))
    add("range_up", -mag[::-1], rng.uniform(-6.0, 6.0, D))
    return names, np.array(Y), np.array(Z)


def crafted_column(cols):
    """A copy of `cols` with cells outside every layer (noisec = -1 on two bands, one in the root zone, one below it) and a root
    density 1000 times the site's (the uptake's tot_x > 1 renormalisation is then taken).  Tables only: the copy feeds
    the oracle and the GPU tables alike.  (uptake_weight_by_cumulative_water counts the states that use the last.)"""
    c = copy.copy(cols)
    c.noisec_mid, c.noisec_node, c.root_mid = cols.noisec_mid.copy(), cols.noisec_node.copy(), cols.root_mid * 1000.0
    # wilting point and field capacity just above the residual water content: a dry profile is then still "above field
    # capacity", and theta / (por - wlt) is small enough for the CUMULATIVE water fraction to decide a cell's uptake weight
    # (tree_roots' alpha_01 = max of the two) -- with the site's tables it never does, and the masked prefix sums of theta
    # would go unobserved
    c.wlt_mid, c.fc_mid = np.full_like(cols.wlt_mid, cols.theta.res + 0.005), np.full_like(cols.fc_mid, cols.theta.res + 0.01)
    M = cols.dim_d - 1
    for lo, hi in ((3, 9), (3 * M // 4, 3 * M // 4 + 7)):
        c.noisec_mid[lo:hi] = -1.0
        c.noisec_node[lo:hi] = -1.0
    return c


# ------------------------------------------------------------------------------------------------ rows and flags
ROW_FIRST = 2       # the bank's rows overwrite forcing rows 2 ... (never row 0: the stepper refuses it as a solve target)
FLAG_SETS = {"default": None, "no_et": {"ET": False}, "no_lf": {"LF": False}, "hlift": {"HLIFT": True},
             "predict": {"PREDICT": True}}


def bank_rows(cols, forcing):
    """-> (forcing copy carrying the bank's rows, [(name, row index, spin-up flag)]).
    night / day_dry: the observed water table where the synthetic record has it; day_demand: an atmospheric demand above
    any root-zone water (the uptake is water-limited), observed water table at the bottom (lateral flow wherever the
    estimate is above it); rain: the record's heaviest rain, at night; wet: a wet-season daylight row with light rain;
    spinup: the night row with the spin-up flag (no evapo-transpiration, no hydraulic lift, no surface evaporation)."""
    from helpers import forcing_with_row
    D = cols.dim_d
    obs = int(forcing.wtd_obs[ROW_FIRST])
    spec = [("night", 0.0, float(forcing.atm.max()), 0, obs, 0),
            ("day_dry", 0.0, float(forcing.atm.max()), 1, obs, 0),
            ("day_demand", 0.0, 50.0, 1, D, 0),
            ("rain", float(forcing.precip.max()), 0.0, 0, D // 2, 0),
            ("wet", 0.1 * float(forcing.precip.max()), float(forcing.atm.max()), 1, obs, 1)]
    f, rows = forcing, []
    for k, (name, precip, atm, day, wtd_obs, wet) in enumerate(spec):
        f = forcing_with_row(f, ROW_FIRST + k, precip, atm, day, wtd_obs, wet=wet)
        rows.append((name, ROW_FIRST + k, False))
    rows.append(("spinup", ROW_FIRST, True))
    return f, rows


# ------------------------------------------------------------------------------------------------ the cases
DEPTHS_DEFAULT = (193, 200, 256, 257, 300, 320, 321, 361, 384, 385, 401, 448)    # first / interior / last depth of 4 ... 7 cells per lane
DEPTHS_SPLIT = (513, 581, 640)             # the lower half holds one node; the reference's deepest well; no padding slot
DEPTHS_GENERIC = (200, 300, 361, 581)
GENERIC = (("vanGenuchten", 2.0, 1.0), ("vrettas_fung", 1.7, 1.3))
DEPTH_PLAIN = 461                          # 8 cells per lane: two_of is false, both variants are one kernel
DEPTHS_CRAFTED = (300, 581)                # crafted_column: the bench's kernel and the split column
GOLDEN_DEPTHS = (200, 300, 401, 581)


def case_column(D, model="vrettas_fung", n=None, lam=None, crafted=False):
    """-> (cols, forcing carrying the bank's rows, rows) of one test case."""
    from hydromodel_amd.digest import ColumnTables, ForcingDigest
    from hydromodel_amd.synthetic import default_parameters, synthetic_well
    from helpers import WELLS, forcing_frame
    params = default_parameters()
    params["Hydrological_Model"]["Name"] = model
    if n is not None:
        params["Soil_Properties"]["n"] = n
        params["Hydraulic_Conductivity"]["Lambda_Exponent"] = lam
    cols = ColumnTables(params, WELLS.get(D) or synthetic_well(D))
    assert cols.dim_d == D
    if crafted:
        cols = crafted_column(cols)
    forcing, rows = bank_rows(cols, ForcingDigest(params, forcing_frame(1), cols))
    return cols, forcing, rows


def case_bank(cols):
    from helpers import golden
    D = cols.dim_d
    return state_bank(cols, golden(f"g34_states_{D}.npz") if D in GOLDEN_DEPTHS else None)


def oracle_row(forcing, row, spinup):
    from oracle.oracle import Oracle
    return Oracle.row(forcing.precip[row], forcing.atm[row], forcing.daylight[row], forcing.wtd_obs[row], spinup=spinup,
                      wet=forcing.wet_season[row])


def uptake_renormalised(cols, theta_int):
    """tree_roots' tot_x > 1 of the interior call, from theta at midpoints 1 .. D - 2: the uptake weights rho / sum(rho dz)
    times the root density integrate to the rho-weighted mean root density."""
    nr = cols.n_root_int
    if nr < 1:
        return False
    th, s = theta_int[:nr], slice(1, 1 + nr)
    wlt, fc, por, root = cols.wlt_mid[s], cols.fc_mid[s], cols.por_mid[s], cols.root_mid[s]
    if not np.sum(th - wlt) * cols.dz > 0.0:
        return False
    local = np.cumsum(th) * cols.dz
    a2 = (th > fc).astype(float)
    d1 = np.where(por - wlt == 0.0, 1.0, por - wlt)
    rho = np.abs(np.maximum(th / d1, local / (local[-1] or 1.0)) * a2 * (0.1 if a2.all() else 1.0))
    return bool(rho.sum() > 0.0 and np.sum(rho * root) / rho.sum() > 1.0)


def uptake_weight_by_cumulative_water(cols, theta_int):
    """Number of root-zone cells above field capacity whose uptake weight is the cumulative water fraction (tree_roots'
    alpha_01 = max(theta / (por - wlt), water above the cell / water in the root zone)), not the local term."""
    nr = cols.n_root_int
    th, s = theta_int[:nr], slice(1, 1 + nr)
    d1 = np.where(cols.por_mid[s] - cols.wlt_mid[s] == 0.0, 1.0, cols.por_mid[s] - cols.wlt_mid[s])
    local = np.cumsum(th)
    return int(((local / (local[-1] or 1.0) > th / d1) & (th > cols.fc_mid[s])).sum())


def coverage(cols, forcing, rows, names, Y, Z, flags=None):
    """What the bank reaches on this column, from the oracle's aux and NumPy on the midpoints (counts of states unless
    said otherwise).  Keys: sat_in_root / sat_below_root -- states with a saturated midpoint inside / below the root zone;
    lf:<row> -- states whose lateral-flow sink acts on that row; transpiring -- (state, row) pairs with transpiration > 0;
    renormalised -- states whose uptake takes the tot_x > 1 branch in daylight; c_clamped -- states with C = epsilon at
    an unsaturated midpoint; no_layer_unsat -- states with an unsaturated cell outside every layer; cumulative_weight --
    states with a cell whose uptake weight is the cumulative water fraction."""
    from oracle.oracle import Oracle
    D, psi_sat = cols.dim_d, cols.soil.psi_sat
    o = Oracle(cols, forcing.surface_evap, flags=flags)
    eps = max(cols.soil.epsilon, 1.0e-8)
    out = {"sat_in_root": 0, "sat_below_root": 0, "transpiring": 0, "renormalised": 0, "c_clamped": 0, "no_layer_unsat": 0,
           "cumulative_weight": 0}
    out.update({f"lf:{name}": 0 for name, _, _ in rows})
    for y, z in zip(Y, Z):
        ym = midpoints(y)
        sat = ym >= psi_sat
        out["sat_in_root"] += bool(sat[1:1 + cols.n_root_int].any())
        out["sat_below_root"] += bool(sat[1 + cols.n_root_int:D - 1].any())
        out["no_layer_unsat"] += bool((~sat & (cols.noisec_mid < 0.0))[1:].any())
        theta_int = o.model_eval(3, ym[1:D - 1], z)[0]
        out["renormalised"] += uptake_renormalised(cols, theta_int)
        out["cumulative_weight"] += uptake_weight_by_cumulative_water(cols, theta_int) > 0
        clamped = False
        for name, row, spin in rows:
            _, aux = o.rhs(oracle_row(forcing, row, spin), y, z, want_aux=True)
            out[f"lf:{name}"] += bool(aux["tr_lf_int"][1] > 0.0)
            out["transpiring"] += bool(aux["tr_lf_int"][0] > 0.0)
            clamped = clamped or bool(((aux["c"] == eps) & ~sat)[1:].any())
        out["c_clamped"] += clamped
    return out
