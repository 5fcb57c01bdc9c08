"""What the EnKF's depth tests need (test_gpu_enkf_depths.py) and what shows on the host that they may be trusted
(test_enkf_depths_cpu.py): one case per column slot of a wavefront (hydrocol.hip ENKF_SLOTS = HC_MAX_DEPTH_NODES / WAVE,
node c * 64 + lane in a[c]) whose observed water table sits on the boundary between two slots, the inputs of a case, the
four configurations, and the gain in np.longdouble as the arbiter of a comparison that misses the project's bar."""
from functools import lru_cache

import numpy as np

WAVE, SLOTS, MAX_D, ENKF_OBS = 64, 10, 640, 9          # hydrocol.hip WAVE, ENKF_SLOTS, HC_MAX_DEPTH_NODES, ENKF_OBS

# (D, node): node is the observed water-table index.  D = 41: one slot, nine of padding; D = 64: one full wave, and with
# m' = 1 the 128-thread block of the column sums; D = 65: a last slot of one node, and node 63 one short of the clamp
# b = 64 = D - 1, whose `lo` comes from slot 0, lane 63; D = 64 k + 1, k = 2 .. 9: the water table at node 64 (k - 1), `hi`
# from slot k - 1, lane 0 and `lo` from slot k - 2, lane 63; D = 640: no padding slot, and with m' = 9 the 704-thread block.
CASES = ((41, 20), (64, 32), (65, 63), (129, 64), (193, 128), (257, 192), (321, 256), (385, 320), (449, 384), (513, 448),
         (577, 512), (640, 576))

MPP = 100                                              # members per point
STRIDE, OFFSETS = 6, (1, 2, 3, 4)                      # the analysis on row 6, the lagged rows 5, 4, 3, 2
SENSOR_VALUES, SENSOR_SIGMAS = (0.12, 0.20, 0.26, 0.29), (0.02, 0.03, 0.015, 0.025)
SIGMA_CM, SEED = 5.0, 11

# tag: method, the full batch (well + 4 sensors + 4 lagged rows, m' = 9) or the well alone, the taper's half-width (cm),
# psi's relaxation, points, the noise field's relaxation (None: the noise field is off)
CONFIGS = {"S1": dict(method="stochastic", wide=False, loc=0.0, alpha=0.0, P=1, alpha_z=None),
           "S9": dict(method="stochastic", wide=True, loc=80.0, alpha=0.5, P=2, alpha_z=0.25),
           "R1": dict(method="sqrt", wide=False, loc=60.0, alpha=0.5, P=2, alpha_z=0.25),
           "R9": dict(method="sqrt", wide=True, loc=0.0, alpha=0.0, P=1, alpha_z=None)}


def sensor_nodes(D, node):
    """Three nodes in the unsaturated zone above the water table and the last node of the last slot, which is saturated
    in every member: that column of Y has no variance."""
    return sorted({max(node - 25, 0), node - 14, node - 6, D - 1})


def coverage_indices(D, node):
    """The find_wtd indices a case must reach: one below, on and one above the slot boundary (D = 65: 62, 63 and the
    clamp 64)."""
    return (node - 1, node, node + 1)


def cross_slot_index(D, node):
    """The covered find_wtd index b whose `hi` is lane 0 of slot b / 64 and whose `lo` is lane 63 of the slot before (None:
    the column has one slot)."""
    b = node if node % WAVE == 0 else node + 1
    return b if b % WAVE == 0 and 0 < b < D else None


@lru_cache(maxsize=None)
def _tables(D, node, n_points):
    from hydromodel_amd.digest import ColumnTables, ForcingDigest
    from hydromodel_amd.synthetic import default_parameters, synthetic_forcing_frame, synthetic_well
    params = default_parameters()
    points = [ColumnTables(params, synthetic_well(D))]
    for _ in range(1, n_points):                                      # test_gpu_enkf.digest_point_like's soil
        other = default_parameters()
        other["Soil_Properties"]["n"] = 1.7
        points.append(ColumnTables(other, synthetic_well(D)))
    forcing = ForcingDigest(params, synthetic_forcing_frame(1, wtd_m=-(node * 5.0) / 100.0), points[0])
    return points, forcing


def build(D, node, n_points=1, mpp=MPP):
    """The inputs of one case: ``points`` (the ColumnTables of every point; ``cols`` the first), ``forcing`` (the well at
    ``node`` on every row), the hydrostatic start states and the host base noise [n_points mpp][D] (every point the same
    block), the sensors' nodes, values and sigmas.  Nothing in it is changed by a test."""
    points, forcing = _tables(D, node, n_points)
    cols = points[0]
    zw = node * cols.dz + np.random.default_rng(12).uniform(-70.0, 30.0, mpp)
    psi0 = np.maximum(cols.z[None, :] - zw[:, None], -300.0)
    base = np.random.default_rng(7).standard_normal((mpp, D))
    return dict(D=D, node=node, P=n_points, mpp=mpp, N=n_points * mpp, cols=cols, points=points, forcing=forcing,
                psi0=np.tile(psi0, (n_points, 1)), base=np.tile(base, (n_points, 1)), nodes=sensor_nodes(D, node),
                values=SENSOR_VALUES, sigmas=np.array(SENSOR_SIGMAS))


def sensor_record(T, nodes, values, row=STRIDE):
    """[T][n]: NaN but on ``row``, where every sensor reads its value."""
    v = np.full((T, len(nodes)), np.nan)
    v[row] = values
    return v


def spread_members(N, count=8):
    """``count`` members spread over the ensemble, the first and the last among them."""
    return np.unique(np.linspace(0, N - 1, min(count, N)).round().astype(np.int64))


# ---- the gain in extended precision --------------------------------------------------------------------------------------
def _gaspari_cohn_long(r):
    """stepper.gaspari_cohn, every operation in np.longdouble (r a scalar)"""
    one = np.longdouble(1.0)
    r = np.longdouble(r)
    if r <= 1.0:
        return (((-r / 4 + one / 2) * r + one * 5 / 8) * r - one * 5 / 3) * r * r + one
    if r <= 2.0:
        return ((((r / 12 - one / 2) * r + one * 5 / 8) * r + one * 5 / 3) * r - 5) * r + 4 - one * 2 / (3 * r)
    return np.longdouble(0.0)


def gain_longdouble(x, Y, obs, sigma, zeta, dz, loc, want_sqrt):
    """stepper._enkf_gains_of for one point with every operation in np.longdouble and no library routine: the means, the
    anomalies and the covariances over N - 1, the taper, the Cholesky factor of S = rho o C_YY + R and the two
    substitutions as plain loops (m' <= 9).  x [N][D] (states or base vectors), Y [N][m'], obs / sigma [m'], zeta
    [m' - 1].  Returns (K [D][m'], Kr [D][m'] or None, shift [D] or None) as np.longdouble."""
    ld = np.longdouble
    x, Y = np.asarray(x, dtype=ld), np.asarray(Y, dtype=ld)
    N, D = x.shape
    W = Y.shape[1]
    assert W <= ENKF_OBS and N > 1
    obs, sigma = np.asarray(obs, dtype=ld).reshape(-1), np.asarray(sigma, dtype=ld).reshape(-1)
    yb = Y.sum(axis=0) / ld(N)
    B = Y - yb
    A = x - x.sum(axis=0) / ld(N)
    cyy, cxy = np.zeros((W, W), dtype=ld), np.zeros((D, W), dtype=ld)
    for i in range(W):
        for k in range(W):
            cyy[i, k] = (B[:, i] * B[:, k]).sum() / ld(N - 1)
        cxy[:, i] = (A * B[:, i:i + 1]).sum(axis=0) / ld(N - 1)
    zt = [yb[0]] + [ld(v) for v in np.asarray(zeta, dtype=np.float64).reshape(-1)]
    loc, dz = ld(loc), ld(dz)
    S = np.zeros((W, W), dtype=ld)
    for i in range(W):
        for k in range(W):
            rho = _gaspari_cohn_long(abs(zt[i] - zt[k]) / loc) if loc > 0 else ld(1.0)
            S[i, k] = rho * cyy[i, k] + (sigma[i] * sigma[i] if i == k else ld(0.0))
    L = np.zeros((W, W), dtype=ld)
    for j in range(W):
        d = S[j, j]
        for k in range(j):
            d = d - L[j, k] * L[j, k]
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, W):
            v = S[i, j]
            for k in range(j):
                v = v - L[i, k] * L[j, k]
            L[i, j] = v / L[j, j]
    c = cxy.copy()
    if loc > 0:
        for d in range(D):
            for i in range(W):
                c[d, i] = c[d, i] * _gaspari_cohn_long(abs(ld(d) * dz - zt[i]) / loc)
    u = np.zeros((D, W), dtype=ld)                                    # L u = c^T, every node at once
    for i in range(W):
        v = c[:, i].copy()
        for k in range(i):
            v = v - L[i, k] * u[:, k]
        u[:, i] = v / L[i, i]

    def back(diag_extra):
        """x (L + diag_extra)^T-wise: x_i = (u_i - sum_{k > i} L_ki x_k) / (L_ii + extra_i)"""
        out = np.zeros((D, W), dtype=ld)
        for i in range(W - 1, -1, -1):
            v = u[:, i].copy()
            for k in range(i + 1, W):
                v = v - L[k, i] * out[:, k]
            out[:, i] = v / (L[i, i] + diag_extra[i])
        return out

    K = back(np.zeros(W, dtype=ld))
    if not want_sqrt:
        return K, None, None
    shift = np.zeros(D, dtype=ld)
    for i in range(W):
        shift = shift + K[:, i] * (obs[i] - yb[i])
    return K, back(sigma), shift


def rel_to_largest(got, want):
    """The largest difference of two arrays relative to ``want``'s largest entry (LAB_NOTES 13), in np.longdouble"""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), np.longdouble(1e-300)))
