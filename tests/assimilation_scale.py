"""What the assimilation tests need at 263 205 members a point (test_gpu_assimilation_scale.py) and what shows on the host
that it may be trusted (test_assimilation_scale_cpu.py): the member count and its sample, vectorised forms of the restatements
that loop over the members in Python, the EnKF's references with their long sums in np.longdouble, and systematic
resampling's defining property as a check on an ancestry."""
import numpy as np

from hydromodel_amd.stepper import (FILTER_Q_ONE, TEMPER_STEPS, filter_temper_ok, filter_temper_target, filter_temper_weights,
                                    gaspari_cohn)

SCAN_TILE, SCAN_THREADS = 1024, 256           # hydrocol.hip FILT_TILE, FILT_THREADS: the prefix scan's tiles and its rounds
ENKF_TILE, ENKF_THREADS = 256, 1024           # hydrocol.hip ENKF_TILE, ENKF_THREADS: the column sums' tiles and their stride
M = SCAN_TILE * SCAN_THREADS + SCAN_TILE + 37  # 263 205: one more scan round, one more EnKF stride, a last tile of 37 members
EDGES = (0, 255, 256, 1023, 1024, 262143, 262144, 262145, M - 38, M - 37, M - 1)


def scan_tiles(n):
    return -(-int(n) // SCAN_TILE)


def enkf_tiles(n):
    return -(-int(n) // ENKF_TILE)


def sampled_members(n=M, count=256, seed=20):
    """``count`` distinct members of [0, n), ascending: the tile and round edges of EDGES that lie in the range and a seeded
    random rest."""
    edges = sorted({m for m in EDGES if 0 <= m < n})
    rest = np.setdiff1d(np.arange(n), edges)
    more = np.random.default_rng(seed).choice(rest, size=max(0, min(count, n) - len(edges)), replace=False)
    return np.sort(np.concatenate([np.asarray(edges, dtype=np.int64), more.astype(np.int64)]))


# ---- the water table of the EnKF tests, without a loop over the members ---------------------------------------------------
def find_wtd(psi, psat):
    """test_gpu_enkf._find_wtd: below the deepest node with psi < psi_sat, clamped to D - 1; 0 when every node is
    saturated."""
    psi = np.asarray(psi)
    D = psi.shape[-1]
    unsat = ~(psi >= psat)
    deepest = D - 1 - np.argmax(unsat[:, ::-1], axis=1)
    return np.where(unsat.any(axis=1), np.minimum(deepest + 1, D - 1), 0).astype(np.int64)


def y_of(psi, b, psat, dz):
    """test_gpu_enkf._y_of: the continuous water table, the same float64 operations member by member."""
    psi, b = np.asarray(psi), np.asarray(b).astype(np.int64)
    k = np.arange(psi.shape[0])
    below = psi[k, b]
    above = psi[k, np.maximum(b - 1, 0)]
    y = b.astype(np.float64) * dz
    with np.errstate(invalid="ignore", divide="ignore"):
        crossing = (b - 1).astype(np.float64) * dz + dz * (psat - above) / (below - above)
        inside = (b >= 1) & (above < psat) & (psat <= below)
    return np.where(inside, crossing, y)


# ---- tempering, the sums of a trial without a loop over the members ------------------------------------------------------
def weighted_sums(mult, q):
    """(sum mult q, sum mult q^2) as Python integers; q <= 2^31, sum mult < 2^31: q^2 in two 32-bit halves, each half's
    sum below 2^63."""
    mult, q = np.asarray(mult, dtype=np.int64), np.asarray(q, dtype=np.int64)
    assert q.size == 0 or (0 <= q.min() and q.max() <= FILTER_Q_ONE and mult.min() >= 0 and int(mult.sum()) < 1 << 31)
    sq = q * q
    lo, hi = sq & 0xFFFFFFFF, sq >> 32
    return int((mult * q).sum()), (int((mult * hi).sum()) << 32) + int((mult * lo).sum())


def temper_of(l, counted, ess_floor, n_b=None):
    """stepper.filter_temper_of with every trial's Q_k and S_k summed by NumPy: the same (k, trials, q)."""
    l = np.asarray(l, dtype=np.float64).reshape(-1)
    counted = np.asarray(counted, dtype=bool).reshape(-1)
    mult = np.ones(l.size, dtype=np.int64) if n_b is None else np.asarray(n_b, dtype=np.int64).reshape(-1)
    n = int(mult[counted].sum())
    if n == 0:
        return None, [], np.zeros(l.size, dtype=np.int64)
    T = filter_temper_target(ess_floor, n)
    trials = []

    def ok(k):
        Q, S = weighted_sums(mult, filter_temper_weights(l, counted, k))
        trials.append((k, Q, S))
        return filter_temper_ok(Q, S, T)

    k = TEMPER_STEPS
    if not ok(TEMPER_STEPS):
        lo, hi = 0, TEMPER_STEPS
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            lo, hi = (mid, hi) if ok(mid) else (lo, mid)
        k = lo
    return k, trials, filter_temper_weights(l, counted, k)


# ---- systematic resampling's defining property ---------------------------------------------------------------------------
def assert_systematic(anc, q_members):
    """``anc`` [N_p] (point-local) is a systematic resampling of the weights ``q_members`` [N_p]: with n_m the slots whose
    ancestor is m, sum n_m = N_p, anc is non-decreasing and |n_m Q - N_p q_m| < Q for every member, in Python integers.
    It names no draw and no prefix sum: an error the kernel shared with stepper.filter_slot_ranges would show here."""
    anc = np.asarray(anc, dtype=np.int64)
    n_p = anc.size
    assert len(q_members) == n_p and anc.min() >= 0 and anc.max() < n_p
    assert np.all(np.diff(anc) >= 0)
    n_m = np.bincount(anc, minlength=n_p)
    assert int(n_m.sum()) == n_p
    q = np.asarray(q_members).astype(object)
    Q = int(q.sum())
    assert Q > 0
    gap = n_m.astype(object) * Q - n_p * q
    worst = max(int(gap.max()), -int(gap.min()))
    assert worst < Q, (worst, Q)
    return n_m


# ---- the EnKF's references, the sums over the members in np.longdouble ----------------------------------------------------
# A mean is an np.longdouble sum rounded to float64 once; an anomaly is one float64 subtraction, a product of two anomalies
# one float64 multiplication, and the products are summed in np.longdouble again.  No rounding accumulates over the
# members: every covariance is within a few 2^-53 of its terms' absolute sum, whatever the member count.
def _long_sum(x):
    return np.asarray(x).sum(axis=0, dtype=np.longdouble)


def _mean(x):
    return (_long_sum(x) / x.shape[0]).astype(np.float64)


def _moments(psi, Y):
    """(psi's mean [D], Y's mean [W], C_psiY [D][W], C_YY [W][W]) of one point, over N_p - 1 (one member: zeros)"""
    n, W = Y.shape
    pb, yb = _mean(psi), _mean(Y)
    cpy, cyy = np.zeros((psi.shape[1], W)), np.zeros((W, W))
    if n > 1:
        A, B = psi - pb, Y - yb
        for i in range(W):
            cpy[:, i] = (_long_sum(A * B[:, i:i + 1]) / (n - 1)).astype(np.float64)
            cyy[:, i] = (_long_sum(B * B[:, i:i + 1]) / (n - 1)).astype(np.float64)
    return pb, yb, cpy, cyy


def std_columns(x):
    """per column, over N_p - 1"""
    a = x - _mean(x)
    return np.sqrt((_long_sum(a * a) / (x.shape[0] - 1)).astype(np.float64))


def _tapers(yb0, zeta_nodes, D, dz, loc, W):
    z = np.arange(D) * dz
    zeta = np.concatenate([[yb0], np.asarray(zeta_nodes, dtype=np.float64)])
    if loc > 0:
        return (gaspari_cohn(np.abs(zeta[:, None] - zeta[None, :]) / loc), gaspari_cohn(np.abs(z[:, None] - zeta[None, :]) / loc))
    return np.ones((W, W)), np.ones((D, W))


def analysis_well(psi, y, eps, obs, dz, sigma, loc, mpp):
    """test_gpu_enkf._analysis_numpy (the well alone): (K [P][D], the analysis states)."""
    N, D = psi.shape
    K = np.zeros((N // mpp, D))
    for p in range(N // mpp):
        sl = slice(p * mpp, (p + 1) * mpp)
        _, yb, cpy, cyy = _moments(psi[sl], y[sl, None])
        rho = gaspari_cohn(np.abs(np.arange(D) * dz - yb[0]) / loc) if loc > 0 else 1.0
        K[p] = rho * cpy[:, 0] / (cyy[0, 0] + sigma * sigma)
    innov = (obs * dz + sigma * eps) - y
    return K, psi + np.repeat(K, mpp, axis=0) * innov[:, None]


def analysis(psi, Y, E, o, R, zeta_nodes, dz, loc, mpp):
    """test_enkf_sm_cpu.analysis_restated: K, post, ybar (the joint log-density is left to the float64 form)."""
    N, D = psi.shape
    W, P = Y.shape[1], N // mpp
    K, ybar, post = np.zeros((P, D, W)), np.zeros((P, W)), psi.copy()
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        _, yb, cpy, cyy = _moments(psi[sl], Y[sl])
        rho_yy, rho_py = _tapers(yb[0], zeta_nodes, D, dz, loc, W)
        L = np.linalg.cholesky(rho_yy * cyy + np.diag(R))
        K[p] = np.linalg.solve(L.T, np.linalg.solve(L, (rho_py * cpy).T)).T
        post[sl] = psi[sl] + ((o[None, :] + np.sqrt(R)[None, :] * E[sl]) - Y[sl]) @ K[p].T
        ybar[p] = yb
    return {"K": K, "post": post, "ybar": ybar}


def sqrt_analysis(psi, Y, o, R, zeta_nodes, dz, loc, mpp):
    """test_enkf_sqrt_cpu.sqrt_analysis_restated: K, Kr, dbar, post, ybar."""
    N, D = psi.shape
    W, P = Y.shape[1], N // mpp
    K, Kr, dbar, ybar = np.zeros((P, D, W)), np.zeros((P, D, W)), np.zeros((P, D)), np.zeros((P, W))
    post = psi.copy()
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        _, yb, cpy, cyy = _moments(psi[sl], Y[sl])
        rho_yy, rho_py = _tapers(yb[0], zeta_nodes, D, dz, loc, W)
        L = np.linalg.cholesky(rho_yy * cyy + np.diag(R))
        u = np.linalg.solve(L, (rho_py * cpy).T)
        K[p] = np.linalg.solve(L.T, u).T
        Kr[p] = np.linalg.solve((L + np.diag(np.sqrt(R))).T, u).T
        dbar[p] = K[p] @ (o - yb)
        post[sl] = psi[sl] + dbar[p][None, :] + (yb[None, :] - Y[sl]) @ Kr[p].T
        ybar[p] = yb
    return {"K": K, "Kr": Kr, "dbar": dbar, "post": post, "ybar": ybar}


def rtps(prior, post, alpha, mpp):
    """test_enkf_sqrt_cpu.rtps_restated: sigma_b, sigma_a, f [P][D] and the relaxed states."""
    N, D = post.shape
    P = N // mpp
    sb, sa, f = np.zeros((P, D)), np.zeros((P, D)), np.ones((P, D))
    out = post.copy()
    for p in range(P):
        sl = slice(p * mpp, (p + 1) * mpp)
        if mpp > 1:
            sb[p], sa[p] = std_columns(prior[sl]), std_columns(post[sl])
        good = (sa[p] > 0) & np.isfinite(sa[p])
        with np.errstate(divide="ignore", invalid="ignore"):
            f[p] = np.where(good, 1.0 + alpha * (sb[p] - sa[p]) / sa[p], 1.0)
        mean = _mean(post[sl])
        out[sl] = np.where(f[p][None, :] == 1.0, post[sl], mean[None, :] + f[p][None, :] * (post[sl] - mean[None, :]))
    return sb, sa, f, out


def mean_std(x):
    """(mean, std over N - 1) of a vector, its sums in np.longdouble"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 1)
    return float(_mean(x)[0]), float(std_columns(x)[0]) if x.shape[0] > 1 else 0.0
