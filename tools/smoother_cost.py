"""What the fixed-lag smoother costs (hc_set_filter_smoother), and what it buys in a twin experiment.

    python tools/smoother_cost.py [--members 262144] [--depth 300] [--days 30] [--warmup 1] [--lag-days 30]
                                  [--runs 0,1,0,1] [--json out.json]
    python tools/smoother_cost.py --twin [--members 4096] [--depth 300] [--days 90] [--lags 0,1,5,10,30]
                                  [--ess-floors 0,0.5] [--sigma-cm 10] [--spread-cm 60] [--json out.json]

Cost: bench.py's set-up (synthetic 10-year forcing, Philox noise, the well's shared initial condition, W warm-up days, K
timed days, the library's own launch length) with a daily particle filter; `--runs` lists the runs: 0 = the filter alone,
1 = the smoother at a daily stride and `--lag-days` record rows on top.  The timed figure is wall time around
hc_step_rows; `kept` is a run's rate over the mean of the runs of kind 0.  Under `rocprofv3 --kernel-trace --stats` the
same command gives the kernel times of smoother_store_kernel, smoother_gather_kernel and smoother_emit_kernel.

Twin: the synthetic truth is the water table of one member outside the ensemble on the same record; the ensemble is
filtered on it daily from initial profiles shifted by up to `--spread-cm`, and the mean CRPS of the forecast
(hc_set_wtd_hist), the analysis (lag 0) and the smoothed distributions at each lag is taken over the same rows -- those
every lag reaches in full -- next to the fewest and the median distinct paths behind them, once per ESS floor (0: no
tempering).  Prints one JSON line.
"""
import argparse
import copy
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def setup(depth, years):
    from hydromodel_amd.digest import ColumnTables, ForcingDigest
    from hydromodel_amd.ensemble import pressure_head
    from hydromodel_amd.synthetic import default_parameters, synthetic_forcing_frame, synthetic_well
    params = default_parameters()
    cols = ColumnTables(params, synthetic_well(depth))
    forcing = ForcingDigest(params, synthetic_forcing_frame(years), cols)
    fixture = REPO / "tests" / "golden" / f"g1_tables_{depth}.npz"
    psi0 = np.load(fixture)["initial_cond"] if fixture.exists() else pressure_head(cols, cols.por_raw)[0]
    return cols, forcing, psi0


def cost_run(cols, forcing, psi0, members, kind, lag_days, warmup_days, days, sigma_cm, seed=2024):
    from hydromodel_amd.stepper import EnsembleStepper
    st = EnsembleStepper(cols, forcing, members)
    try:
        st.set_state(psi0)
        st.set_noise_philox(seed, 0)
        st.set_filter(48, sigma_cm, seed)
        if kind == 1:
            st.set_filter_smoother(48, lag_days)
        row = 1
        if warmup_days:
            st.step_rows(row, 48 * warmup_days)
            row += 48 * warmup_days
        st.lib.hc_synchronize(st.h)
        t0 = time.perf_counter()
        out = st.step_rows(row, 48 * days)
        st.lib.hc_synchronize(st.h)
        wall = time.perf_counter() - t0
        rec = {"kind": kind, "what": ("filter", "smoother")[kind], "wall_s": wall, "step_kernel_ms": out["kernel_ms"],
               "launches": out["launches"], "column_days_per_s": members * days / wall}
        if kind == 1:
            t1 = time.perf_counter()
            st.filter_smoother_flush()
            paths = st.filter_smoother_paths()[0]
            rec["flush_ms"] = 1e3 * (time.perf_counter() - t1)
            emitted = paths[:, 1] >= 0
            rec.update(lag_days=lag_days, rows_emitted=int(emitted.sum()), fewest_paths=int(paths[emitted, 0].min()),
                       ring_bytes=6 * (lag_days + 1) * members)
        return rec
    finally:
        st.close()


def twin(cols, forcing, psi0, members, days, lags, floors, sigma_cm, spread_cm, seed=2024):
    from hydromodel_amd.stepper import EnsembleStepper, filter_smoother_summary, wtd_distribution
    rows = 48 * days
    st = EnsembleStepper(cols, forcing, 1)
    try:                                             # the truth: a member of another stream, unfiltered
        st.set_state(np.asarray(psi0) + 0.37 * spread_cm)     # somewhere inside the ensemble's initial spread
        st.set_noise_philox(seed, 1 << 40)
        truth = st.step_rows(1, rows, want_wtd=True)["wtd"][:, 0]
    finally:
        st.close()
    record = copy.copy(forcing)
    record.wtd_obs = np.array(forcing.wtd_obs, dtype=np.int32)
    record.wtd_obs[1:rows + 1] = np.where(truth < cols.dim_d, truth, -1)
    common = np.arange(1, days - max(lags) + 1)       # the days every lag reaches in full
    out = []
    for floor in floors:
        for lag in lags:
            st = EnsembleStepper(cols, record, members)
            try:
                shift = np.random.default_rng(seed).uniform(-spread_cm, spread_cm, size=members)
                st.set_state(np.asarray(psi0)[None, :] + shift[:, None])
                st.set_noise_philox(seed, 0)
                st.set_filter(48, sigma_cm, seed)
                if floor:
                    st.set_filter_tempering(floor)
                st.set_wtd_hist(48)
                st.set_filter_smoother(48, lag)
                st.step_rows(1, rows)
                st.filter_smoother_flush()
                s = filter_smoother_summary(st.filter_smoother_hist()[0], st.filter_smoother_paths()[0], record.wtd_obs,
                                            (0.5,), cols.dz, cols.z, 48)
                f = wtd_distribution(st.wtd_hist_table()[0], record.wtd_obs, (0.5,), cols.dz, cols.z, stride=48)
                ok = common[(s["count"][common] > 0) & (s["lag_rows"][common] == 48 * lag)]
                out.append({"ess_floor": floor, "lag_days": lag, "rows": int(ok.size),
                            "crps_forecast_cm": float(f["crps_cm"][ok].mean()), "crps_smoothed_cm": float(s["crps_cm"][ok].mean()),
                            "fewest_paths": int(s["unique_paths"][ok].min()),
                            "median_paths": float(np.median(s["unique_paths"][ok])),
                            "ess_mean": float(np.nanmean(st.filter_table()[0, 1:days + 1, 1]))})
            finally:
                st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--twin", action="store_true")
    ap.add_argument("--members", type=int, default=0)
    ap.add_argument("--depth", type=int, default=300)
    ap.add_argument("--days", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--years", type=int, default=10)
    ap.add_argument("--lag-days", type=int, default=30)
    ap.add_argument("--lags", default="0,1,5,10,30")
    ap.add_argument("--ess-floors", default="0,0.5")
    ap.add_argument("--sigma-cm", type=float, default=10.0)
    ap.add_argument("--spread-cm", type=float, default=60.0, help="twin: the members' initial profiles are shifted by +-this")
    ap.add_argument("--runs", default="0,1,0,1")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    from hydromodel_amd import _lib
    cols, forcing, psi0 = setup(args.depth, args.years)
    if args.twin:
        members, days = args.members or 4096, args.days or 90
        res = {"twin": twin(cols, forcing, psi0, members, days, [int(v) for v in args.lags.split(",")],
                            [float(v) for v in args.ess_floors.split(",")], args.sigma_cm, args.spread_cm)}
    else:
        members, days = args.members or 262144, args.days or 30
        recs = [cost_run(cols, forcing, psi0, members, int(k), args.lag_days, args.warmup, days, args.sigma_cm)
                for k in args.runs.split(",")]
        base = [r["column_days_per_s"] for r in recs if r["kind"] == 0]
        if base:
            for r in recs:
                r["kept"] = r["column_days_per_s"] / float(np.mean(base))
        res = {"runs": recs}
    line = json.dumps({"members": members, "depth": args.depth, "days": days, "sigma_cm": args.sigma_cm,
                       "kernels": _lib.kernel_hash(), **res})
    print(line)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(line + "\n")


if __name__ == "__main__":
    main()
