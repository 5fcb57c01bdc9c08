"""What the period totals per member cost (hc_set_period_totals): column-days/s of the bench-size ensemble without the
feature and with it, one handle each, back to back on one GPU.

    python tools/period_totals_cost.py [--members 262144] [--depth 300] [--days 30] [--warmup 1] [--rows 1440]
                                       [--thresholds-cm 100,200] [--bins 128] [--runs 0,1,0,1,0,1] [--json out.json]

Same set-up as tools/storage_cost.py and bench.py's timed region: synthetic 10-year forcing, Philox noise, the shared
initial condition of the well's digest (tests/golden/g1_tables_<depth>.npz where it exists, else the hydrostatic profile),
W warm-up days, then K timed days, the library's own launch length.  No profile statistics: a run without the feature
stores no diag at all, so the feature's figure holds the diag stores of the step kernels, the shorter launches (a launch
ends on every period end and holds at most 1 GiB of diag), period_accumulate_kernel behind every launch and
period_reduce_kernel at the end of every period.  The timed figure is wall time around hc_step_rows.  `--runs` lists the
runs, 0 = without and 1 = with the feature (0,1,0,1 to alternate); `--rows` is the length of a period.  `kept` is a run's
rate over the mean of the runs without the feature.  A library without hc_set_period_totals (an earlier build, for the
comparison against it) runs the 0 entries only.  Mean, sigma and the quantiles (five levels, NumPy on the host) of each
run's tables are timed on their own.  Prints one JSON line.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def run(cols, forcing, psi0, members, feature, period_rows, thresholds_cm, bins, flux_max_cm, warmup_days, days, seed=2024):
    from hydromodel_amd.stepper import EnsembleStepper
    st = EnsembleStepper(cols, forcing, members)
    try:
        st.set_state(psi0)
        st.set_noise_philox(seed, 0)
        if feature:
            from hydromodel_amd.stepper import flux_max_log2_of, period_ends, sensor_nodes
            ends = period_ends(forcing.dim_t, rows=period_rows)
            ends = ends[ends <= 48 * (warmup_days + days)]
            st.set_period_totals(ends, sensor_nodes(cols.z, thresholds_cm), bins, [flux_max_log2_of(v) for v in flux_max_cm])
        row = 1
        if warmup_days:
            st.step_rows(row, 48 * warmup_days)
            row += 48 * warmup_days
        st.lib.hc_synchronize(st.h)
        t0 = time.perf_counter()
        out = st.step_rows(row, 48 * days)
        st.lib.hc_synchronize(st.h)
        wall = time.perf_counter() - t0
        rec = {"feature": int(bool(feature)), "wall_s": wall, "step_kernel_ms": out["kernel_ms"], "launches": out["launches"],
               "column_days_per_s": members * days / wall}
        if feature:
            from hydromodel_amd.stepper import period_totals_distribution
            t1 = time.perf_counter()
            stats = st.period_totals_stats()
            rec["stats_ms"] = 1e3 * (time.perf_counter() - t1)
            counted = stats["count"] > 0
            rec.update(period_rows=period_rows, periods=int(ends.size), periods_counted=int(counted.sum()), bins=bins,
                       threshold_nodes=st.period_threshold_nodes.tolist(),
                       members_per_period=sorted({int(c) for c in stats["count"][counted]}),
                       overflow=st.period_totals_overflow(), outside=st.period_totals_outside())
            if counted.any():
                for k in ("transpiration_mean_cm", "transpiration_std_cm", "lateral_flow_mean_cm", "lateral_flow_std_cm",
                          "wtd_shallowest_mean_cm", "wtd_deepest_mean_cm"):
                    rec["last_" + k] = float(stats[k][counted][-1])
                rec["last_below_fraction_mean"] = stats["below_fraction_mean"][counted][-1].tolist()
            if bins:
                hf, hw = st.period_totals_hists()
                t1 = time.perf_counter()
                period_totals_distribution(hf[0], hw[0], (0.05, 0.25, 0.5, 0.75, 0.95), st.period_flux_max_log2,
                                           float(cols.z[0]), cols.dz)
                rec["quantiles_ms"] = 1e3 * (time.perf_counter() - t1)
                rec["flux_bins_occupied_mean"] = float((hf[0][counted] > 0).sum(axis=-1).mean()) if counted.any() else 0.0
        return rec
    finally:
        st.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=262144)
    ap.add_argument("--depth", type=int, default=300)
    ap.add_argument("--days", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--years", type=int, default=10)
    ap.add_argument("--rows", type=int, default=1440)
    ap.add_argument("--thresholds-cm", default="100,200")
    ap.add_argument("--bins", type=int, default=128)
    ap.add_argument("--flux-max-cm", default="16,64")
    ap.add_argument("--runs", default="0,1,0,1,0,1")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    from hydromodel_amd import _lib
    from hydromodel_amd.digest import ColumnTables, ForcingDigest
    from hydromodel_amd.ensemble import pressure_head
    from hydromodel_amd.synthetic import default_parameters, synthetic_forcing_frame, synthetic_well
    params = default_parameters()
    cols = ColumnTables(params, synthetic_well(args.depth))
    forcing = ForcingDigest(params, synthetic_forcing_frame(args.years), cols)
    fixture = REPO / "tests" / "golden" / f"g1_tables_{args.depth}.npz"
    psi0 = np.load(fixture)["initial_cond"] if fixture.exists() else pressure_head(cols, cols.por_raw)[0]
    thresholds = [float(v) for v in args.thresholds_cm.split(",") if v]
    flux_max = [float(v) for v in args.flux_max_cm.split(",")]
    have = "hc_set_period_totals" in _lib.EXPORTS
    recs = [run(cols, forcing, psi0, args.members, int(f), args.rows, thresholds, args.bins, flux_max, args.warmup, args.days)
            for f in args.runs.split(",") if have or int(f) == 0]
    base = [r["column_days_per_s"] for r in recs if not r["feature"]]
    if base:
        for r in recs:
            r["kept"] = r["column_days_per_s"] / float(np.mean(base))
    line = json.dumps({"members": args.members, "depth": args.depth, "days": args.days, "kernels": _lib.kernel_hash(),
                       "runs": recs})
    print(line)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(line + "\n")


if __name__ == "__main__":
    main()
