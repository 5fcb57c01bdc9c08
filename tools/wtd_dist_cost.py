"""What the ensemble water-table histograms cost (hc_set_wtd_hist): column-days/s of the bench-size ensemble without
histograms, with a daily stride (48) and with every row (1), one handle each, back to back on one GPU.

    python tools/wtd_dist_cost.py [--members 262144] [--depth 300] [--days 30] [--warmup 1] [--strides 0,48,1]
                                  [--json out.json]

Same set-up as tools/profile_stats_cost.py and bench.py's timed region: synthetic 10-year forcing, Philox noise, the
shared initial condition of the well's digest (tests/golden/g1_tables_<depth>.npz where it exists, else the hydrostatic
profile), W warm-up days, then K timed days, the library's own launch length.  The timed figure is wall time around
hc_step_rows: the step launches AND the histogram kernels behind them.  A stride may be listed more than once (e.g.
0,1,0,1 to alternate); `kept` is a run's rate over the mean of the stride-0 runs.  The summary (hc_wtd_distribution, five
levels) of each table is timed on its own.  Prints one JSON line.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def run(cols, forcing, psi0, members, stride, warmup_days, days, seed=2024):
    from hydromodel_amd.stepper import EnsembleStepper, wtd_distribution
    st = EnsembleStepper(cols, forcing, members)
    try:
        st.set_state(psi0)
        st.set_noise_philox(seed, 0)
        if stride:
            st.set_wtd_hist(stride)
        row = 1
        if warmup_days:
            st.step_rows(row, 48 * warmup_days)
            row += 48 * warmup_days
        st.lib.hc_synchronize(st.h)
        t0 = time.perf_counter()
        out = st.step_rows(row, 48 * days)
        st.lib.hc_synchronize(st.h)
        wall = time.perf_counter() - t0
        rec = {"stride": stride, "wall_s": wall, "step_kernel_ms": out["kernel_ms"], "launches": out["launches"],
               "column_days_per_s": members * days / wall}
        if stride:
            table = st.wtd_hist_table()
            t1 = time.perf_counter()
            d = wtd_distribution(table, forcing.wtd_obs, (0.05, 0.25, 0.5, 0.75, 0.95), cols.dz, cols.z, 0, stride)
            rec["summary_ms"] = 1e3 * (time.perf_counter() - t1)
            counted = d["count"][0] > 0
            rec["rows_counted"] = int(counted.sum())
            rec["members_per_row"] = sorted({int(c) for c in d["count"][0][counted]})
            rec["crps_mean_cm"] = d["crps_mean_cm"][0]
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
    ap.add_argument("--strides", default="0,48,1")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    from hydromodel_amd.digest import ColumnTables, ForcingDigest
    from hydromodel_amd.ensemble import pressure_head
    from hydromodel_amd.synthetic import default_parameters, synthetic_forcing_frame, synthetic_well
    params = default_parameters()
    cols = ColumnTables(params, synthetic_well(args.depth))
    forcing = ForcingDigest(params, synthetic_forcing_frame(args.years), cols)
    fixture = REPO / "tests" / "golden" / f"g1_tables_{args.depth}.npz"
    psi0 = np.load(fixture)["initial_cond"] if fixture.exists() else pressure_head(cols, cols.por_raw)[0]
    recs = [run(cols, forcing, psi0, args.members, int(s), args.warmup, args.days) for s in args.strides.split(",")]
    base = [r["column_days_per_s"] for r in recs if r["stride"] == 0]
    if base:
        for r in recs:
            r["kept"] = r["column_days_per_s"] / float(np.mean(base))
    line = json.dumps({"members": args.members, "depth": args.depth, "days": args.days, "runs": recs})
    print(line)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(line + "\n")


if __name__ == "__main__":
    main()
