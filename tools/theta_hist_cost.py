"""What the ensemble soil-moisture histograms cost (hc_set_theta_hist): column-days/s of the bench-size ensemble with
profile statistics at a daily stride, without the histograms and with them, one handle each, back to back on one GPU.

    python tools/theta_hist_cost.py [--members 262144] [--depth 300] [--days 30] [--warmup 1] [--stride 48]
                                    [--bins 0,128,0,128,0,128] [--json out.json]

Same set-up as tools/wtd_dist_cost.py and bench.py's timed region: synthetic 10-year forcing, Philox noise, the shared
initial condition of the well's digest (tests/golden/g1_tables_<depth>.npz where it exists, else the hydrostatic profile),
W warm-up days, then K timed days, the library's own launch length.  The timed figure is wall time around hc_step_rows: the
step launches AND the profile and histogram kernels behind them.  A bin count may be listed more than once (0,128,0,128 to
alternate); `kept` is a run's rate over the mean of the runs without histograms.  A library without hc_set_theta_hist (an
earlier build, for the comparison against it) runs the bins = 0 entries only.  The quantile bands (five levels, NumPy on
the host) of each table are timed on their own.  Prints one JSON line.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def run(cols, forcing, psi0, members, stride, bins, warmup_days, days, seed=2024):
    from hydromodel_amd.stepper import EnsembleStepper
    st = EnsembleStepper(cols, forcing, members)
    try:
        st.set_state(psi0)
        st.set_noise_philox(seed, 0)
        st.set_profile_stats(stride)
        if bins:
            st.set_theta_hist(bins)
        st.profile_snapshot(0)
        row = 1
        if warmup_days:
            st.step_rows(row, 48 * warmup_days)
            row += 48 * warmup_days
        st.lib.hc_synchronize(st.h)
        t0 = time.perf_counter()
        out = st.step_rows(row, 48 * days)
        st.lib.hc_synchronize(st.h)
        wall = time.perf_counter() - t0
        rec = {"bins": bins, "stride": stride, "wall_s": wall, "step_kernel_ms": out["kernel_ms"],
               "launches": out["launches"], "column_days_per_s": members * days / wall}
        if bins:
            from hydromodel_amd.stepper import theta_distribution
            table = st.theta_hist_table()
            t1 = time.perf_counter()
            d = theta_distribution(table[0], (0.05, 0.25, 0.5, 0.75, 0.95), bins, stride)
            rec["bands_ms"] = 1e3 * (time.perf_counter() - t1)
            counted = d["count"] > 0
            rec["rows_counted"] = int(counted.sum())
            rec["members_per_row"] = sorted({int(c) for c in d["count"][counted]})
            rec["outside"] = st.theta_hist_outside()
            rec["bins_occupied_per_node_mean"] = float((table[0][counted] > 0).sum(axis=-1).mean())
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
    ap.add_argument("--stride", type=int, default=48)
    ap.add_argument("--bins", default="0,128,0,128,0,128")
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
    have = "hc_set_theta_hist" in _lib.EXPORTS
    recs = [run(cols, forcing, psi0, args.members, args.stride, int(b), args.warmup, args.days)
            for b in args.bins.split(",") if have or int(b) == 0]
    base = [r["column_days_per_s"] for r in recs if r["bins"] == 0]
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
