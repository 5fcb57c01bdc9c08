"""What the root-water uptake by depth costs (hc_set_root_uptake): column-days/s of the bench-size ensemble with the period
totals alone, with the uptake on top of them, and with `Profiles: 1` (the profile statistics at stride 1, which stage every
row's end state as the uptake does), one handle each, back to back on one GPU.

    python tools/uptake_cost.py [--members 262144] [--depth 300] [--days 30] [--warmup 1] [--rows 1440]
                                [--layers-cm 0:100,100:300,300:1500] [--bins 128] [--runs 0,1,0,1,2] [--json out.json]

Same set-up as tools/period_totals_cost.py and bench.py's timed region: synthetic 10-year forcing, Philox noise, the shared
initial condition of the well's digest (tests/golden/g1_tables_<depth>.npz where it exists, else the hydrostatic profile),
W warm-up days, then K timed days, the library's own launch length.  `--runs` lists the runs: 0 = the period totals alone
(the feature off), 1 = the uptake on, 2 = the period totals with the profile statistics at stride 1.  The uptake's figure
holds the stores of every row's end state by the step kernels, the launches shortened to what ~4 GiB of staged states
admit, root_uptake_kernel behind every daylight row and uptake_reduce_kernel at the end of every period.  The timed figure
is wall time around hc_step_rows.  `kept` is a run's rate over the mean of the runs of kind 0.  Prints one JSON line.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def run(cols, forcing, psi0, members, kind, period_rows, layers_cm, bins, warmup_days, days, seed=2024):
    from hydromodel_amd.stepper import EnsembleStepper, layer_cells, period_ends
    st = EnsembleStepper(cols, forcing, members)
    try:
        st.set_state(psi0)
        st.set_noise_philox(seed, 0)
        if kind == 2:
            st.set_profile_stats(1)
        ends = period_ends(forcing.dim_t, rows=period_rows)
        ends = ends[ends <= 48 * (warmup_days + days)]
        st.set_period_totals(ends)
        if kind == 1:
            st.set_root_uptake(layer_cells(cols.z, layers_cm), bins)
        row = 1
        if warmup_days:
            st.step_rows(row, 48 * warmup_days)
            row += 48 * warmup_days
        st.lib.hc_synchronize(st.h)
        t0 = time.perf_counter()
        out = st.step_rows(row, 48 * days)
        st.lib.hc_synchronize(st.h)
        wall = time.perf_counter() - t0
        rec = {"kind": kind, "what": ("periods", "uptake", "profiles_1")[kind], "wall_s": wall, "step_kernel_ms": out["kernel_ms"],
               "launches": out["launches"], "column_days_per_s": members * days / wall}
        if kind == 1:
            t1 = time.perf_counter()
            stats = st.root_uptake_stats()
            rec["stats_ms"] = 1e3 * (time.perf_counter() - t1)
            counted = stats["count"] > 0
            rec.update(period_rows=period_rows, periods=int(ends.size), periods_counted=int(counted.sum()), bins=bins,
                       cells=st.uptake_cells.tolist(), overflow=st.root_uptake_overflow(), outside=st.root_uptake_outside())
            if counted.any():
                rec["last_total_mean_cm"] = float(stats["total_mean_cm"][counted][-1])
                rec["last_total_std_cm"] = float(stats["total_std_cm"][counted][-1])
                rec["last_share_of_mean"] = stats["share_of_mean"][counted][-1].tolist()
                rec["last_depth_quantile_cm"] = stats["depth_quantile_cm"][counted][-1].tolist()
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
    ap.add_argument("--layers-cm", default="0:100,100:300,300:1500")
    ap.add_argument("--bins", type=int, default=128)
    ap.add_argument("--runs", default="0,1,0,1,2")
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
    layers = [tuple(float(v) for v in lay.split(":")) for lay in args.layers_cm.split(",") if lay]
    recs = [run(cols, forcing, psi0, args.members, int(k), args.rows, layers, args.bins, args.warmup, args.days)
            for k in args.runs.split(",")]
    base = [r["column_days_per_s"] for r in recs if r["kind"] == 0]
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
