"""What the ensemble profile statistics cost (hc_set_profile_stats): column-days/s of the bench-size ensemble without
statistics, with a daily stride (48) and with every row (1), one handle each, back to back on one GPU.

    python tools/profile_stats_cost.py [--members 262144] [--depth 300] [--days 30] [--warmup 1] [--strides 0,48,1]
                                       [--json out.json]

Same set-up as bench.py's timed region: synthetic 10-year forcing, Philox noise, the shared initial condition of the
well's digest (the member-0 spin-up is replaced by the committed fixture tests/golden/g1_tables_300.npz at D = 300; other
depths start from the hydrostatic profile), W warm-up days, then K timed days, the library's own launch length.  The
timed figure is wall time around hc_step_rows: the step launches AND the reductions behind them.  Prints one JSON line.
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
    from hydromodel_amd.stepper import EnsembleStepper
    st = EnsembleStepper(cols, forcing, members)
    try:
        st.set_state(psi0)
        st.set_noise_philox(seed, 0)
        if stride:
            st.set_profile_stats(stride)
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
        rec = {"stride": stride, "wall_s": wall, "step_kernel_ms": out["kernel_ms"], "launches": out["launches"],
               "column_days_per_s": members * days / wall}
        if stride:
            rec["overflow"] = st.profile_overflow()
            s = st.profile_stats()
            rec["finite_profile_rows"] = int(np.isfinite(s["theta_vol_mean"][:, 0]).sum())
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
    base = next((r for r in recs if r["stride"] == 0), None)
    if base:
        for r in recs:
            r["kept"] = r["column_days_per_s"] / base["column_days_per_s"]
    line = json.dumps({"members": args.members, "depth": args.depth, "days": args.days, "runs": recs})
    print(line)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(line + "\n")


if __name__ == "__main__":
    main()
