"""What the soil-water storage by depth layer costs (hc_set_layer_storage): column-days/s of the bench-size ensemble with
profile statistics at a daily stride, without the storage tables and with them, one handle each, back to back on one GPU.

    python tools/storage_cost.py [--members 262144] [--depth 300] [--days 30] [--warmup 1] [--stride 48]
                                 [--layers 0,4,0,4,0,4] [--bins 128] [--json out.json]

Same set-up as tools/theta_hist_cost.py and bench.py's timed region: synthetic 10-year forcing, Philox noise, the shared
initial condition of the well's digest (tests/golden/g1_tables_<depth>.npz where it exists, else the hydrostatic profile),
W warm-up days, then K timed days, the library's own launch length.  The timed figure is wall time around hc_step_rows: the
step launches AND the profile and storage kernels behind them.  `--layers` lists layer counts, one run each (0,4,0,4 to
alternate): n layers are the root zone [0, 100) cm, the column [0, D dz), and nested layers [0, 100 k) cm between them.
`kept` is a run's rate over the mean of the runs without storage.  A library without hc_set_layer_storage (an earlier
build, for the comparison against it) runs the 0 entries only.  Mean, sigma and the quantile bands (five levels, NumPy on
the host) of each run's tables are timed on their own.  Prints one JSON line.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def layers_cm(n, cols):
    """n nested layers from the surface: 100 cm, the whole column, then 200, 300, ... cm."""
    bottom = float(cols.z[-1]) + float(cols.dz)
    tops = [100.0, bottom] + [100.0 * k for k in range(2, n)]
    return [(float(cols.z[0]), min(b, bottom)) for b in tops[:n]]


def run(cols, forcing, psi0, members, stride, n_layers, bins, warmup_days, days, seed=2024):
    from hydromodel_amd.stepper import EnsembleStepper
    st = EnsembleStepper(cols, forcing, members)
    try:
        st.set_state(psi0)
        st.set_noise_philox(seed, 0)
        st.set_profile_stats(stride)
        if n_layers:
            from hydromodel_amd.stepper import layer_ranges
            ranges = layer_ranges(cols.z, layers_cm(n_layers, cols))
            st.set_layer_storage(ranges, bins)
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
        rec = {"layers": n_layers, "bins": bins if n_layers else 0, "stride": stride, "wall_s": wall,
               "step_kernel_ms": out["kernel_ms"], "launches": out["launches"], "column_days_per_s": members * days / wall}
        if n_layers:
            from hydromodel_amd.stepper import layer_storage_distribution
            t1 = time.perf_counter()
            stats = st.layer_storage_stats()
            rec["stats_ms"] = 1e3 * (time.perf_counter() - t1)
            counted = stats["count"] > 0
            rec["nodes"] = ranges.tolist()
            rec["rows_counted"] = int(counted.sum())
            rec["members_per_row"] = sorted({int(c) for c in stats["count"][counted]})
            rec["overflow"], rec["outside"] = st.layer_storage_overflow(), st.layer_storage_outside()
            rec["last_mean_cm"] = stats["mean_cm"][counted][-1].tolist()
            rec["last_std_cm"] = stats["std_cm"][counted][-1].tolist()
            if bins:
                table = st.layer_storage_hist_table()
                t1 = time.perf_counter()
                layer_storage_distribution(table[0], ranges, cols.dz, (0.05, 0.25, 0.5, 0.75, 0.95), stride)
                rec["bands_ms"] = 1e3 * (time.perf_counter() - t1)
                rec["bins_occupied_per_layer_mean"] = float((table[0][counted] > 0).sum(axis=-1).mean())
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
    ap.add_argument("--layers", default="0,4,0,4,0,4")
    ap.add_argument("--bins", type=int, default=128)
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
    have = "hc_set_layer_storage" in _lib.EXPORTS
    recs = [run(cols, forcing, psi0, args.members, args.stride, int(n), args.bins, args.warmup, args.days)
            for n in args.layers.split(",") if have or int(n) == 0]
    base = [r["column_days_per_s"] for r in recs if r["layers"] == 0]
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
