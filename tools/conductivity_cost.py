"""What the ensemble conductivity profiles cost (hc_set_conductivity_stats): column-days/s of the bench-size ensemble with
the profile statistics alone and with the conductivity table on top of them, one handle each, back to back on one GPU.

    python tools/conductivity_cost.py [--members 262144] [--depth 300] [--days 30] [--warmup 1] [--stride 48]
                                      [--layers-cm 0:100,100:300] [--source philox|correlated] [--runs 0,1,0,2]
                                      [--json out.json]

Same set-up as tools/storage_cost.py and bench.py's timed region: synthetic 10-year forcing, Philox noise, the shared
initial condition of the well's digest (tests/golden/g1_tables_<depth>.npz where it exists, else the hydrostatic profile),
W warm-up days, then K timed days, the library's own launch length.  `--runs` lists the runs: 0 = the profile statistics
alone (the feature off: on the parent commit the same run), 1 = the node statistics on, 2 = with the layers as well, 3 = a
run of kind 0 with its launches cut at every profile row by hand (the launch cut without the kernels).  `--source
correlated` sets a noise correlation, so that the handle fills the vectors in memory and the table reads them there
instead of regenerating the normals.  A run's figure holds the launches that now end on every profile row, the per-row
stats the launch stages, and conductivity_kernel / conductivity_layer_kernel behind every profile row.  The timed figure is
wall time around hc_step_rows.  `kept` is a run's rate over the mean of the runs of kind 0.  Prints one JSON line.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def run(cols, forcing, psi0, members, kind, stride, layers_cm, source, warmup_days, days, seed=2024):
    from hydromodel_amd.stepper import EnsembleStepper, layer_ranges, noise_correlation_tables
    st = EnsembleStepper(cols, forcing, members)
    try:
        st.set_state(psi0)
        st.set_noise_philox(seed, 0)
        if source == "correlated":
            st.set_noise_correlation(*noise_correlation_tables(cols.z, 50.0, ()))
        st.set_profile_stats(stride)
        if kind in (1, 2):
            st.set_conductivity_stats(layer_ranges(cols.z, layers_cm) if kind == 2 else ())
        st.profile_snapshot(0)
        row = 1
        if warmup_days:
            st.step_rows(row, 48 * warmup_days)
            row += 48 * warmup_days
        st.lib.hc_synchronize(st.h)
        last, kernel_ms, launches = row + 48 * days - 1, 0.0, 0
        t0 = time.perf_counter()
        while row <= last:
            stop = min(last, (row + stride - 1) // stride * stride) if kind == 3 else last
            out = st.step_rows(row, stop - row + 1)
            kernel_ms, launches, row = kernel_ms + out["kernel_ms"], launches + out["launches"], stop + 1
        st.lib.hc_synchronize(st.h)
        wall = time.perf_counter() - t0
        rec = {"kind": kind, "what": ("profiles", "conductivity", "conductivity_layers", "profiles_cut")[kind], "source": source,
               "wall_s": wall, "step_kernel_ms": kernel_ms, "launches": launches, "column_days_per_s": members * days / wall}
        if kind in (1, 2):
            t1 = time.perf_counter()
            stats = st.conductivity_stats()
            rec["stats_ms"] = 1e3 * (time.perf_counter() - t1)
            counted = np.flatnonzero(stats["count"][..., 1].max(axis=-1) > 0)
            rec.update(rows_counted=int(counted.size), overflow=st.conductivity_overflow(),
                       left_out_hrc=int((members - stats["count"][counted, :, 0]).sum()))
            j = counted[-1]
            rec["last_K_bkg_geomean_minmax"] = [float(np.nanmin(stats["K_bkg_geomean"][j])), float(np.nanmax(stats["K_bkg_geomean"][j]))]
            rec["last_lnK_hrc_std_max"] = float(np.nanmax(stats["lnK_hrc_std"][j]))
            if kind == 2:
                rec["last_K_eff_geomean"] = stats["K_eff_geomean"][j].tolist()
                rec["last_lnK_eff_std"] = stats["lnK_eff_std"][j].tolist()
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
    ap.add_argument("--layers-cm", default="0:100,100:300")
    ap.add_argument("--source", choices=("philox", "correlated"), default="philox")
    ap.add_argument("--runs", default="0,1,0,2")
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
    recs = [run(cols, forcing, psi0, args.members, int(k), args.stride, layers, args.source, args.warmup, args.days)
            for k in args.runs.split(",")]
    base = [r["column_days_per_s"] for r in recs if r["kind"] == 0]
    if base:
        for r in recs:
            r["kept"] = r["column_days_per_s"] / float(np.mean(base))
    line = json.dumps({"members": args.members, "depth": args.depth, "days": args.days, "stride": args.stride,
                       "kernels": _lib.kernel_hash(), "runs": recs})
    print(line)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(line + "\n")


if __name__ == "__main__":
    main()
