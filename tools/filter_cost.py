"""What the particle filter costs (hc_set_filter): column-days/s of the bench-size ensemble without the filter and with
assimilations every 48th row (one a day), one handle each, back to back on one GPU.

    python tools/filter_cost.py [--members 262144] [--depth 300] [--days 30] [--warmup 1] [--strides 0,48]
                                [--sigma 10] [--spread-cm 0] [--sensors 0,0] [--ess-floor 0,0.5] [--window 0,1]
                                [--window-offsets 12,24,36] [--rejuvenation 0.95] [--json out.json]

Same set-up as tools/wtd_dist_cost.py and bench.py's timed region: synthetic 10-year forcing, Philox noise, the shared
initial condition of the well's digest (tests/golden/g1_tables_<depth>.npz where it exists, else the hydrostatic profile),
W warm-up days, then K timed days, the library's own launch length.  The timed figure is wall time around hc_step_rows:
the step launches AND everything behind them -- with the filter, the Philox staging of the refresh vectors, the
weights, scan, fill and gather kernels.  `step_kernel_ms` is the step kernel alone (HIP events around its launches), so
`other_ms` = wall - step kernel is what the rest costs; `filter_ms_per_assimilation` is the filtered run's `other_ms` over
the unfiltered one's, per assimilation.  A stride may be listed more than once (e.g. 0,48,0,48 to alternate); `kept` is a
run's rate over the mean of the stride-0 runs.  --spread-cm W starts every member from the initial profile shifted by its
own offset, uniform over +-W cm: water tables in many bins, unequal weights, and (small sigma) the weight on a few members
whose slot ranges are long.  --sensors lists, run by run like --strides, how many soil-moisture sensors join the well
(hc_set_filter_soil_moisture: nodes 6, 12, 24, ..., a reading of 0.25 with error --sensor-sigma on every assimilation row,
so every assimilation takes the per-member path; one count serves every run).  --ess-floor lists, run by run, the floor
of the tempered weights (hc_set_filter_tempering; 0 = off, the untempered path): `tempered_rows` and `beta_min` over the
timed assimilations, and -- when no run has stride 0 -- `kept` and `temper_ms_per_assimilation` are taken against the
mean of the runs with floor 0.  --window lists, run by run, whether the well's record inside the window joins the weights
(hc_set_filter_window with --window-offsets; 1 = on): `lagged_per_assimilation`, and -- when no run has stride 0 and no
floor is set -- `kept` and `window_ms_per_assimilation` against the mean of the runs without a window.  --rejuvenation
delta rejuvenates the base noise vectors of every filtered run (hc_set_filter_rejuvenation; 0 = off): `rejuvenated_rows`
and `spread_kept` (the mean of the table's entry 3 over entry 2) over the timed assimilations; its cost is the
`filter_ms_per_assimilation` of this command against the same command without the flag.  Prints one JSON line.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def run(cols, forcing, psi0, members, stride, sigma, warmup_days, days, spread_cm=0.0, seed=2024, sensors=0,
        sensor_sigma=0.05, ess_floor=0.0, window=(), rejuvenation=0.0):
    from hydromodel_amd.stepper import EnsembleStepper, filter_summary
    st = EnsembleStepper(cols, forcing, members)
    try:
        if spread_cm:
            off = np.random.default_rng(seed).uniform(-spread_cm, spread_cm, size=members)
            st.set_state(np.asarray(psi0)[None, :] + off[:, None])
        else:
            st.set_state(psi0)
        st.set_noise_philox(seed, 0)
        if stride:
            st.set_filter(stride, sigma, seed)
        if stride and sensors:
            values = np.full((forcing.dim_t, sensors), np.nan)
            values[::stride] = 0.25
            st.set_filter_soil_moisture([6 * (1 << i) for i in range(sensors)], values, sensor_sigma)
        if stride and ess_floor:
            st.set_filter_tempering(ess_floor)
        if stride and window:
            st.set_filter_window(window)
        if stride and rejuvenation:
            st.set_filter_rejuvenation(rejuvenation)
        row = 1
        if warmup_days:
            st.step_rows(row, 48 * warmup_days)
            row += 48 * warmup_days
        st.lib.hc_synchronize(st.h)
        t0 = time.perf_counter()
        out = st.step_rows(row, 48 * days)
        st.lib.hc_synchronize(st.h)
        wall = time.perf_counter() - t0
        rec = {"stride": stride, "sensors": sensors if stride else 0, "ess_floor": ess_floor if stride else 0.0,
               "window": list(window) if stride else [], "rejuvenation": rejuvenation if stride else 0.0, "wall_s": wall, "step_kernel_ms": out["kernel_ms"], "launches": out["launches"],
               "other_ms": 1e3 * wall - out["kernel_ms"], "column_days_per_s": members * days / wall}
        if stride:
            s = filter_summary(st.filter_table()[0], stride, sigma)
            timed = s["rows"] >= row
            rec["assimilations"] = int(timed.sum())
            rec["ess_median"] = float(np.median(s["ess"][timed])) if timed.any() else None
            rec["survivors_median"] = float(np.median(s["survivors"][timed])) if timed.any() else None
            rec["loglik"] = s["loglik"]
            if ess_floor:
                beta = st.filter_temper_table()[0, s["rows"] // stride, 0][timed]
                rec["tempered_rows"] = int((beta < 1.0).sum())
                rec["beta_min"] = float(np.nanmin(beta)) if timed.any() else None
            if window:
                wt = st.filter_window_table()[0, s["rows"] // stride, :, 0][timed]
                rec["lagged_per_assimilation"] = float((wt == 1.0).sum() / max(int(timed.sum()), 1))
            if rejuvenation:
                rt = st.filter_rejuvenation_table()[0, s["rows"] // stride][timed]
                moved = rt[:, 0] == 1.0
                rec["rejuvenated_rows"] = int(moved.sum())
                rec["rejuvenation_refused"] = int(np.nansum(rt[:, 1]))
                rec["spread_kept"] = float((rt[moved, 3] / rt[moved, 2]).mean()) if moved.any() else None
            if timed.any():
                rec["longest_range"] = int(np.bincount(st.filter_ancestors(), minlength=members).max())   # the last one
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
    ap.add_argument("--strides", default="0,48")
    ap.add_argument("--sigma", type=float, default=10.0)
    ap.add_argument("--spread-cm", type=float, default=0.0)
    ap.add_argument("--sensors", default="")
    ap.add_argument("--sensor-sigma", type=float, default=0.05)
    ap.add_argument("--ess-floor", default="")
    ap.add_argument("--window", default="")
    ap.add_argument("--window-offsets", default="12,24,36")
    ap.add_argument("--rejuvenation", type=float, default=0.0)
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
    strides = [int(s) for s in args.strides.split(",")]
    sensors = [int(s) for s in args.sensors.split(",")] if args.sensors else [0] * len(strides)
    if len(sensors) == 1:
        sensors = sensors * len(strides)
    if len(sensors) != len(strides):
        ap.error("--sensors lists one count per entry of --strides")
    floors = [float(s) for s in args.ess_floor.split(",")] if args.ess_floor else [0.0] * len(strides)
    if len(floors) != len(strides):
        ap.error("--ess-floor lists one floor per entry of --strides")
    offsets = tuple(int(o) for o in args.window_offsets.split(","))
    windows = [offsets if int(w) else () for w in args.window.split(",")] if args.window else [()] * len(strides)
    if len(windows) != len(strides):
        ap.error("--window lists one flag per entry of --strides")
    recs = [run(cols, forcing, psi0, args.members, s, args.sigma, args.warmup, args.days, args.spread_cm, sensors=n,
                sensor_sigma=args.sensor_sigma, ess_floor=f, window=w, rejuvenation=args.rejuvenation)
            for s, n, f, w in zip(strides, sensors, floors, windows)]
    base = [r for r in recs if r["stride"] == 0]
    if base:
        rate = float(np.mean([r["column_days_per_s"] for r in base]))
        other = float(np.mean([r["other_ms"] for r in base]))
        for r in recs:
            r["kept"] = r["column_days_per_s"] / rate
            if r["stride"] and r.get("assimilations"):
                r["filter_ms_per_assimilation"] = (r["other_ms"] - other) / r["assimilations"]
    untempered = [r for r in recs if r["stride"] and not r["ess_floor"]]
    if not base and untempered:
        rate = float(np.mean([r["column_days_per_s"] for r in untempered]))
        other = float(np.mean([r["other_ms"] for r in untempered]))
        for r in recs:
            r["kept"] = r["column_days_per_s"] / rate
            r["other_ms_per_assimilation"] = r["other_ms"] / max(r.get("assimilations", 0), 1)
            if r["ess_floor"] and r.get("assimilations"):
                r["temper_ms_per_assimilation"] = (r["other_ms"] - other) / r["assimilations"]
    plain = [r for r in recs if r["stride"] and not r["ess_floor"] and not r["window"]]
    if not base and plain and any(r["window"] for r in recs) and not any(r["ess_floor"] for r in recs):
        rate = float(np.mean([r["column_days_per_s"] for r in plain]))
        other = float(np.mean([r["other_ms"] for r in plain]))
        step = float(np.mean([r["step_kernel_ms"] for r in plain]))
        for r in recs:
            r["kept"] = r["column_days_per_s"] / rate
            if r["window"] and r.get("assimilations"):
                r["window_ms_per_assimilation"] = (r["other_ms"] - other) / r["assimilations"]
                r["window_step_kernel_ms_per_assimilation"] = (r["step_kernel_ms"] - step) / r["assimilations"]
    line = json.dumps({"members": args.members, "depth": args.depth, "days": args.days, "sigma_cm": args.sigma, "spread_cm": args.spread_cm,
                       "runs": recs})
    print(line)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(line + "\n")


if __name__ == "__main__":
    main()
