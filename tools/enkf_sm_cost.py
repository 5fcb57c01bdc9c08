"""What the ensemble Kalman filter costs (hc_set_enkf, hc_set_enkf_soil_moisture): column-days/s of the bench-size
ensemble without the EnKF, with the well-only EnKF, and with the well plus sensors every 48th row (one analysis a day),
one handle each, back to back on one GPU.

    python tools/enkf_sm_cost.py [--members 262144] [--depth 300] [--days 30] [--warmup 1] [--runs 0,48s,0,48s]
                                 [--sensors 30,60,120] [--sigma 10] [--sm-sigma 0.02] [--localisation 0] [--spread-cm 0]
                                 [--method stochastic|sqrt] [--relaxation 0] [--offsets 12,24,36] [--json out.json]

Same set-up as tools/filter_cost.py and bench.py's timed region: synthetic 10-year forcing, Philox noise, the shared
initial condition of the well's digest (tests/golden/g1_tables_<depth>.npz where it exists, else the hydrostatic profile),
W warm-up days, then K timed days, the library's own launch length.  The timed figure is wall time around hc_step_rows:
the step launches AND everything behind them -- with the EnKF, the observation, reduction, gain and update kernels.
`step_kernel_ms` is the step kernel alone (HIP events around its launches), so `other_ms` = wall - step kernel is what the
rest costs; `enkf_ms_per_analysis` (well-only runs) and `sm_ms_per_analysis` (sensor runs) are a run's `other_ms` over the
stride-0 runs', per analysis.  A run is a stride (0: no EnKF, 48: the well alone) or a stride with the suffix "s" (the
well and the sensors at --sensors cm, every sensor observed on every analysis row: theta of the initial profile at its
node, held fixed -- the cost does not depend on the values); a run may be listed more than once (e.g. 0,48,0,48 to
alternate); `kept` is a run's rate over the mean of the stride-0 runs.  --spread-cm W starts every member from the
initial profile shifted by its own offset, uniform over +-W cm.  Under `rocprofv3 --kernel-trace --stats` run it with
--runs 48s (or 48) --days 1 --warmup 0 for the per-kernel time of the analyses.  --method / --relaxation: the analysis
scheme of every EnKF run (hc_set_enkf_method; the defaults do not call it).  --offsets: the well's record inside the
window (hc_set_enkf_window) for the runs with the suffix "w" (48w, 48sw): each offset's row ends a launch and records
y, so `launches` grows and the step kernel runs in shorter pieces -- `step_kernel_ms` against the stride-0 runs' is what
the cuts cost the step kernel, `window_ms_per_analysis` what everything else costs.  The suffix "g" (48g, 48sg) runs the
analysis sharded with the handle holding every member and nothing to gather (hc_set_enkf_shard, identity exchange):
`shard_ms_per_analysis` against the same run without "g" is what the global layout and the stream drains before each
reduction cost.  Prints one JSON line.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def run(cols, forcing, psi0, members, stride, sigma, loc, warmup_days, days, spread_cm=0.0, seed=2024, sensors=None,
        method="stochastic", relaxation=0.0, offsets=(), shard=False):
    from hydromodel_amd.stepper import EnsembleStepper, enkf_sm_summary, enkf_summary
    st = EnsembleStepper(cols, forcing, members)
    try:
        if spread_cm:
            off = np.random.default_rng(seed).uniform(-spread_cm, spread_cm, size=members)
            st.set_state(np.asarray(psi0)[None, :] + off[:, None])
        else:
            st.set_state(psi0)
        st.set_noise_philox(seed, 0)
        if stride:
            st.set_enkf(stride, sigma, loc, seed)
        if stride and sensors is not None:
            st.set_enkf_soil_moisture(sensors["nodes"], sensors["values"], sensors["sigma"])
        if stride and (method, relaxation) != ("stochastic", 0.0):
            st.set_enkf_method(method, relaxation)
        if stride and offsets:
            st.set_enkf_window(offsets)
        if stride and shard:
            st.set_enkf_shard(members, 0, None)
        row = 1
        if warmup_days:
            st.step_rows(row, 48 * warmup_days)
            row += 48 * warmup_days
        st.lib.hc_synchronize(st.h)
        t0 = time.perf_counter()
        out = st.step_rows(row, 48 * days)
        st.lib.hc_synchronize(st.h)
        wall = time.perf_counter() - t0
        rec = {"stride": stride, "sensors": 0 if sensors is None else len(sensors["nodes"]), "wall_s": wall, "step_kernel_ms": out["kernel_ms"], "launches": out["launches"],
               "other_ms": 1e3 * wall - out["kernel_ms"], "column_days_per_s": members * days / wall,
               "offsets": list(offsets) if stride else [], "shard": bool(stride and shard)}
        if stride:
            s = enkf_summary(st.enkf_table()[0], stride, sigma)
            timed = s["rows"] >= row
            rec["analyses"] = int(timed.sum())
            rec["prior_std_cm_median"] = float(np.median(s["prior_std_cm"][timed])) if timed.any() else None
            rec["post_std_cm_median"] = float(np.median(s["post_std_cm"][timed])) if timed.any() else None
            rec["rejected"] = int(s["rejected"].sum())
            rec["loglik"] = s["loglik"]
            if offsets:
                rec["lagged_observations"] = int(np.nansum(st.enkf_window_table()[0, :, :, 0]))
            if sensors is not None:
                sm = enkf_sm_summary(st.enkf_sm_table()[0], stride, sensors["sigma"])
                rec["sm_forecast_rmse"] = sm["rmse"].tolist()
                rec["sm_post_std_median"] = np.nanmedian(sm["post_std"], axis=0).tolist() if sm["rows"].size else None
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
    ap.add_argument("--runs", default="0,48s,0,48s")
    ap.add_argument("--sensors", default="30,60,120")
    ap.add_argument("--sm-sigma", type=float, default=0.02)
    ap.add_argument("--sigma", type=float, default=10.0)
    ap.add_argument("--localisation", type=float, default=0.0)
    ap.add_argument("--spread-cm", type=float, default=0.0)
    ap.add_argument("--method", default="stochastic", choices=("stochastic", "sqrt"))
    ap.add_argument("--relaxation", type=float, default=0.0)
    ap.add_argument("--offsets", default="12,24,36")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if "g" in args.runs:
        from hydromodel_amd import _lib
        _lib.load(with_torch=True)      # the shard's buffer is a torch tensor: torch before the library
    from hydromodel_amd.digest import ColumnTables, ForcingDigest
    from hydromodel_amd.ensemble import pressure_head
    from hydromodel_amd.synthetic import default_parameters, synthetic_forcing_frame, synthetic_well
    params = default_parameters()
    cols = ColumnTables(params, synthetic_well(args.depth))
    forcing = ForcingDigest(params, synthetic_forcing_frame(args.years), cols)
    fixture = REPO / "tests" / "golden" / f"g1_tables_{args.depth}.npz"
    psi0 = np.load(fixture)["initial_cond"] if fixture.exists() else pressure_head(cols, cols.por_raw)[0]
    from hydromodel_amd.stepper import EnsembleStepper, soil_moisture_record
    depths = [float(d) for d in args.sensors.split(",")]
    probe = EnsembleStepper(cols, forcing, 1)
    try:
        probe.set_state(psi0)
        probe.set_noise_philox(2024, 0)
        theta0 = probe.model_nodes()["theta"][0]
    finally:
        probe.close()
    rec = soil_moisture_record(cols.z, depths, np.zeros((forcing.dim_t, len(depths))), args.sm_sigma)
    rec["values"][:] = theta0[rec["nodes"]][None, :]
    offsets = tuple(int(o) for o in args.offsets.split(",") if o)
    recs = [run(cols, forcing, psi0, args.members, int(s.rstrip("swg")), args.sigma, args.localisation, args.warmup,
                args.days, args.spread_cm, sensors=rec if "s" in s else None, method=args.method,
                relaxation=args.relaxation, offsets=offsets if "w" in s else (), shard="g" in s)
            for s in args.runs.split(",")]
    base = [r for r in recs if r["stride"] == 0]
    if base:
        rate = float(np.mean([r["column_days_per_s"] for r in base]))
        other = float(np.mean([r["other_ms"] for r in base]))
        for r in recs:
            r["kept"] = r["column_days_per_s"] / rate
            if r["stride"] and r.get("analyses"):
                key = "shard_ms_per_analysis" if r["shard"] else "window_ms_per_analysis" if r["offsets"] else "sm_ms_per_analysis" if r["sensors"] else "enkf_ms_per_analysis"
                r[key] = (r["other_ms"] - other) / r["analyses"]
    line = json.dumps({"members": args.members, "depth": args.depth, "days": args.days, "sigma_cm": args.sigma,
                       "localisation_cm": args.localisation, "spread_cm": args.spread_cm, "sensors_cm": depths,
                       "sensor_nodes": rec["nodes"].tolist(), "sm_sigma": args.sm_sigma, "method": args.method,
                       "relaxation": args.relaxation,
                       "runs": recs})
    print(line)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(line + "\n")


if __name__ == "__main__":
    main()
