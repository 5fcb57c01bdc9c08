"""What the noise field costs the EnKF (hc_set_enkf_noise_field): column-days/s of the bench-size ensemble with the
state-only EnKF and with the EnKF that also updates the members' base noise vectors, one analysis a day, one handle each,
back to back on one GPU.

    python tools/enkf_noise_cost.py [--members 262144] [--depth 300] [--days 30] [--warmup 1] [--runs 48,48n,48,48n]
                                    [--sigma 10] [--localisation 0] [--spread-cm 0] [--method stochastic|sqrt]
                                    [--relaxation 0] [--noise-relaxation 0.5] [--json out.json]

Same set-up as tools/enkf_sm_cost.py and bench.py's timed region: synthetic 10-year forcing, Philox noise, the shared
initial condition of the well's digest (tests/golden/g1_tables_<depth>.npz where it exists, else the hydrostatic
profile), W warm-up days, then K timed days, the library's own launch length.  The timed figure is wall time around
hc_step_rows: the step launches and everything behind them.  `step_kernel_ms` is the step kernel alone (HIP events around
its launches), `other_ms` = wall - step kernel what the rest costs.  A run is a stride (48: the state-only EnKF, the
yardstick; 0: no EnKF) or a stride with the suffix "n" (the noise field on: a Philox run then takes the caller-noise path,
which shows in `step_kernel_ms`, and the analysis takes its passes over z, which shows in `other_ms`); list a run more than
once to alternate.  `kept` is a run's rate over the mean of the state-only runs of the same stride;
`noise_ms_per_analysis` and `step_ms_per_day_lost` attribute the difference.  Under `rocprofv3 --kernel-trace --stats`
run it with --runs 48n --days 1 --warmup 0 for the per-kernel time of the analyses.  Prints one JSON line.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def run(cols, forcing, psi0, members, stride, noise_field, sigma, loc, warmup_days, days, spread_cm=0.0, seed=2024,
        method="stochastic", relaxation=0.0, noise_relaxation=0.5):
    from hydromodel_amd.stepper import EnsembleStepper, enkf_noise_summary, enkf_summary
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
        if stride and (method, relaxation) != ("stochastic", 0.0):
            st.set_enkf_method(method, relaxation)
        if stride and noise_field:
            st.set_enkf_noise_field(True, noise_relaxation)
        row = 1
        if warmup_days:
            st.step_rows(row, 48 * warmup_days)
            row += 48 * warmup_days
        st.lib.hc_synchronize(st.h)
        t0 = time.perf_counter()
        out = st.step_rows(row, 48 * days)
        st.lib.hc_synchronize(st.h)
        wall = time.perf_counter() - t0
        rec = {"stride": stride, "noise_field": bool(stride and noise_field), "wall_s": wall,
               "step_kernel_ms": out["kernel_ms"], "launches": out["launches"], "other_ms": 1e3 * wall - out["kernel_ms"],
               "column_days_per_s": members * days / wall}
        if stride:
            s = enkf_summary(st.enkf_table()[0], stride, sigma)
            timed = s["rows"] >= row
            rec["analyses"] = int(timed.sum())
            rec["prior_std_cm_median"] = float(np.median(s["prior_std_cm"][timed])) if timed.any() else None
            rec["rejected"] = int(s["rejected"].sum())
        if stride and noise_field:
            n = enkf_noise_summary(st.enkf_noise_table()[0], stride, noise_relaxation)
            rec["noise_spread_ratio"] = n["noise_spread_ratio"]
            rec["noise_rejected"] = int(n["noise_rejected"].sum())
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
    ap.add_argument("--runs", default="48,48n,48,48n")
    ap.add_argument("--sigma", type=float, default=10.0)
    ap.add_argument("--localisation", type=float, default=0.0)
    ap.add_argument("--spread-cm", type=float, default=0.0)
    ap.add_argument("--method", default="stochastic", choices=("stochastic", "sqrt"))
    ap.add_argument("--relaxation", type=float, default=0.0)
    ap.add_argument("--noise-relaxation", type=float, default=0.5)
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
    recs = [run(cols, forcing, psi0, args.members, int(s.rstrip("n")), "n" in s, args.sigma, args.localisation, args.warmup,
                args.days, args.spread_cm, method=args.method, relaxation=args.relaxation,
                noise_relaxation=args.noise_relaxation) for s in args.runs.split(",")]
    for r in recs:
        base = [b for b in recs if b["stride"] == r["stride"] and not b["noise_field"]]
        if not base or not r["stride"]:
            continue
        rate = float(np.mean([b["column_days_per_s"] for b in base]))
        r["kept"] = r["column_days_per_s"] / rate
        if r["noise_field"] and r.get("analyses"):
            r["noise_ms_per_analysis"] = (r["other_ms"] - float(np.mean([b["other_ms"] for b in base]))) / r["analyses"]
            r["step_ms_per_day_lost"] = (r["step_kernel_ms"] - float(np.mean([b["step_kernel_ms"] for b in base]))) / args.days
    line = json.dumps({"members": args.members, "depth": args.depth, "days": args.days, "sigma_cm": args.sigma,
                       "localisation_cm": args.localisation, "spread_cm": args.spread_cm, "method": args.method,
                       "relaxation": args.relaxation, "noise_relaxation": args.noise_relaxation, "runs": recs})
    print(line)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(line + "\n")


if __name__ == "__main__":
    main()
