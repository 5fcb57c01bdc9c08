"""What the ensemble Kalman filter costs (hc_set_enkf): column-days/s of the bench-size ensemble without the EnKF and with
analyses every 48th row (one a day), one handle each, back to back on one GPU.

    python tools/enkf_cost.py [--members 262144] [--depth 300] [--days 30] [--warmup 1] [--strides 0,48]
                              [--sigma 10] [--localisation 0] [--spread-cm 0] [--json out.json]

Same set-up as tools/filter_cost.py and bench.py's timed region: synthetic 10-year forcing, Philox noise, the shared
initial condition of the well's digest (tests/golden/g1_tables_<depth>.npz where it exists, else the hydrostatic profile),
W warm-up days, then K timed days, the library's own launch length.  The timed figure is wall time around hc_step_rows:
the step launches AND everything behind them -- with the EnKF, the observation, reduction, gain and update kernels.
`step_kernel_ms` is the step kernel alone (HIP events around its launches), so `other_ms` = wall - step kernel is what the
rest costs; `enkf_ms_per_analysis` is the EnKF run's `other_ms` over the plain one's, per analysis.  A stride may be
listed more than once (e.g. 0,48,0,48 to alternate); `kept` is a run's rate over the mean of the stride-0 runs.
--spread-cm W starts every member from the initial profile shifted by its own offset, uniform over +-W cm.  Prints one
JSON line.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def run(cols, forcing, psi0, members, stride, sigma, loc, warmup_days, days, spread_cm=0.0, seed=2024):
    from hydromodel_amd.stepper import EnsembleStepper, enkf_summary
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
               "other_ms": 1e3 * wall - out["kernel_ms"], "column_days_per_s": members * days / wall}
        if stride:
            s = enkf_summary(st.enkf_table()[0], stride, sigma)
            timed = s["rows"] >= row
            rec["analyses"] = int(timed.sum())
            rec["prior_std_cm_median"] = float(np.median(s["prior_std_cm"][timed])) if timed.any() else None
            rec["post_std_cm_median"] = float(np.median(s["post_std_cm"][timed])) if timed.any() else None
            rec["rejected"] = int(s["rejected"].sum())
            rec["loglik"] = s["loglik"]
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
    ap.add_argument("--localisation", type=float, default=0.0)
    ap.add_argument("--spread-cm", type=float, default=0.0)
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
    recs = [run(cols, forcing, psi0, args.members, int(s), args.sigma, args.localisation, args.warmup, args.days,
                args.spread_cm)
            for s in args.strides.split(",")]
    base = [r for r in recs if r["stride"] == 0]
    if base:
        rate = float(np.mean([r["column_days_per_s"] for r in base]))
        other = float(np.mean([r["other_ms"] for r in base]))
        for r in recs:
            r["kept"] = r["column_days_per_s"] / rate
            if r["stride"] and r.get("analyses"):
                r["enkf_ms_per_analysis"] = (r["other_ms"] - other) / r["analyses"]
    line = json.dumps({"members": args.members, "depth": args.depth, "days": args.days, "sigma_cm": args.sigma,
                       "localisation_cm": args.localisation, "spread_cm": args.spread_cm,
                       "runs": recs})
    print(line)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(line + "\n")


if __name__ == "__main__":
    main()
