"""What perturbed forcing costs and buys (hc_set_forcing_perturbation).

    python tools/forcing_perturbation_cost.py [--members 262144] [--depth 300] [--days 30] [--warmup 1] [--runs p,z,f,p,z,f]
                                              [--sigmas 0.3,0.1] [--tau 3] [--json out.json]
    python tools/forcing_perturbation_cost.py --spread [--members 4096] [--depth 300] [--days 30]

Cost (default): column-days/s of the bench-size ensemble, one handle per run, back to back on one GPU, with the set-up of
tools/noise_correlation_cost.py and bench.py's timed region (synthetic 10-year forcing, Philox noise, the shared initial
condition of the well's digest, W warm-up days, then K timed days, the library's own launch length; wall time around
hc_step_rows).  A run is "p" (the feature off: the monitoring-mode build, the yardstick), "z" (on with both sigma = 0: the
build with the predictive branch and the two products, every factor 1.0 -- the cost of the wider build and of the fill) or
"f" (on with --sigmas and --tau: the cost of the spread on top, e.g. more failed attempts); list a run more than once to
alternate.  `kept` is a run's rate over the mean of the plain runs.  Under `rocprofv3 --kernel-trace --stats` run it with
--runs f --days 2 --warmup 0 for forcing_factor_fill_kernel next to the step kernel.
--spread: the forecast spread of the water table -- the ensemble's sigma (cm), its mean over the solved rows of --days and
on the last of them, free runs from one shared initial state -- without the feature and with it.  Prints one JSON line.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def start(cols, forcing, psi0, members, kind, sigmas, tau, seed=2024):
    from hydromodel_amd.stepper import EnsembleStepper
    st = EnsembleStepper(cols, forcing, members)
    st.set_state(psi0)
    st.set_noise_philox(seed, 0)
    if kind == "z":
        st.set_forcing_perturbation(0.0, 0.0, tau, seed)
    elif kind == "f":
        st.set_forcing_perturbation(sigmas[0], sigmas[1], tau, seed)
    return st


def run(cols, forcing, psi0, members, kind, sigmas, tau, warmup_days, days):
    st = start(cols, forcing, psi0, members, kind, sigmas, tau)
    try:
        row = 1
        if warmup_days:
            st.step_rows(row, 48 * warmup_days)
            row += 48 * warmup_days
        st.lib.hc_synchronize(st.h)
        before = st.counters()["failed_attempts"]
        t0 = time.perf_counter()
        out = st.step_rows(row, 48 * days)
        st.lib.hc_synchronize(st.h)
        wall = time.perf_counter() - t0
        return {"kind": kind, "wall_s": wall, "step_kernel_ms": out["kernel_ms"], "launches": out["launches"],
                "other_ms": 1e3 * wall - out["kernel_ms"], "column_days_per_s": members * days / wall,
                "failed_per_member_day": (st.counters()["failed_attempts"] - before) / (members * days)}
    finally:
        st.close()


def spread(cols, forcing, psi0, members, days, sigmas, tau):
    from hydromodel_amd.stepper import moments_to_mean_std
    out = []
    for kind in ("p", "f"):
        st = start(cols, forcing, psi0, members, kind, sigmas, tau)
        try:
            st.step_rows(1, 48 * days)
            mean, std = moments_to_mean_std(st.moments(), cols.dz, cols.z[0])
            rows = np.flatnonzero(np.asarray(forcing.wtd_obs[:48 * days + 1]) >= 0)
            rows = rows[rows >= 1]
            out.append({"kind": kind, "wtd_std_cm_last": float(std[rows[-1]]), "wtd_mean_cm_last": float(mean[rows[-1]]),
                        "wtd_std_cm_mean": float(np.mean(std[rows])), "wtd_std_cm_max": float(np.max(std[rows]))})
        finally:
            st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=None)
    ap.add_argument("--depth", type=int, default=300)
    ap.add_argument("--days", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--years", type=int, default=10)
    ap.add_argument("--runs", default="p,z,f,p,z,f")
    ap.add_argument("--sigmas", default="0.3,0.1")
    ap.add_argument("--tau", type=float, default=3.0)
    ap.add_argument("--spread", action="store_true")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    from hydromodel_amd.digest import ColumnTables, ForcingDigest
    from hydromodel_amd.ensemble import pressure_head
    from hydromodel_amd.synthetic import default_parameters, synthetic_forcing_frame, synthetic_well
    params = default_parameters()
    cols = ColumnTables(params, synthetic_well(args.depth))
    forcing = ForcingDigest(params, synthetic_forcing_frame(1 if args.spread else args.years), cols)
    fixture = REPO / "tests" / "golden" / f"g1_tables_{args.depth}.npz"
    psi0 = np.load(fixture)["initial_cond"] if fixture.exists() else pressure_head(cols, cols.por_raw)[0]
    sigmas = [float(x) for x in args.sigmas.split(",")]
    members = args.members or (4096 if args.spread else 262144)
    if args.spread:
        line = {"mode": "spread", "members": members, "depth": args.depth, "days": args.days, "sigmas": sigmas, "tau": args.tau,
                "runs": spread(cols, forcing, psi0, members, args.days, sigmas, args.tau)}
    else:
        recs = [run(cols, forcing, psi0, members, k, sigmas, args.tau, args.warmup, args.days) for k in args.runs.split(",")]
        plain = [r["column_days_per_s"] for r in recs if r["kind"] == "p"]
        for r in recs:
            if plain:
                r["kept"] = r["column_days_per_s"] / float(np.mean(plain))
        line = {"mode": "cost", "members": members, "depth": args.depth, "days": args.days, "sigmas": sigmas, "tau": args.tau,
                "runs": recs}
    line = json.dumps(line)
    print(line)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(line + "\n")


if __name__ == "__main__":
    main()
