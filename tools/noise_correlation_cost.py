"""What a vertical correlation of the noise fields costs and buys (hc_set_noise_correlation).

    python tools/noise_correlation_cost.py [--members 262144] [--depth 300] [--days 30] [--warmup 1] [--runs p,c,p,c]
                                           [--length 50] [--json out.json]
    python tools/noise_correlation_cost.py --spread [--members 256] [--days 10] [--lengths 25,50,100]
    python tools/noise_correlation_cost.py --twin [--members 256] [--days 10] [--length 50]

Cost (default): column-days/s of the bench-size ensemble, one handle per run, back to back on one GPU, with the set-up of
tools/enkf_noise_cost.py and bench.py's timed region (synthetic 10-year forcing, Philox noise, the shared initial condition
of the well's digest, W warm-up days, then K timed days, the library's own launch length; wall time around hc_step_rows).
A run is "p" (plain in-kernel Philox, the yardstick), "c" (a correlation of --length cm with the layers' breaks: the handle
fills base and refresh vectors with noise_field_fill_kernel and runs the caller-noise path) or "f" (white vectors on the
same caller-noise path: a particle filter that never assimilates, stride past the run's rows, which fills them with
filter_philox_fill_kernel); list a run more than once to alternate.  `kept` is a run's rate over the mean of the plain runs.
Under `rocprofv3 --kernel-trace --stats` run it with --runs f,c --days 2 --warmup 0 for the two fill kernels side by side.
--spread: the ensemble's water-table sigma (cm) on the last row of --days on well 1 from one shared initial state, white
against each of --lengths (with the layers' breaks).  --twin: LAB_NOTES 28's twin experiment (well 1, +-60 cm offsets, the
truth at +35 cm with its own seed, sigma = 2 dz, noise-field relaxation 0.5) white and with --length, the truth's field
drawn like the members'.  Prints one JSON line.
"""
import argparse
import copy
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
WELL_1 = {"soil": 0.0, "saprolite": 50.0, "weathered": 200.0, "max_depth": 500.0, "sat_depth": 100.0}


def tables(cols, length):
    from hydromodel_amd.stepper import noise_correlation_breaks, noise_correlation_tables
    return noise_correlation_tables(cols.z, length, noise_correlation_breaks(cols.layers, cols.z))


def run(cols, forcing, psi0, members, kind, length, warmup_days, days, seed=2024):
    from hydromodel_amd.stepper import EnsembleStepper
    st = EnsembleStepper(cols, forcing, members)
    try:
        st.set_state(psi0)
        st.set_noise_philox(seed, 0)
        if kind == "c":
            st.set_noise_correlation(*tables(cols, length))
        elif kind == "f":
            st.set_filter(48 * (warmup_days + days) + 1, 1e30, seed)
        row = 1
        if warmup_days:
            st.step_rows(row, 48 * warmup_days)
            row += 48 * warmup_days
        st.lib.hc_synchronize(st.h)
        t0 = time.perf_counter()
        out = st.step_rows(row, 48 * days)
        st.lib.hc_synchronize(st.h)
        wall = time.perf_counter() - t0
        return {"kind": kind, "wall_s": wall, "step_kernel_ms": out["kernel_ms"], "launches": out["launches"],
                "other_ms": 1e3 * wall - out["kernel_ms"], "refresh_rows": st.n_refresh(row, 48 * days),
                "column_days_per_s": members * days / wall}
    finally:
        st.close()


def spread(cols, forcing, psi0, members, days, lengths, seed=2024):
    from hydromodel_amd.stepper import EnsembleStepper, moments_to_mean_std
    out = []
    for length in [0.0] + list(lengths):
        st = EnsembleStepper(cols, forcing, members)
        try:
            st.set_state(psi0)
            st.set_noise_philox(seed, 0)
            if length:
                st.set_noise_correlation(*tables(cols, length))
            stats = st.step_rows(1, 48 * days, want_stats=True)
            mean, std = moments_to_mean_std(st.moments(), cols.dz, cols.z[0])
            rows = np.flatnonzero(np.asarray(forcing.wtd_obs[:48 * days + 1]) >= 0)
            out.append({"length_cm": length, "wtd_std_cm_last": float(std[rows[-1]]), "wtd_mean_cm_last": float(mean[rows[-1]]),
                        "wtd_std_cm_mean": float(np.mean(std[rows[rows >= 1]])),
                        "failed_per_member_day": float(stats["failed"].sum()) / (members * days)})
        finally:
            st.close()
    return out


def twin(cols, forcing, psi0, members, days, length):
    from hydromodel_amd.stepper import EnsembleStepper, noise_correlate, split_enkf_noise_table, wtd_distribution
    rows = 48 * days
    shifts = np.random.default_rng(12).uniform(-60.0, 60.0, size=members)
    layered = np.flatnonzero(np.asarray(cols.noisec_node) >= 0)
    out = []
    for ell in (0.0, length):
        truth = EnsembleStepper(cols, forcing, 1)
        try:
            truth.set_state(psi0 + 35.0)
            truth.set_noise_philox(999, 0)
            z_truth = truth.philox_normals(0, 0)
            if ell:
                a, b = tables(cols, ell)
                truth.set_noise_correlation(a, b)
                z_truth = noise_correlate(z_truth, a, b)
            w_truth = truth.step_rows(1, rows, want_wtd=True)["wtd"][:, 0]
        finally:
            truth.close()
        obs = np.array(forcing.wtd_obs, dtype=np.int32)
        obs[1:rows + 1] = np.where(obs[1:rows + 1] >= 0, w_truth, -1)
        obs[rows + 1:] = -1
        record = copy.copy(forcing)
        record.wtd_obs = obs
        for field in (False, True):
            st = EnsembleStepper(cols, record, members)
            try:
                st.set_state(psi0[None, :] + shifts[:, None])
                st.set_noise_philox(4, 0)
                if ell:
                    st.set_noise_correlation(*tables(cols, ell))
                st.set_wtd_hist(48)
                st.set_enkf(48, 2.0 * cols.dz, 0.0, 17)
                if field:
                    st.set_enkf_noise_field(True, 0.5)
                st.step_rows(1, rows)
                hist = st.wtd_hist_table()[0]
                r = {"length_cm": ell, "noise_field": field,
                     "crps_cm": float(wtd_distribution(hist, obs, (0.5,), cols.dz, cols.z, 0, 48)["crps_mean_cm"])}
                if field:
                    stats, rej = split_enkf_noise_table(st.enkf_noise_table()[0], cols.dim_d)
                    done = np.flatnonzero(np.isfinite(rej))
                    r.update(analyses=int(done.size), rejected=int(rej[done].sum()),
                             rmse_before=float(np.sqrt(np.mean((stats[done[0], 0] - z_truth)[layered] ** 2))),
                             rmse_after=float(np.sqrt(np.mean((stats[done[-1], 2] - z_truth)[layered] ** 2))),
                             spread_ratio=float(np.mean(stats[done, 3][:, layered] / stats[done, 1][:, layered])))
                out.append(r)
            finally:
                st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=None)
    ap.add_argument("--depth", type=int, default=300)
    ap.add_argument("--days", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--years", type=int, default=10)
    ap.add_argument("--runs", default="p,c,p,c")
    ap.add_argument("--length", type=float, default=50.0)
    ap.add_argument("--lengths", default="25,50,100")
    ap.add_argument("--spread", action="store_true")
    ap.add_argument("--twin", action="store_true")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    from hydromodel_amd.digest import ColumnTables, ForcingDigest
    from hydromodel_amd.ensemble import pressure_head
    from hydromodel_amd.synthetic import default_parameters, synthetic_forcing_frame, synthetic_well
    params = default_parameters()
    small = args.spread or args.twin
    cols = ColumnTables(params, WELL_1 if small else synthetic_well(args.depth))
    forcing = ForcingDigest(params, synthetic_forcing_frame(1 if small else args.years), cols)
    fixture = REPO / "tests" / "golden" / f"g1_tables_{1 if small else args.depth}.npz"
    psi0 = np.load(fixture)["initial_cond"] if fixture.exists() else pressure_head(cols, cols.por_raw)[0]
    members = args.members or (256 if small else 262144)
    days = args.days or (10 if small else 30)
    if args.spread:
        line = {"mode": "spread", "members": members, "days": days,
                "runs": spread(cols, forcing, psi0, members, days, [float(x) for x in args.lengths.split(",")])}
    elif args.twin:
        line = {"mode": "twin", "members": members, "days": days, "runs": twin(cols, forcing, psi0, members, days, args.length)}
    else:
        recs = [run(cols, forcing, psi0, members, k, args.length, args.warmup, days) for k in args.runs.split(",")]
        plain = [r["column_days_per_s"] for r in recs if r["kind"] == "p"]
        for r in recs:
            if plain:
                r["kept"] = r["column_days_per_s"] / float(np.mean(plain))
        line = {"mode": "cost", "members": members, "depth": args.depth, "days": days, "length_cm": args.length, "runs": recs}
    line = json.dumps(line)
    print(line)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(line + "\n")


if __name__ == "__main__":
    main()
