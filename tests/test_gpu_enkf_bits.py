"""The EnKF's results to the bit, across commits: SHA-1 digests of the raw bytes of the states, the tables, the gains
and the relaxation arrays after one or two analyses, against tests/golden/enkf_bits.json.

The other EnKF tests compare configurations within one build (sharded against unsharded, launch lengths, NumPy to
1e-13); this one pins the build itself.  Every floating-point operation of the analysis runs with contraction off and in
an order fixed by the member count alone, so a change to the kernels that keeps the arithmetic keeps these digests.  A
mismatch is a failure of the change, never a reason to record again.

The file was written by this module on the commit its header names:

    python tests/test_gpu_enkf_bits.py --record --commit <hash> [--out <file>]
"""
import hashlib
import json
import sys
import time
from pathlib import Path

import numpy as np
import pytest
import torch  # (before the library, as in test_gpu_enkf_shard)

if __name__ == "__main__":                                            # run as a script: the recorder
    sys.path[:0] = [str(Path(__file__).resolve().parent), str(Path(__file__).resolve().parent.parent)]

from helpers import GOLDEN, digest, golden
from test_gpu_enkf_shard import NODES, VALUES, _record, _spread

pytestmark = pytest.mark.gpu

BITS = GOLDEN / "enkf_bits.json"
NOISE_SEED, ENKF_SEED = 7, 3
WINDOW, LOCALISATION_CM = (12, 24), 50.0

# name -> (well, points, members per point, rows, stride, method, relaxation, observations)
# observations: "well" (the well alone), "sensors" (three sensors at NODES), "window" (offsets WINDOW, localised)
CASES = {}
for _method in ("stochastic", "sqrt"):
    for _alpha in (0.0, 0.5):
        for _obs in ("well", "sensors", "window"):
            # one point of 1000 members: 4 tiles of 256, the last holds 232; D = 200 = 3 * 64 + 8, a partial last slot
            CASES[f"one-{_method}-a{_alpha:g}-{_obs}"] = (200, 1, 1000, 96, 48, _method, _alpha, _obs)
# three points of 300 members: 2 tiles each, the last holds 44; the only cases with a second point (blockIdx.y > 0)
CASES["three-sqrt-a0.5-sensors"] = (200, 3, 300, 96, 48, "sqrt", 0.5, "sensors")
CASES["three-stochastic-a0.5-window"] = (200, 3, 300, 96, 48, "stochastic", 0.5, "window")
# one deep column (D = 581: every slot of the wave-per-member update), one analysis
CASES["deep-stochastic-a0.5-well"] = (581, 1, 300, 48, 48, "stochastic", 0.5, "well")


def _sha1(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def _digests(case):
    """Run ``case`` and digest everything its analyses left behind."""
    from hydromodel_amd.stepper import EnsembleStepper
    well, P, mpp, rows, stride, method, alpha, obs = CASES[case]
    _, cols, forcing = digest(well)
    st = EnsembleStepper([cols] * P if P > 1 else cols, forcing, P * mpp)
    try:
        st.set_state(_spread(golden(f"g1_tables_{well}.npz")["initial_cond"], P * mpp))
        st.set_noise_philox(NOISE_SEED, 0)
        st.set_enkf(stride, 2.0 * cols.dz, LOCALISATION_CM if obs == "window" else 0.0, ENKF_SEED)
        if obs == "sensors":
            st.set_enkf_soil_moisture(NODES, _record(st.T, NODES, VALUES, rows=(48, 96)), 0.02)
        st.set_enkf_method(method, alpha)
        if obs == "window":
            st.set_enkf_window(WINDOW)
        st.step_rows(1, rows)
        table = st.enkf_table()
        assert np.all(table[:, 1:rows // stride + 1, 0] == mpp), case           # every analysis took every member
        out = dict(psi=st.get_state(), table=table, gain=st.enkf_gain(), full_gain=st.enkf_full_gain(),
                   moments=np.asarray(st.moments()))
        if obs == "sensors":
            out["sm"] = st.enkf_sm_table()
        if obs == "window":
            out["win"] = st.enkf_window_table()
        if method == "sqrt":
            out["sqrt_gain"], out["sqrt_shift"] = st.enkf_sqrt_gain(), st.enkf_sqrt_shift()
        if alpha > 0.0:
            out["sigma_b"], out["sigma_a"], out["relax_f"] = st.enkf_relaxation_factors()
    finally:
        st.close()
    return {k: _sha1(v) for k, v in out.items()}


@pytest.mark.parametrize("case", list(CASES))
def test_bits_are_those_recorded(case):
    doc = json.loads(BITS.read_text())
    recorded = doc["cases"]
    assert case in recorded, f"{BITS.name} holds no digests of {case}"
    got = _digests(case)
    assert sorted(got) == sorted(recorded[case])
    differ = [k for k in got if got[k] != recorded[case][k]]
    # (a compiler that lowers a division or a square root differently would show here too: the versions tell which)
    assert not differ, (f"{case}: {differ} differ from the digests recorded at commit {doc['recorded_at_commit'][:12]} "
                        f"with ROCm {doc['rocm']}; this build runs ROCm {torch.version.hip}")


def record(commit, out=BITS):
    """Write the digests of every case, with the commit and the ROCm they were recorded at."""
    cases = {}
    for case in CASES:
        t0 = time.perf_counter()
        cases[case] = _digests(case)
        print(f"{case}: {time.perf_counter() - t0:.2f} s", flush=True)
    doc = {"recorded_at_commit": commit, "rocm": torch.version.hip, "device": torch.cuda.get_device_name(0),
           "what": "SHA-1 of the raw bytes of each array, tests/test_gpu_enkf_bits.py", "cases": cases}
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(doc, indent=1, sort_keys=True) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--record", action="store_true", required=True)
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", default=str(BITS))
    a = ap.parse_args()
    record(a.commit, a.out)
