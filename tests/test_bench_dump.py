"""bench.py --dump-outputs on the host side (no GPU): which members are written, in which dtype, how much, and the rows of
the last step.  The end-to-end run on the GPU is in tests/test_gpu_bench.py."""
import subprocess
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent


class _Stepper:
    """The two reads dump_outputs makes of an EnsembleStepper, over host arrays."""

    def __init__(self, n, d):
        self.N, self.D = n, d
        self.psi = np.arange(n * d, dtype=np.float64).reshape(n, d)
        self.scale = 0.8 ** (np.arange(n) % 3)

    def get_state(self, first=0, count=None):
        return self.psi[first:first + count].copy()

    def noise_scale(self, first=0, count=None):
        return self.scale[first:first + count].copy()


def _moments(T, n):
    rng = np.random.default_rng(3)
    idx = rng.integers(10, 60, size=(T, 7))
    return np.stack([np.full(T, n), idx.sum(axis=1), (idx ** 2).sum(axis=1)]).astype(np.int64)


def _load(d):
    return {p.stem: np.load(p) for p in sorted(Path(d).glob("*.npy"))}


def test_dump_writes_the_last_step_of_a_small_ensemble_whole(tmp_path):
    import bench
    st, T = _Stepper(100, 30), 1 + 3 * bench.ROWS_PER_DAY
    m = _moments(T, 100)
    bench.dump_outputs(tmp_path, st, T - bench.ROWS_PER_DAY, m, 5.0, 0.0)
    out = _load(tmp_path)
    assert sorted(out) == ["noise_scale", "psi", "wtd_mean_cm", "wtd_moments", "wtd_std_cm"]
    assert all(a.dtype == np.float64 for a in out.values())
    assert np.array_equal(out["psi"], st.psi) and np.array_equal(out["noise_scale"], st.scale)
    assert np.array_equal(out["wtd_moments"], m[:, -bench.ROWS_PER_DAY:])
    assert np.allclose(out["wtd_mean_cm"], 5.0 * m[1, -bench.ROWS_PER_DAY:] / 100.0)
    assert out["wtd_std_cm"].shape == (bench.ROWS_PER_DAY,)


def test_dump_samples_a_large_ensemble_the_same_way_every_time(tmp_path):
    import bench
    n, D, T = 3 * bench.DUMP_MEMBERS + 5, 640, 1 + 2 * bench.ROWS_PER_DAY
    st = _Stepper(n, D)
    for run in ("a", "b"):
        bench.dump_outputs(tmp_path / run, st, 1 + bench.ROWS_PER_DAY, _moments(T, n), 5.0, 0.0)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    psi = a["psi"]
    assert psi.shape == (bench.DUMP_MEMBERS, D)
    ids = psi[:, 0] / D                                    # row k of the fake state starts with k * D
    assert np.all(np.diff(ids) > 0) and ids[-1] < n and ids[-1] > 2 * bench.DUMP_MEMBERS
    assert np.array_equal(a["noise_scale"], st.scale[ids.astype(np.int64)])
    size = sum(p.stat().st_size for p in (tmp_path / "a").glob("*.npy"))
    assert size <= 64 << 20


def test_dump_of_a_sweep_keeps_the_points(tmp_path):
    import bench
    P, M, T = 4, 16, 1 + 2 * bench.ROWS_PER_DAY
    m = np.stack([_moments(T, M) for _ in range(P)])
    bench.dump_outputs(tmp_path, _Stepper(P * M, 20), 1 + bench.ROWS_PER_DAY, m, 5.0, 0.0)
    out = _load(tmp_path)
    assert out["wtd_moments"].shape == (P, 3, bench.ROWS_PER_DAY) and out["wtd_mean_cm"].shape == (P, bench.ROWS_PER_DAY)
    assert np.array_equal(out["wtd_moments"], m[:, :, -bench.ROWS_PER_DAY:])


def test_steps_below_one_are_refused():
    p = subprocess.run([sys.executable, "bench.py", "--steps", "0"], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--steps must be >= 1" in p.stderr


def test_the_extra_legs_wait_for_full():
    """A plain run is the headline alone; --full asks for the legs after it."""
    import bench
    assert bench.parse([]).full is False
    assert bench.parse(["--full"]).full is True
