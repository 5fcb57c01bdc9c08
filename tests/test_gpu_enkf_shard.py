"""One point's members on several handles (include/hydrocol.h hc_set_enkf_shard): the analyses of 2 and 3 handles that
share an ensemble of 1000 members are those of the one handle that holds them all, to the bit -- states, the EnKF's, the
sensors' and the window's tables, the gains; a handle that holds every member is the unsharded run; the refusals; a
failing callback; the CLI's ``"Sharded": true`` on two ranks against one.

The handles of a test share one card and one process: one thread per handle (ctypes releases the GIL), and the exchange
is a barrier, device copies between the handles' buffers, a barrier.  Every join and barrier has a timeout, so a
mismatch in the calls fails the test instead of hanging it."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: a shard's buffer is torch's, one HIP runtime serves both)

from helpers import GOLDEN, digest, golden
from helpers import cli_params as _cli_params
from test_gpu_enkf import _spread
from test_gpu_enkf_sm import _record, _sensor_csv

pytestmark = pytest.mark.gpu

N, WELL, ROWS, STRIDE, SEED = 1000, 200, 96, 48, 7
NODES, VALUES = [6, 20, 45], [0.22, 0.26, 0.2]

# (method, relaxation, sensors, window offsets, localisation cm)
CASES = {"stochastic-well": ("stochastic", 0.0, False, (), 0.0),
         "three-sensors": ("stochastic", 0.0, True, (), 0.0),
         "sqrt-relaxed": ("sqrt", 0.5, False, (), 0.0),
         "window-localised": ("stochastic", 0.0, False, (12, 24), 50.0)}


class CardExchange:
    """The gather between ``n`` handles of one process: handle k's callable publishes its view and word range, waits for
    the others, copies their ranges out of their buffers into its own, and waits again (nobody overwrites a buffer that
    is still being read)."""

    def __init__(self, n, timeout=120.0):
        self.n, self.posts = n, [None] * n
        self.barrier = threading.Barrier(n, timeout=timeout)
        self.calls = [0] * n

    def of(self, k):
        import torch

        def exchange(block, first, count):
            self.calls[k] += 1
            self.posts[k] = (block, first, count)
            self.barrier.wait()
            for j, (theirs, f, c) in enumerate(self.posts):
                assert theirs.numel() == block.numel(), "the handles are in different passes"
                if j != k and c:
                    block[f:f + c].copy_(theirs[f:f + c])
            torch.cuda.synchronize()
            self.barrier.wait()
        return exchange


def _handle(lo, hi, case, exchange="unsharded", n_global=N, well=WELL):
    """Members [lo, hi) of the ensemble of ``n_global``, set up as ``case`` says; ``exchange`` = "unsharded": no
    hc_set_enkf_shard."""
    from hydromodel_amd.stepper import EnsembleStepper
    method, alpha, sensors, window, loc = CASES[case]
    _, cols, forcing = digest(well)
    st = EnsembleStepper(cols, forcing, hi - lo)
    st.set_state(_spread(golden(f"g1_tables_{well}.npz")["initial_cond"], n_global)[lo:hi])
    st.set_noise_philox(SEED, lo)
    st.set_enkf(STRIDE, 2.0 * cols.dz, loc, 3)
    if sensors:
        st.set_enkf_soil_moisture(NODES, _record(st.T, NODES, VALUES, rows=(48, 96)), 0.02)
    st.set_enkf_method(method, alpha)
    if window:
        st.set_enkf_window(window)
    if exchange != "unsharded":
        st.set_enkf_shard(n_global, lo, exchange)
    return st


def _results(st, case):
    sensors, window = CASES[case][2], CASES[case][3]
    out = dict(psi=st.get_state(), table=st.enkf_table(), gain=st.enkf_gain(), full_gain=st.enkf_full_gain(),
               moments=np.asarray(st.moments()))
    if sensors:
        out["sm"] = st.enkf_sm_table()
    if window:
        out["win"] = st.enkf_window_table()
    return out


def _run_together(bounds, case, rows=ROWS, n_global=N, well=WELL, look=None):
    """One handle per block of ``bounds`` stepping ``rows`` rows at once; every handle's results, in block order.
    ``look(handles)`` is called before they step."""
    card = CardExchange(len(bounds))
    handles = [_handle(lo, hi, case, card.of(k), n_global, well) for k, (lo, hi) in enumerate(bounds)]
    if look:
        look(handles)
    failures = [None] * len(bounds)

    def work(k):
        try:
            handles[k].step_rows(1, rows)
        except BaseException as e:  # noqa: BLE001
            failures[k] = e
            card.barrier.abort()                                    # the others must not wait for this one
    try:
        threads = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(len(bounds))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=600)
        assert not any(t.is_alive() for t in threads), "a handle's step did not return"
        assert failures == [None] * len(bounds), failures
        assert len(set(card.calls)) == 1 and card.calls[0] > 0      # every handle made the same calls
        return [_results(st, case) for st in handles], card.calls[0]
    finally:
        for st in handles:
            st.close()


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 1. bit equality --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_two_and_three_handles_analyse_like_one(case):
    whole = _handle(0, N, case)
    try:
        whole.step_rows(1, ROWS)
        ref = _results(whole, case)
    finally:
        whole.close()
    assert ref["table"][0, 1, 0] == N and ref["table"][0, 2, 0] == N           # both rows were analysed
    for bounds in ([(0, 512), (512, 1000)], [(0, 256), (256, 768), (768, 1000)]):
        got, calls = _run_together(bounds, case)
        # per analysis: prior sums, prior products, posterior sums and products; relaxation: sigma_b, the first member's
        # column, the analysis mean, sigma_a
        assert calls == 2 * (8 if CASES[case][1] > 0 else 4)
        assert _bits(np.concatenate([g["psi"] for g in got]), ref["psi"]), (case, bounds)
        assert _bits(sum(g["moments"] for g in got), ref["moments"])
        for g in got:                                               # identical on every handle, and the one handle's
            for key in ("table", "gain", "full_gain", "sm", "win"):
                if key in ref:
                    assert _bits(g[key], ref[key]), (case, bounds, key)


# ---- 2. identity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["three-sensors", "sqrt-relaxed"])
def test_a_handle_that_holds_every_member_is_the_unsharded_run(case):
    runs = {}
    for tag, exchange in (("plain", "unsharded"), ("sharded", None)):
        st = _handle(0, N, case, exchange)
        try:
            assert st.get_enkf_shard() == ((N, 0) if tag == "sharded" else (0, 0))
            st.step_rows(1, ROWS)
            runs[tag] = _results(st, case)
        finally:
            st.close()
    for key in runs["plain"]:
        assert _bits(runs["plain"][key], runs["sharded"][key]), key


# ---- 3. refusals ------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    from hydromodel_amd import _lib as L
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(WELL)
    fn = L.EXCHANGE_FN(lambda *a: 0)
    buf = torch.zeros(1 << 20, dtype=torch.float64, device="cuda")

    def refused(st, n_global, first, n_words=None, match=""):
        words = buf.numel() if n_words is None else n_words
        rc = st.lib.hc_set_enkf_shard(st.h, n_global, first, buf.data_ptr(), words, fn, None)
        assert rc == -1 and match in st.lib.hc_last_error().decode(), st.lib.hc_last_error()       # HC_ERR_ARG
        assert st.get_enkf_shard() == (0, 0)

    st = EnsembleStepper(cols, forcing, 300)
    try:
        st.set_state(golden(f"g1_tables_{WELL}.npz")["initial_cond"])
        st.set_noise_philox(SEED, 0)
        refused(st, 1000, 0, match="EnKF is off")
        st.set_enkf(STRIDE, 5.0, 0.0, 1)
        refused(st, 1000, 0, match="multiple of 256")                   # 300 members, not the last shard
        refused(st, 300, 100, match="multiple of 256")                  # first_global = 100
        refused(st, 200, 0, match="outside")
        need = st.enkf_shard_words(300)
        assert need == 2 * ((cols.dim_d + 1) * 1 + cols.dim_d)
        refused(st, 300, 0, n_words=need - 1, match="needed")
        assert st.lib.hc_set_enkf_shard(st.h, 300, 0, buf.data_ptr(), need, fn, None) == 0
        assert st.get_enkf_shard() == (300, 0)
        st.set_enkf(STRIDE, 5.0, 0.0, 1)                                # whatever turns the EnKF off turns it off
        assert st.get_enkf_shard() == (0, 0)
        st.set_noise_philox(SEED, 256)
        st.set_enkf(STRIDE, 5.0, 0.0, 1)
        refused(st, 300, 0, match="hc_set_noise_philox")                # the members are keyed from 256
    finally:
        st.close()
    two = EnsembleStepper([cols, cols], forcing, 512)
    try:
        two.set_state(golden(f"g1_tables_{WELL}.npz")["initial_cond"])
        two.set_noise_philox(SEED, 0)
        two.set_enkf(STRIDE, 5.0, 0.0, 1)
        refused(two, 1024, 0, match="2 points")
    finally:
        two.close()


# ---- 4. the CLI -------------------------------------------------------------------------------------------------------
def _run_cli(tmp_path, name, params, gpus):
    from hydromodel_amd.simulation import loadResults
    d = tmp_path / name
    d.mkdir()
    (d / "p.json").write_text(json.dumps(dict(params, Output_Name=name)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    env.update(HYDROCOL_DIST_BACKEND="gloo", HYDROCOL_SHARE_DEVICE="1")
    cmd = ["timeout", "-k", "10", "600", sys.executable, str(GOLDEN.parent.parent / "berkeley_hydro_main.py"),
           "--params", str(d / "p.json")]
    if gpus > 1:
        cmd += ["--gpus", str(gpus)]
    r = subprocess.run(cmd, cwd=d, env=env, capture_output=True, text=True, timeout=660)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return loadResults(d / f"{name}_ensemble.h5"), r.stdout


def test_cli_sharded_on_two_ranks_writes_the_one_rank_file(tmp_path):
    params = _cli_params(tmp_path)
    sm = {"Filename": _sensor_csv(tmp_path, 3), "Depths_cm": [20, 60, 150], "Sigma": 0.02}
    params["Ensemble"] = {"Members": 1024, "Seed": 5, "Days": 4, "Distribution": {"Stride": 48},
                          "EnKF": {"Stride": 24, "Sigma_cm": 8.0, "Soil_Moisture": sm, "Sharded": True}}
    one, log1 = _run_cli(tmp_path, "run", params, 1)
    (tmp_path / "run").rename(tmp_path / "run_one")
    two, log2 = _run_cli(tmp_path, "run", params, 2)
    assert set(one) == set(two) and "enkf_sharded" in one and "enkf_sm_obs" in one
    assert int(one["gpus"]) == 1 and int(two["gpus"]) == 2
    for k in sorted(set(one) - {"gpus"}):
        a, b = np.asarray(one[k]), np.asarray(two[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert one["enkf_sharded"].dtype == np.int8 and int(one["enkf_sharded"]) == 1
    assert one["enkf_count"].tolist() == [1024] * one["enkf_rows"].size and one["enkf_rows"].size == 8
    closing = [[s for s in log.splitlines() if "log-likelihood" in s or "RMSE" in s or "CRPS" in s] for log in (log1, log2)]
    assert closing[0] == closing[1] and len(closing[0]) >= 2


# ---- 5. a failing callback --------------------------------------------------------------------------------------------
def test_a_failing_callback_fails_the_step_cleanly():
    from hydromodel_amd import _lib as L

    def broken(block, first, count):
        raise RuntimeError("the peer is gone")
    st = _handle(0, N, "stochastic-well", broken)
    try:
        a = L.StepArgs()
        a.row_begin, a.n_rows, a.accumulate_moments = 1, ROWS, 1
        rc = st.lib.hc_step_rows(st.h, C.byref(a))
        assert rc == -2 and "exchange callback returned 1" in st.lib.hc_last_error().decode()     # HC_ERR_DEVICE
        st._shard_error = None
    finally:
        st.close()
    assert st.h is None                                              # ... and the handle could be destroyed
    st = _handle(0, N, "stochastic-well", broken)
    try:
        with pytest.raises(L.HcError, match="exchange callback") as info:
            st.step_rows(1, ROWS)
        assert isinstance(info.value.__cause__, RuntimeError)        # the Python face keeps the callback's exception
    finally:
        st.close()
