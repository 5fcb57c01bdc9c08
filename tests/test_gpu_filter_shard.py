"""One point's members on several handles, particle filter (include/hydrocol.h hc_set_filter_shard): the assimilations of
2 and 3 handles that share an ensemble of 1000 members are those of the one handle that holds them all, to the bit --
states, base noise vectors, the filter's table, weights, draw and ancestry; every column routed, none routed; host noise;
a handle that holds every member is the unsharded run; the refusals; a failing callback; the CLI's ``"Sharded": true`` on
two ranks against one.

The handles of a test share one card and one process: one thread per handle (ctypes releases the GIL), and the exchange
is a barrier, device copies between the handles' buffers, a barrier.  Every join and barrier has a timeout, so a
mismatch in the calls fails the test instead of hanging it."""
import ctypes as C
import threading
import time

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: a shard's buffer is torch's, one HIP runtime serves both)

from helpers import digest, golden
from helpers import cli_params as _cli_params
from test_gpu_enkf import _spread
from test_gpu_enkf_shard import _bits, _run_cli

pytestmark = pytest.mark.gpu

N, WELL, ROWS, STRIDE, SEED, FSEED = 1000, 200, 96, 48, 7, 3
TWO, THREE = [0, 512, 1000], [0, 300, 301, 1000]           # (THREE: a shard of one member)


class CardExchange:
    """The exchange between ``n`` handles of one process.  Handle k's gather publishes its view and word range, waits
    for the others, copies their ranges out of their buffers into its own, and waits again (nobody overwrites a buffer
    that is still being read); its route publishes its send region and counts, waits, copies the block every other
    handle packed for it into its receive region, and waits again."""

    def __init__(self, n, timeout=120.0):
        self.n, self.posts = n, [None] * n
        self.barrier = threading.Barrier(n, timeout=timeout)
        self.gathers, self.routes = [0] * n, [0] * n
        self.sent = [[] for _ in range(n)]             # per handle: the send counts of every routing call

    def of(self, k):
        card = self

        class Exchange:
            def __call__(self, block, first, count):
                card.gathers[k] += 1
                card.posts[k] = (block, first, count)
                card.barrier.wait()
                for j, (theirs, f, c) in enumerate(card.posts):
                    assert theirs.numel() == block.numel()
                    if j != k and c:
                        block[f:f + c].copy_(theirs[f:f + c])
                torch.cuda.synchronize()
                card.barrier.wait()

            def route(self, send, send_words, recv, recv_words):
                card.routes[k] += 1
                card.sent[k].append(list(send_words))
                card.posts[k] = (send, list(send_words))
                card.barrier.wait()
                at = 0
                for j, (theirs, words) in enumerate(card.posts):
                    assert words[k] == recv_words[j], "the two ends of a transfer disagree"
                    if j != k and words[k]:
                        skip = sum(words[:k])
                        recv[at:at + words[k]].copy_(theirs[skip:skip + words[k]])
                    at += recv_words[j]
                torch.cuda.synchronize()
                card.barrier.wait()
        return Exchange()


def _initial(kind, n=N, well=WELL):
    psi0 = golden(f"g1_tables_{well}.npz")["initial_cond"]
    if kind == "spread":
        return _spread(psi0, n)
    assert n == N, kind
    # "lower half": the water tables of members [0, 512) start within a cell of each other, those of members
    # [512, 1000) more than half a metre deeper
    # "one survivor": member 300 alone (a shard of its own in THREE) starts there
    off = np.random.default_rng(12).uniform(-2.0, 2.0, size=N)
    deep = np.arange(N) >= 512 if kind == "lower half" else np.arange(N) != 300
    off[deep] -= HALF_SHIFT_CM
    return psi0[None, :] + off[:, None]


HALF_SHIFT_CM = 60.0


def _handle(lo, hi, shard=None, sigma=None, noise="philox", initial="spread", n=N, well=WELL):
    """Members [lo, hi) of the ensemble of ``n``; ``shard`` = (bounds, index, exchange) or None: no hc_set_filter_shard."""
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(well)
    st = EnsembleStepper(cols, forcing, hi - lo)
    st.set_state(_initial(initial, n, well)[lo:hi])
    if noise == "philox":
        st.set_noise_philox(SEED, lo)
    else:
        st.set_noise_host(np.random.default_rng(SEED).standard_normal((n, cols.dim_d))[lo:hi])
    st.set_filter(STRIDE, 2.0 * cols.dz if sigma is None else sigma, FSEED)
    if shard is not None:
        st.set_filter_shard(*shard)
    return st


def _step(st, lo, hi, rows, noise, n_all=N):
    """rows [1, rows] in two calls (a call's refresh vectors, host noise: the handle's members of the ensemble's
    ``n_all``)"""
    for r0, n in ((1, rows // 2), (1 + rows // 2, rows - rows // 2)):
        kw = {}
        if noise == "numpy":
            fresh = np.random.default_rng(1000 + r0).standard_normal((st.n_refresh(r0, n), n_all, st.D))
            kw["fresh_noise"] = np.ascontiguousarray(fresh[:, lo:hi])
        st.step_rows(r0, n, **kw)


def _results(st, noise):
    return dict(psi=st.get_state(), base=st.filter_base() if noise == "philox" else st.get_noise_base(),
                table=st.filter_table(), weights=st.filter_weights(), draw=st.filter_draw(), anc=st.filter_ancestors(),
                moments=np.asarray(st.moments()))


_WHOLE = {}


def _whole(sigma=None, noise="philox", initial="spread", rows=ROWS):
    """the one handle that holds all N members: computed once per setting, shared and left unchanged"""
    key = (sigma, noise, initial, rows)
    if key not in _WHOLE:
        st = _handle(0, N, None, sigma, noise, initial)
        try:
            _step(st, 0, N, rows, noise)
            _WHOLE[key] = _results(st, noise)
        finally:
            st.close()
    return _WHOLE[key]


def _run_together(bounds, sigma=None, noise="philox", initial="spread", rows=ROWS, exchange_of=None, well=WELL):
    """One handle per block of ``bounds`` stepping the rows at once: (every handle's results in block order, the card,
    the handles' failures)."""
    S = len(bounds) - 1
    card = CardExchange(S)
    make = exchange_of or CardExchange.of
    handles = [_handle(bounds[k], bounds[k + 1], (bounds, k, make(card, k)), sigma, noise, initial, bounds[-1], well)
               for k in range(S)]
    failures = [None] * S

    def work(k):
        try:
            _step(handles[k], bounds[k], bounds[k + 1], rows, noise, bounds[-1])
        except BaseException as e:  # noqa: BLE001
            failures[k] = e
            card.barrier.abort()                                    # the others must not wait for this one
    try:
        threads = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(S)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=600)
        assert not any(t.is_alive() for t in threads), "a handle's step did not return"
        got = [_results(st, noise) if failures[k] is None else None for k, st in enumerate(handles)]
        return got, card, failures
    finally:
        for st in handles:
            st.close()


def _assert_like_one(got, ref, bounds, what):
    for key in ("psi", "base", "anc"):
        assert _bits(np.concatenate([g[key] for g in got]), ref[key]), (what, bounds, key)
    assert _bits(sum(g["moments"] for g in got), ref["moments"]), (what, bounds)
    for g in got:                                                   # identical on every handle, and the one handle's
        for key in ("table", "weights", "draw"):
            assert _bits(g[key], ref[key]), (what, bounds, key)


# ---- 1. bit equality --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", [TWO, THREE], ids=["two", "three"])
def test_two_and_three_handles_resample_like_one(bounds):
    ref = _whole()
    assert ref["table"][0, 1, 0] == N and ref["table"][0, 2, 0] == N           # both rows were assimilated
    assert not np.array_equal(ref["anc"], np.arange(N))                        # ... and resampling chose
    got, card, failures = _run_together(bounds)
    assert failures == [None] * (len(bounds) - 1), failures
    assert card.gathers == [2] * card.n and card.routes == [2] * card.n        # once per assimilation on every handle
    assert any(sum(words) for k in range(card.n) for words in card.sent[k])    # columns did change hands
    _assert_like_one(got, ref, bounds, "spread")


# ---- 2. everything routed, nothing routed -----------------------------------------------------------------------------
def test_a_handle_whose_members_all_die_takes_every_column_from_the_other():
    _, cols, _ = digest(WELL)
    kw = dict(sigma=0.5 * cols.dz, initial="lower half", rows=STRIDE)
    ref = _whole(**kw)
    assert ref["table"][0, 1, 0] == N
    assert ref["anc"].max() < 512 and ref["anc"][512:].min() >= 0               # the case is what it says
    got, card, failures = _run_together(TWO, **kw)
    assert failures == [None, None], failures
    distinct = np.unique(ref["anc"][512:]).size
    assert card.sent[0] == [[0, distinct * 2 * cols.dim_d]] and card.sent[1] == [[0, 0]]
    _assert_like_one(got, ref, TWO, "lower half")


def test_one_survivor_in_a_shard_of_its_own_fills_every_slot():
    _, cols, _ = digest(WELL)
    kw = dict(sigma=0.5 * cols.dz, initial="one survivor", rows=STRIDE)
    ref = _whole(**kw)
    assert ref["table"][0, 1, 0] == N and ref["table"][0, 1, 3] == 1
    assert np.array_equal(ref["anc"], np.full(N, 300))                          # the case is what it says
    got, card, failures = _run_together(THREE, **kw)
    assert failures == [None] * 3, failures
    one = 2 * cols.dim_d                                                        # the same column, once to either side
    assert card.sent == [[[0, 0, 0]], [[one, 0, one]], [[0, 0, 0]]]
    _assert_like_one(got, ref, THREE, "one survivor")


def test_equal_weights_route_nothing():
    ref = _whole(sigma=1e30)
    assert np.array_equal(ref["anc"], np.arange(N)) and ref["table"][0, 2, 0] == N
    got, card, failures = _run_together(THREE, sigma=1e30)
    assert failures == [None] * 3, failures
    assert card.gathers == [2] * 3 and card.routes == [2] * 3                  # both callbacks are still called
    assert all(words == [0, 0, 0] for k in range(3) for words in card.sent[k])
    _assert_like_one(got, ref, THREE, "flat")


# ---- 3. host noise ----------------------------------------------------------------------------------------------------
def test_host_noise_carries_the_base_vectors_along():
    ref = _whole(noise="numpy")
    assert ref["table"][0, 2, 0] == N and not np.array_equal(ref["anc"], np.arange(N))
    got, card, failures = _run_together(THREE, noise="numpy")
    assert failures == [None] * 3, failures
    _assert_like_one(got, ref, THREE, "host noise")


# ---- 4. identity ------------------------------------------------------------------------------------------------------
def test_a_handle_that_holds_every_member_is_the_unsharded_run():
    ref = _whole()
    st = _handle(0, N, ([0, N], 0, None))
    try:
        assert st.get_filter_shard() == (1, 0, N)
        _step(st, 0, N, ROWS, "philox")
        got = _results(st, "philox")
    finally:
        st.close()
    for key in ref:
        assert _bits(got[key], ref[key]), key


# ---- 5. refusals ------------------------------------------------------------------------------------------------------
def test_refusals():
    from hydromodel_amd import _lib as L
    from hydromodel_amd.stepper import EnsembleStepper
    _, cols, forcing = digest(WELL)
    gather, route = L.EXCHANGE_FN(lambda *a: 0), L.ROUTE_FN(lambda *a: 0)
    buf = torch.zeros(1 << 20, dtype=torch.float64, device="cuda")

    def call(st, bounds, index, n_words=None, ptr="buf", g=gather, r=route):
        b = np.asarray(bounds, dtype=np.int64)
        words = buf.numel() if n_words is None else n_words
        return st.lib.hc_set_filter_shard(st.h, b.size - 1, L.lptr(b), index, buf.data_ptr() if ptr == "buf" else None,
                                          words, g, r, None)

    def refused(st, bounds, index, match, **kw):
        assert call(st, bounds, index, **kw) == -1 and match in st.lib.hc_last_error().decode(), st.lib.hc_last_error()
        assert st.get_filter_shard() == (0, 0, 0)                       # HC_ERR_ARG, a message, and sharding off

    st = EnsembleStepper(cols, forcing, 300)
    try:
        st.set_state(golden(f"g1_tables_{WELL}.npz")["initial_cond"])
        st.set_noise_philox(SEED, 100)
        refused(st, [0, 100, 400], 1, "particle filter is off")
        st.set_filter(STRIDE, 5.0, 1)
        refused(st, [1, 100, 400], 1, "start at 0")
        refused(st, [0, 100, 100, 400], 1, "strictly increasing")
        refused(st, [0, 400, 100], 0, "strictly increasing")
        refused(st, [0, 100, 400], 2, "outside [0, 2)")
        refused(st, [0, 100, 400], -1, "outside [0, 2)")
        refused(st, [0, 100, 401], 1, "holds 300 members")
        refused(st, [0, 100, 400, 1 << 31], 1, "2^31 - 1")
        refused(st, [0, 300, 400], 0, "hc_set_noise_philox")            # the members are keyed from 100
        refused(st, [0, 100, 400], 1, "NULL buffer or callback", ptr=None)
        refused(st, [0, 100, 400], 1, "NULL buffer or callback", g=L.EXCHANGE_FN())
        refused(st, [0, 100, 400], 1, "NULL buffer or callback", r=L.ROUTE_FN())
        need = st.filter_shard_words([0, 100, 400], 1)
        assert need == 400 + (300 + 2 - 1) * 2 * cols.dim_d + 300 * 2 * cols.dim_d
        refused(st, [0, 100, 400], 1, "needed", n_words=need - 1)
        for off in (lambda: st.set_filter(0), lambda: L.check(st.lib.hc_set_members(st.h, 300)),
                    lambda: st.set_noise_philox(SEED, 100), lambda: st.set_filter_shard(None)):
            L.check(st.lib.hc_set_members(st.h, 300))                  # from the start: members, state, noise, filter
            st.set_state(golden(f"g1_tables_{WELL}.npz")["initial_cond"])
            st.set_noise_philox(SEED, 100)
            st.set_filter(STRIDE, 5.0, 1)
            assert call(st, [0, 100, 400], 1, n_words=need) == 0 and st.get_filter_shard() == (2, 1, 400)
            off()
            assert st.get_filter_shard() == (0, 0, 0)
    finally:
        st.close()
    two = EnsembleStepper([cols, cols], forcing, 512)
    try:
        two.set_state(golden(f"g1_tables_{WELL}.npz")["initial_cond"])
        two.set_noise_philox(SEED, 0)
        two.set_filter(STRIDE, 5.0, 1)
        refused(two, [0, 512], 0, "2 points")
    finally:
        two.close()


# ---- 6. a failing callback --------------------------------------------------------------------------------------------
def test_a_failing_callback_fails_the_step_cleanly():
    from hydromodel_amd import _lib as L

    class Broken:
        def __call__(self, block, first, count):
            pass

        def route(self, send, send_words, recv, recv_words):
            raise RuntimeError("the peer is gone")

    st = _handle(0, N, ([0, N], 0, Broken()))
    try:
        a = L.StepArgs()
        a.row_begin, a.n_rows, a.accumulate_moments = 1, ROWS, 1
        rc = st.lib.hc_step_rows(st.h, C.byref(a))
        assert rc == -2 and "routing callback returned 1" in st.lib.hc_last_error().decode()       # HC_ERR_DEVICE
        st._shard_error = None
    finally:
        st.close()
    assert st.h is None                                              # ... and the handle could be destroyed


def test_a_raising_callback_releases_the_other_handle():
    from hydromodel_amd import _lib as L

    class Raises:
        def __call__(self, block, first, count):
            raise RuntimeError("the peer is gone")

        def route(self, send, send_words, recv, recv_words):
            raise AssertionError("never reached")

    t0 = time.monotonic()
    got, card, failures = _run_together(TWO, exchange_of=lambda card, k: card.of(0) if k == 0 else Raises())
    assert time.monotonic() - t0 < 60.0                              # released by the abort, not by the barrier's timeout
    assert got == [None, None]
    assert all(isinstance(f, L.HcError) and "gather callback returned 1" in str(f) for f in failures), failures
    assert isinstance(failures[1].__cause__, RuntimeError) and "the peer is gone" in str(failures[1].__cause__)
    assert isinstance(failures[0].__cause__, threading.BrokenBarrierError)


# ---- 7. the CLI -------------------------------------------------------------------------------------------------------
def test_cli_sharded_on_two_ranks_writes_the_one_rank_file(tmp_path):
    params = _cli_params(tmp_path)
    params["Ensemble"] = {"Members": 1001, "Seed": 5, "Days": 3, "Distribution": {"Stride": 48},
                          "Filter": {"Stride": 48, "Sigma_cm": 8.0, "Sharded": True}}
    one, log1 = _run_cli(tmp_path, "run", params, 1)
    (tmp_path / "run").rename(tmp_path / "run_one")
    two, log2 = _run_cli(tmp_path, "run", params, 2)
    assert set(one) == set(two) and "filter_sharded" in one and "filter_loglik" in one
    assert int(one["gpus"]) == 1 and int(two["gpus"]) == 2
    for k in sorted(set(one) - {"gpus"}):
        a, b = np.asarray(one[k]), np.asarray(two[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert one["filter_sharded"].dtype == np.int8 and int(one["filter_sharded"]) == 1
    assert one["filter_count"].tolist() == [1001] * one["filter_rows"].size and one["filter_rows"].size == 3
    closing = [[s for s in log.splitlines() if "filter log-likelihood" in s or "CRPS" in s] for log in (log1, log2)]
    assert closing[0] == closing[1] and len(closing[0]) == 2
