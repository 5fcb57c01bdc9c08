"""The particle filter over several handles, the parts that need no GPU: the NumPy restatement of the routing
(``stepper.filter_routes``) against a per-slot lookup, the CLI's ``"Filter": {"Sharded": true}``, and the column exchange
(``multigpu.ShardExchange.route``) over gloo on CPU tensors in a world of 3."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from hydromodel_amd import multigpu
from hydromodel_amd.cli import FILTER_KEYS, filter_settings, filter_sharded
from hydromodel_amd.stepper import FILTER_Q_ONE, filter_ancestors_of, filter_routes


# ---- 1. the routing ---------------------------------------------------------------------------------------------------
N = 97
BOUNDS = ([0, 40, 41, 97], [0, 1, 2, 97], [0, 50, 97], [0, 97], [0, 30, 60, 61, 97])


def _ancestries():
    rng = np.random.default_rng(11)
    out = {}
    q = rng.integers(0, FILTER_Q_ONE + 1, size=N)
    out["random"] = filter_ancestors_of(q, int(rng.integers(0, int(q.sum()))))
    q = np.where(rng.random(N) < 0.8, 0, rng.integers(1, FILTER_Q_ONE + 1, size=N))       # most members leave no offspring
    out["sparse"] = filter_ancestors_of(q, int(rng.integers(0, int(q.sum()))))
    for m in (0, 40, 96):                                                                 # one survivor, in each shard
        q = np.zeros(N, dtype=np.int64)
        q[m] = 5
        out[f"collapsed-{m}"] = filter_ancestors_of(q, 3)
    out["flat"] = filter_ancestors_of(np.full(N, FILTER_Q_ONE), 12345)
    out["Q=0"] = np.arange(N, dtype=np.int64)              # no member counted: the library keeps the identity
    return out


ANCESTRIES = _ancestries()


def test_the_cases_are_what_they_say():
    assert np.array_equal(ANCESTRIES["flat"], np.arange(N))
    assert all(np.unique(ANCESTRIES[f"collapsed-{m}"]).tolist() == [m] for m in (0, 40, 96))
    assert all((np.diff(a) >= 0).all() and a.min() >= 0 and a.max() < N for a in ANCESTRIES.values())
    assert 1 < np.unique(ANCESTRIES["sparse"]).size < N // 2


@pytest.mark.parametrize("bounds", BOUNDS, ids=str)
@pytest.mark.parametrize("case", list(ANCESTRIES))
def test_routes_against_a_per_slot_lookup(case, bounds):
    anc = ANCESTRIES[case]
    S = len(bounds) - 1
    send, recv = filter_routes(anc, bounds)
    owner = np.searchsorted(bounds, np.arange(N), side="right") - 1
    for d in range(S):
        for s in range(S):
            lst = np.asarray(recv[d][s])
            assert np.array_equal(lst, send[s][d])                        # both ends hold the same list
            assert (np.diff(lst) > 0).all()                               # ascending and distinct
            assert ((lst >= bounds[s]) & (lst < bounds[s + 1])).all()
            assert s != d or lst.size == 0
        # every slot finds its ancestor: on its own shard, or in the list of the shard that owns it
        want = {(int(owner[a]), int(a)) for a in anc[bounds[d]:bounds[d + 1]] if owner[a] != d}
        assert want == {(s, int(a)) for s in range(S) for a in recv[d][s]}
        assert sum(len(recv[d][s]) for s in range(S)) <= bounds[d + 1] - bounds[d]
    for s in range(S):
        assert sum(len(send[s][d]) for d in range(S)) <= bounds[s + 1] - bounds[s] + S - 1
        for d in range(S):
            for e in range(d + 1, S):                                     # two destinations share at most one member
                assert np.intersect1d(send[s][d], send[s][e]).size <= 1
    if case in ("flat", "Q=0"):
        assert all(len(send[s][d]) == 0 for s in range(S) for d in range(S))


def test_a_collapsed_ensemble_sends_one_column_to_everyone():
    send, _ = filter_routes(ANCESTRIES["collapsed-40"], [0, 40, 41, 97])
    assert [a.tolist() for a in send[1]] == [[40], [], [40]]
    assert all(a.size == 0 for s in (0, 2) for a in send[s])


# ---- 2. the CLI's key -------------------------------------------------------------------------------------------------
def test_sharded_is_a_filter_key():
    assert "Sharded" in FILTER_KEYS
    ens = {"Filter": {"Sigma_cm": 1.0, "Sharded": True}}
    assert filter_settings(ens, 2) == (48, 1.0, None) and filter_settings(ens, 1) == (48, 1.0, None)
    assert filter_settings(ens, 8) == (48, 1.0, None)
    assert filter_sharded(ens) is True


def test_false_or_no_key_keeps_the_refusal():
    for block in ({"Sigma_cm": 1.0, "Sharded": False}, {"Sigma_cm": 1.0}):
        with pytest.raises(ValueError, match="resampling would move members between ranks"):
            filter_settings({"Filter": block}, 2)
        assert filter_settings({"Filter": block}, 1) == (48, 1.0, None)
    assert filter_sharded({"Filter": {"Sigma_cm": 1.0, "Sharded": False}}) is False
    assert filter_sharded({"Filter": {"Sigma_cm": 1.0}}) is None
    assert filter_sharded({}) is None
    assert filter_sharded({"Filter": {"Stride": 0, "Sigma_cm": 1.0, "Sharded": True}}) is None       # the filter is off


@pytest.mark.parametrize("value", [1, 0, "true", None, [True]])
def test_a_non_boolean_is_rejected(value):
    with pytest.raises(ValueError, match="Filter.Sharded"):
        filter_settings({"Filter": {"Sigma_cm": 1.0, "Sharded": value}}, 2)


def test_a_sweep_accepts_and_ignores_the_key():
    ens = {"Points": [{"a": 1}], "Filter": {"Sigma_cm": 2.0, "Sharded": True}}
    assert filter_settings(ens, 4) == (48, 2.0, None)
    assert filter_settings(dict(ens, Filter={"Sigma_cm": 2.0}), 4) == (48, 2.0, None)


# ---- 3. the column exchange over gloo ---------------------------------------------------------------------------------
WORLD = 3
COUNTS = [[0, 4, 0], [6, 0, 2], [0, 0, 0]]           # COUNTS[s][d] words from rank s to rank d: unequal, with zeros


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _words(s, d):
    """what rank s sends rank d: random bits with -0.0 and a NaN payload planted"""
    v = np.random.default_rng(100 * s + d).standard_normal(COUNTS[s][d])
    bits = v.view(np.int64)
    if bits.size > 1:
        bits[0] = np.int64(-(2**63))
        bits[1] = np.int64(0x7FF8_0000_0BAD_0000 + 16 * s + d)
    return v


def _route_worker(rank, world, port, out_dir):
    import torch
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), HYDROCOL_DIST_BACKEND="gloo")
    ranks = multigpu.Ranks(expect=world)
    out, back = COUNTS[rank], [COUNTS[s][rank] for s in range(world)]
    send = torch.from_numpy(np.concatenate([_words(rank, d) for d in range(world)]))
    got = {}
    for tag, exchange in (("alltoall", multigpu.ShardExchange(ranks)), ("padded", multigpu.ShardExchange(ranks, padded=True))):
        recv = torch.full((sum(back),), float(rank + 10), dtype=torch.float64)           # stale words
        exchange.route(send, out, recv, back)
        exchange.route(send[:0], [0] * world, recv[:0], [0] * world)                     # nothing routed: still a call
        got[tag] = recv.numpy()
        assert exchange.routes == 2 and exchange.routed_words == sum(out)
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), **got)
    ranks.close()


def test_the_route_moves_every_bit_over_gloo(tmp_path):
    mp.spawn(_route_worker, args=(WORLD, _free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    for r in range(WORLD):
        want = np.concatenate([_words(s, r) for s in range(WORLD)])
        got = np.load(tmp_path / f"r{r}.npz")
        for tag in ("alltoall", "padded"):
            assert np.array_equal(got[tag].view(np.int64), want.view(np.int64)), (r, tag)
    assert np.isnan(_words(1, 0)[1]) and np.signbit(_words(1, 0)[0]) and _words(1, 0)[0] == 0.0


def test_the_route_is_the_identity_with_one_rank_and_checks_its_counts():
    import torch
    exchange = multigpu.ShardExchange(multigpu.Ranks())
    none = torch.zeros(0, dtype=torch.float64)
    exchange.route(none, [0], none, [0])
    assert exchange.routes == 1 and exchange.routed_words == 0
    with pytest.raises(RuntimeError, match="counts"):
        exchange.route(torch.zeros(2, dtype=torch.float64), [2], none, [0])              # words for itself


# ---- 4. the entry points ----------------------------------------------------------------------------------------------
def test_the_shard_entry_points_are_exported_as_declared():
    import __graft_entry__ as ge
    ge.build()
    from hydromodel_amd import _lib
    lib = _lib.load()
    header = (ge.REPO / "include" / "hydrocol.h").read_text()
    assert ("typedef int (*hc_filter_route_fn)(void *ctx, void *send, const int64_t *send_words, void *recv, "
            "const int64_t *recv_words);") in header
    for name in ("hc_get_filter_shard_words", "hc_set_filter_shard", "hc_get_filter_shard"):
        assert f"int {name}(hc_handle *h" in header and name in _lib.EXPORTS
        assert getattr(lib, name) is not None
