"""The sharded EnKF without a GPU: the dealing of tiles to ranks, the ``"Sharded"`` key of the EnKF block, the gather of
unequal blocks over gloo, and the three entry points of include/hydrocol.h."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from hydromodel_amd import multigpu
from hydromodel_amd.cli import ENKF_KEYS, enkf_settings, enkf_sharded

TILE = 256


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("n", [1000, 4099, 262144])
@pytest.mark.parametrize("world", [1, 2, 3, 5, 8])
def test_shard_tiles_deals_whole_tiles(n, world):
    n_tiles = -(-n // TILE)
    if n_tiles < world:
        # `world` non-empty blocks that each start on a multiple of 256 below n need `world` such multiples: there are
        # only n_tiles of them (1000 members are 4 tiles: 5 or 8 ranks cannot all own one)
        with pytest.raises(ValueError, match="a rank would be empty"):
            [multigpu.shard_tiles(n, r, world) for r in range(world)]
        return
    parts = [multigpu.shard_tiles(n, r, world) for r in range(world)]
    assert parts[0][0] == 0 and parts[-1][1] == n                                   # they cover [0, n) ...
    assert all(parts[r][1] == parts[r + 1][0] for r in range(world - 1))            # ... contiguously
    assert all(lo % TILE == 0 and hi > lo for lo, hi in parts)
    assert all((hi - lo) % TILE == 0 for lo, hi in parts[:-1])                      # only the last block ends inside a tile
    tiles = [-(-(hi - lo) // TILE) for lo, hi in parts]
    assert sum(tiles) == n_tiles and max(tiles) - min(tiles) <= 1
    sizes = [hi - lo for lo, hi in parts]
    assert max(sizes) - min(sizes) <= TILE


def test_shard_tiles_refuses_an_empty_rank():
    with pytest.raises(ValueError, match="a rank would be empty"):
        [multigpu.shard_tiles(300, r, 3) for r in range(3)]
    assert [multigpu.shard_tiles(300, r, 2) for r in range(2)] == [(0, 256), (256, 300)]
    assert multigpu.shard_tiles(262144, 1, 2) == (131072, 262144)
    assert multigpu.shard_tiles(10, 0, 1, tile=4) == (0, 10)


def test_the_sharded_key_opts_a_single_point_enkf_into_several_gpus():
    assert "Sharded" in ENKF_KEYS
    block = {"Stride": 24, "Sigma_cm": 8.0, "Localisation_cm": 40, "Seed": 9}
    plain = enkf_settings({"EnKF": dict(block)}, 1)
    assert enkf_settings({"EnKF": dict(block, Sharded=True)}, 2) == plain == (24, 8.0, 40.0, 9)
    assert enkf_settings({"EnKF": dict(block, Sharded=True)}, 1) == plain
    for ens in ({"EnKF": dict(block)}, {"EnKF": dict(block, Sharded=False)}):       # without it the refusal stands
        with pytest.raises(ValueError, match="covariances would need a sum over the ranks"):
            enkf_settings(ens, 2)
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="EnKF.Sharded"):
            enkf_settings({"EnKF": dict(block, Sharded=bad)}, 2)
    pts = [{"Soil_Properties": {"n": 1.6}}, {"Soil_Properties": {"n": 2.4}}]
    assert enkf_settings({"Points": pts, "EnKF": dict(block, Sharded=True)}, 2) == plain     # a sweep: accepted, ignored
    with pytest.raises(ValueError, match="exclude each other"):                     # "Filter" stays refused
        enkf_settings({"Filter": {"Sigma_cm": 5.0}, "EnKF": dict(block, Sharded=True)}, 2)
    assert enkf_sharded({"EnKF": dict(block)}) is None
    assert enkf_sharded({"EnKF": dict(block, Sharded=True)}) is True
    assert enkf_sharded({"EnKF": dict(block, Sharded=False)}) is False
    assert enkf_sharded({"EnKF": dict(block, Stride=0, Sharded=True)}) is None and enkf_sharded({}) is None


COLS, TILES = 7, (3, 1)


def _block_of(rank):
    """What rank `rank` writes into its tiles: values no other rank has, with a -0.0 and a NaN payload among them."""
    t0 = sum(TILES[:rank])
    v = np.random.default_rng(50 + rank).standard_normal(TILES[rank] * COLS)
    bits = v.view(np.int64)
    bits[0] = np.int64(-(2**63))
    bits[1] = np.int64(0x7FF8_0000_0BAD_0000 + rank)
    return t0 * COLS, v


def _exchange_worker(rank, world, port, out_dir):
    import torch
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), HYDROCOL_DIST_BACKEND="gloo")
    ranks = multigpu.Ranks(expect=world)
    exchange = multigpu.ShardExchange(ranks)
    first, mine = _block_of(rank)
    block = torch.full((sum(TILES) * COLS,), float(rank + 10), dtype=torch.float64)     # (stale words everywhere else)
    block[first:first + mine.size] = torch.from_numpy(mine)
    exchange(block, first, mine.size)
    # the first member's column: rank 0 alone contributes
    col = torch.full((5,), -1.0, dtype=torch.float64)
    if rank == 0:
        col[:] = torch.arange(5, dtype=torch.float64)
    exchange(col, 0, 5 if rank == 0 else 0)
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), block=block.numpy(), col=col.numpy(), calls=exchange.calls)
    ranks.close()


def test_the_exchange_gathers_unequal_blocks_over_gloo(tmp_path):
    world = 2
    mp.spawn(_exchange_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    want = np.concatenate([_block_of(r)[1] for r in range(world)])
    for r in range(world):
        got = np.load(tmp_path / f"r{r}.npz")
        assert np.array_equal(got["block"].view(np.int64), want.view(np.int64))         # to the bit, on both ranks
        assert got["col"].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and int(got["calls"]) == 2


def test_the_exchange_is_the_identity_with_one_rank():
    import torch
    exchange = multigpu.ShardExchange(multigpu.Ranks())
    block = torch.arange(12, dtype=torch.float64)
    exchange(block, 0, 12)
    assert block.tolist() == list(range(12)) and exchange.calls == 1


def test_the_shard_entry_points_are_exported_as_declared():
    import __graft_entry__ as ge
    ge.build()
    from hydromodel_amd import _lib
    lib = _lib.load()
    header = (ge.REPO / "include" / "hydrocol.h").read_text()
    assert ("typedef int (*hc_enkf_exchange_fn)(void *ctx, void *device_buf, int64_t n_words, int64_t first_word, "
            "int64_t count_words);") in header
    for decl in ("int hc_get_enkf_shard_words(hc_handle *h, int64_t n_global, int64_t *n_words);",
                 "int hc_set_enkf_shard(hc_handle *h, int64_t n_global, int64_t first_global, void *device_buf, int64_t n_words,",
                 "int hc_get_enkf_shard(hc_handle *h, int64_t *n_global, int64_t *first_global);"):
        assert decl in header, decl
    lp = C.POINTER(C.c_int64)
    want = {"hc_get_enkf_shard_words": [C.c_void_p, C.c_int64, lp],
            "hc_set_enkf_shard": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, _lib.EXCHANGE_FN, C.c_void_p],
            "hc_get_enkf_shard": [C.c_void_p, lp, lp]}
    for name, argtypes in want.items():
        fn = getattr(lib, name)
        assert _lib.EXPORTS[name] == (argtypes, C.c_int) and fn.argtypes == argtypes and fn.restype is C.c_int
    proto = _lib.EXCHANGE_FN
    assert proto._restype_ is C.c_int and proto._argtypes_ == (C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64)
    # NULL handles are refused with a message, never dereferenced
    n = C.c_int64(0)
    assert lib.hc_get_enkf_shard_words(None, 1000, C.byref(n)) == -1
    assert lib.hc_set_enkf_shard(None, 1000, 0, None, 0, proto(), None) == -1 and b"hc_set_enkf_shard" in lib.hc_last_error()
    assert lib.hc_get_enkf_shard(None, C.byref(n), C.byref(n)) == -1


_ORDER = """
import sys
sys.path.insert(0, {repo!r})
from hydromodel_amd import _lib
first = sys.argv[1]
if first == "library":
    _lib.load()
    try:
        _lib.load(with_torch=True)
    except _lib.HcError as e:
        print("refused:", e)
else:
    _lib.load(with_torch=True)
    _lib.load(with_torch=True)
runtimes = sorted({{line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}})
print("torch" in sys.modules, len(runtimes))
"""


@pytest.mark.parametrize("first", ["torch", "library"])
def test_the_library_and_torch_share_one_hip_runtime(first):
    """The shard's buffer is a torch tensor the library's kernels write: `load(with_torch=True)` brings torch in before
    the library (one HIP runtime in the process, torch's), and refuses when the library was there first."""
    import subprocess
    import sys
    import __graft_entry__ as ge
    ge.build()
    r = subprocess.run([sys.executable, "-c", _ORDER.format(repo=str(ge.REPO)), first], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    if first == "torch":
        assert lines == ["True 1"], r.stdout
    else:
        assert lines[0].startswith("refused:") and "before torch" in lines[0]
        assert lines[-1] == "False 1", r.stdout                      # ... and torch was not imported after it
