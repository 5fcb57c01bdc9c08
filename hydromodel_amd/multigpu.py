"""One process per GPU for the two workloads that shard: ensemble members and whole parameter points.

The reference runs ONE column in ONE process (``/root/reference/code/berkeley_hydro_main.py:128-137``: ``sim.run();
sim.saveResults()``).  Here ``berkeley_hydro_main.py --gpus N`` (or ``"Ensemble": {"GPUs": N}``) starts N ranks of the
same command line -- child processes of ``torch.distributed.run`` on 127.0.0.1, started BEFORE this process has touched
a GPU, never a re-exec -- and every rank runs its share with no communication while stepping:

* ensemble: rank r owns the contiguous member block ``shard(N, r, world)``; the Philox stream is keyed by the GLOBAL
  member id, the shared initial condition is global member 0's spin-up on every rank, and ONE int64 all-reduce of the
  per-row water-table moments ``[3][T]`` ends the run (RCCL over xGMI with the nccl backend); with a sharded EnKF
  (``"EnKF": {"Sharded": true}``) the members are dealt in whole tiles (:func:`shard_tiles`) and every analysis gathers
  the ranks' tile partials before each of its reductions (:class:`ShardExchange`), so the analyses are the one-rank run's;
  with a sharded particle filter (``"Filter": {"Sharded": true}``) the members are dealt by :func:`shard`, every
  assimilation gathers the members' water-table indices and then moves the columns whose ancestor lives on another rank
  (:meth:`ShardExchange.route`), so the resampled ensemble is the one-rank run's;
* sweep (BASELINE config 5): whole points are dealt round-robin (``ensemble.deal_points``); every rank places ITS points
  in zeroed ``[P][3][T]`` / ``[P][D]`` / ``[P]`` tables and one all-reduce each assembles them (:func:`place_points`: float64
  tables travel as their int64 bits, so the assembled file holds every point's bits exactly as the rank that ran it
  produced them).

Rank 0 owns the output file.  Integer moment sums are order-independent: the file is bit-identical at any rank count.
"""
import os
import subprocess
import sys

import numpy as np


def requested_gpus(cli_gpus, params):
    """--gpus wins over "Ensemble": {"GPUs": N}; 1 when neither is given."""
    if cli_gpus:
        return int(cli_gpus)
    ens = params.get("Ensemble") or {}
    return int(ens.get("GPUs", 1) or 1)


def in_rank():
    """True inside a rank started by a launcher (torch.distributed.run sets these)."""
    return "RANK" in os.environ and "WORLD_SIZE" in os.environ


def launch_ranks(n_ranks, script, argv):
    """Start ``n_ranks`` ranks of ``python script argv...`` as children of torch.distributed.run and return the launcher's
    exit code.  Must run before anything in this process has initialised a GPU."""
    # --standalone: the launcher's own c10d store picks a free port on 127.0.0.1 and hands it to the ranks (no
    # bind-close-reuse of a port another process can take in between)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"),
               HYDROCOL_EXPECT_WORLD=str(n_ranks))
    for k in ("MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
           "--nproc-per-node", str(n_ranks), str(script)] + list(argv)
    return subprocess.run(cmd, env=env).returncode


class Ranks:
    """The process group of a multi-GPU run (or a stand-in with one rank when there is none)."""

    def __init__(self, expect=None):
        self.rank, self.world, self.local_rank = 0, 1, 0
        self.dist = None
        self.backend = None
        if not in_rank():
            if expect and int(expect) > 1:
                raise RuntimeError(f" {expect} GPUs requested but this process is not a rank of a launcher.")
            return
        import torch.distributed as dist
        self.rank, self.world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
        self.local_rank = int(os.environ.get("LOCAL_RANK", self.rank))
        want = expect or os.environ.get("HYDROCOL_EXPECT_WORLD")
        if want and int(want) != self.world:
            raise RuntimeError(f" {want} GPUs requested but the launcher started WORLD_SIZE={self.world} ranks.")
        # nccl (= RCCL) unless a rehearsal asks for gloo (CPU tensors; e.g. several ranks sharing one card in a test)
        self.backend = os.environ.get("HYDROCOL_DIST_BACKEND", "nccl")
        if self.world > 1 or os.environ.get("HYDROCOL_DIST_FORCE"):
            if self.backend == "nccl":
                import torch
                torch.cuda.set_device(self.device_index())
            dist.init_process_group(self.backend, rank=self.rank, world_size=self.world)
            self.dist = dist

    def device_index(self):
        """GPU ordinal of this rank: its local rank, or 0 for every rank when a rehearsal shares one card."""
        return 0 if os.environ.get("HYDROCOL_SHARE_DEVICE") else self.local_rank

    def allreduce_sum(self, array):
        """Element-wise sum over the ranks (int64 or float64 NumPy array); identity with one rank."""
        a = np.ascontiguousarray(array)
        if self.dist is None:
            return a
        import torch
        t = torch.from_numpy(a.copy())
        if self.backend == "nccl":
            t = t.to(torch.device("cuda", self.device_index()))
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return t.cpu().numpy()

    def barrier(self):
        if self.dist is not None:
            self.dist.barrier()

    def close(self):
        if self.dist is not None:
            self.dist.destroy_process_group()
            self.dist = None


def shard(n_members, rank, world):
    """[lo, hi): the contiguous block of global member ids rank `rank` owns (sizes differ by at most one)."""
    n, r, w = int(n_members), int(rank), int(world)
    base, extra = divmod(n, w)
    lo = r * base + min(r, extra)
    return lo, lo + base + (1 if r < extra else 0)


def shard_tiles(n_members, rank, world, tile=256):
    """[lo, hi): the contiguous member block of rank `rank` when whole tiles of `tile` members are dealt (the EnKF's sums
    are formed tile by tile: a sharded analysis needs every block to start on a tile boundary, include/hydrocol.h
    hc_set_enkf_shard).  The tiles are dealt as evenly as :func:`shard` deals members, the ranks that get one more being
    the last ones -- the last tile may be partial, so the blocks differ by at most one tile of members.  A rank left
    without a member is a ValueError."""
    n, r, w, t = int(n_members), int(rank), int(world), int(tile)
    n_tiles = -(-n // t)
    base, extra = divmod(n_tiles, w)
    lo = r * base + max(0, r - (w - extra))
    hi = lo + base + (1 if r >= w - extra else 0)
    lo, hi = lo * t, min(hi * t, n)
    if hi <= lo:
        raise ValueError(f" Ensemble: {n} members are {n_tiles} tiles of {t}: they do not shard over {w} GPUs "
                         f"(a rank would be empty).")
    return lo, hi


class ShardExchange:
    """The gather of a sharded EnKF analysis over the ranks (``EnsembleStepper.set_enkf_shard``'s ``exchange``; also the
    index gather of a sharded particle filter, ``set_filter_shard``, whose column exchange is :meth:`route`): called
    with ``block``, a float64 tensor whose words [first, first + count) are this rank's, it returns with every other
    rank's words in place.  The ranks' blocks differ in size (and one rank alone contributes the point's first member),
    so each call first gathers the (first, count) pairs and pads the blocks to the largest: one regular all-gather.  Copies
    only: every bit arrives as it was written.  nccl gathers on the device tensor; gloo (ranks sharing a card in a
    rehearsal, CPU tensors in a test) stages through the host.  One rank: the identity."""

    def __init__(self, ranks, padded=False):
        self.ranks = ranks
        self.calls = 0
        self.routes, self.routed_words = 0, 0          # route() calls, and the words this rank sent in them
        self.padded = padded

    def __call__(self, block, first, count):
        import torch
        self.calls += 1
        dist, world = self.ranks.dist, self.ranks.world
        if dist is None or world == 1:
            return
        on_device = self.ranks.backend == "nccl"
        where = block.device if on_device else torch.device("cpu")
        meta = torch.tensor([int(first), int(count)], dtype=torch.int64, device=where)
        metas = [torch.zeros_like(meta) for _ in range(world)]
        dist.all_gather(metas, meta)
        spans = [tuple(int(v) for v in m.tolist()) for m in metas]
        if any(f < 0 or c < 0 or f + c > block.numel() for f, c in spans):
            raise RuntimeError(f" EnKF shard exchange: the ranks' word ranges {spans} do not fit {block.numel()} words.")
        widest = max(c for _, c in spans)
        if widest == 0:
            return
        mine = torch.zeros(widest, dtype=torch.float64, device=where)
        mine[:count] = block[first:first + count].to(where)
        parts = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(parts, mine)
        for r, (f, c) in enumerate(spans):
            if r != self.ranks.rank and c:
                block[f:f + c] = parts[r][:c].to(block.device)
        if block.is_cuda:
            torch.cuda.synchronize(block.device)          # in place before the library's stream reads it

    def route(self, send, send_words, recv, recv_words):
        """The column exchange of a sharded particle-filter assimilation (``EnsembleStepper.set_filter_shard``): a variable
        all-to-all of float64 words.  ``send`` holds this rank's blocks for the ranks one after the other,
        ``send_words[r]`` words for rank r; on return ``recv`` holds the blocks from them, ``recv_words[r]`` words from
        rank r.  Both ends derived the counts from the same ancestor table, so none travels.  nccl: on the device tensors;
        gloo: staged through the host.  ``padded``: the same exchange for a gloo without a variable all-to-all -- the
        counts gathered, then one all-gather of the send regions padded to the longest."""
        import torch
        self.routes += 1
        self.routed_words += int(sum(send_words))
        dist, world, me = self.ranks.dist, self.ranks.world, self.ranks.rank
        out, back = [int(v) for v in send_words], [int(v) for v in recv_words]
        if len(out) != world or len(back) != world or out[me] or back[me]:
            raise RuntimeError(f" Filter shard routing: counts {out} / {back} do not belong to rank {me} of {world}.")
        if send.numel() != sum(out) or recv.numel() != sum(back):
            raise RuntimeError(f" Filter shard routing: regions of {send.numel()} / {recv.numel()} words, counts {out} / {back}.")
        if dist is None or world == 1:
            return
        if self.ranks.backend == "nccl":
            dist.all_to_all_single(recv, send, back, out)
            torch.cuda.synchronize(recv.device)
            return
        host_in, host_out = send.cpu(), torch.empty(recv.numel(), dtype=torch.float64)
        if not self.padded:
            dist.all_to_all_single(host_out, host_in, back, out)
        else:
            counts = torch.tensor(out, dtype=torch.int64)
            table = [torch.zeros_like(counts) for _ in range(world)]
            dist.all_gather(table, counts)
            table = [[int(v) for v in t.tolist()] for t in table]
            if [table[r][me] for r in range(world)] != back:
                raise RuntimeError(f" Filter shard routing: rank {me} expects {back}, the ranks send {table}.")
            widest = max(sum(t) for t in table)
            if widest:
                mine = torch.zeros(widest, dtype=torch.float64)
                mine[:host_in.numel()] = host_in
                parts = [torch.empty_like(mine) for _ in range(world)]
                dist.all_gather(parts, mine)
                at = 0
                for r in range(world):
                    skip = sum(table[r][:me])
                    host_out[at:at + back[r]] = parts[r][skip:skip + back[r]]
                    at += back[r]
        recv.copy_(host_out)
        if recv.is_cuda:
            torch.cuda.synchronize(recv.device)


def place_points(local, point_ids, n_points, ranks=None):
    """A rank's ``[p][...]`` tables at rows ``point_ids`` of a zeroed ``[n_points][...]`` table, summed over ``ranks`` when
    given: every point has one owner, so the sum is the whole table with each point's entries as its rank made them.
    Integer tables come back as int64.  float64 tables are summed as their int64 bit patterns (``x + 0.0`` is not ``x`` for
    ``-0.0``, nor need a NaN's payload survive an add), so every bit of them survives."""
    local = np.asarray(local)
    bits = local.dtype == np.float64
    out = np.zeros((int(n_points),) + local.shape[1:], dtype=np.int64)
    if len(point_ids):
        out[np.asarray(point_ids, dtype=np.int64)] = local.view(np.int64) if bits else local
    if ranks is not None:
        out = ranks.allreduce_sum(out)
    return out.view(np.float64) if bits else out


def assemble_points(ranks, n_points, local, T, D):
    """Sweep result of ALL ranks from each rank's own points.

    ``local`` = {global point index: {"moments" int64 [3][T], "psi0" float64 [D], "spinup_iterations" int}} for the points
    this rank ran (possibly none).  Every rank's points are placed and summed over the ranks (:func:`place_points`), so
    every point's bits survive unchanged.  ``owners`` counts how many ranks delivered each point -- exactly one each, or
    the sweep was dealt wrongly."""
    P, ids = int(n_points), list(local)
    recs = [local[k] for k in ids]
    moments = place_points(np.array([r["moments"] for r in recs], dtype=np.int64).reshape(-1, 3, T), ids, P, ranks)
    psi0 = place_points(np.array([r["psi0"] for r in recs], dtype=np.float64).reshape(-1, D), ids, P, ranks)
    spin = np.array([0 if r.get("spinup_iterations") is None else int(r["spinup_iterations"]) for r in recs], dtype=np.int64)
    spin = place_points(spin, ids, P, ranks)
    owners = place_points(np.ones(len(ids), dtype=np.int64), ids, P, ranks)
    if not np.array_equal(owners, np.ones(P, dtype=np.int64)):
        bad = np.flatnonzero(owners != 1)
        raise RuntimeError(f" Sweep: points {bad[:8].tolist()} were delivered by {owners[bad[:8]].tolist()} ranks (expected one each).")
    return moments, psi0, spin
