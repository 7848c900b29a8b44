"""One process per GPU: torch.distributed plumbing (backend "nccl" is RCCL on ROCm; "gloo" for the CPU tests).

Reads shard across ranks with no data-path collective; the only exchange is the sum of the small per-name /
per-species int64 counters around the reassignment pass."""
import os

import numpy as np


def init_from_env(backend=None):
    """Initialise torch.distributed from RANK/WORLD_SIZE/MASTER_* if WORLD_SIZE > 1.  Returns (rank, world, local_rank)."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if world > 1:
        import torch.distributed as dist
        import torch
        if backend is None:
            backend = 'nccl' if torch.cuda.is_available() else 'gloo'
        if backend == 'nccl' and os.environ.get('MPN_SINGLE_DEVICE') != '1':
            torch.cuda.set_device(local)
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if not dist.is_initialized():
            dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, world, local


def make_allreduce(device=None):
    """-> callable(np.ndarray[int64]) summing in place over all ranks (identity when not distributed)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return None
    import torch

    def allreduce(arr):
        t = torch.from_numpy(arr)
        if device is not None:
            t = t.to(device)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        if device is not None:
            arr[:] = t.cpu().numpy()
    return allreduce


def shard_bounds(lengths, world):
    """Contiguous read ranges with balanced total bases (equal sum of bp, not equal count).
    -> list of (lo, hi) per rank."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n = len(lengths)
    if n == 0:
        return [(0, 0)] * world
    csum = np.cumsum(lengths)
    total = int(csum[-1])
    cuts = [0]
    for r in range(1, world):
        cuts.append(int(np.searchsorted(csum, total * r / world, side='left')) + 1 if total else 0)
    cuts.append(n)
    cuts = [min(max(c, 0), n) for c in cuts]
    for i in range(1, len(cuts)):
        cuts[i] = max(cuts[i], cuts[i - 1])
    return [(cuts[r], cuts[r + 1]) for r in range(world)]


def barrier():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        dist.barrier()


# ---- index parts sharded over ranks -----------------------------------------------------------------
# World W = R x S: rank r is shard s = r % S of read group g = r // S.  The S shards of a group hold contiguous blocks of the
# index parts; every rank of a group maps the group's whole batch against its own parts, and the hits of each owner sub-range
# go to the rank that owns it, which merges them (mpn_hits_export / mpn_hits_import).

def index_shard_layout(rank, world, n_shards):
    """-> (read group, index shard) of `rank`; n_shards must divide world."""
    if n_shards < 1 or world % n_shards:
        raise ValueError(f'{n_shards} index shards do not divide a world of {world} ranks')
    if not 0 <= rank < world:
        raise ValueError(f'rank {rank} outside a world of {world}')
    return rank // n_shards, rank % n_shards


def assign_parts(part_bases, n_shards):
    """Contiguous blocks of the index parts (in target order), one per shard, balanced by their bases: cut s sits at the part
    boundary nearest to s / n_shards of the total, and every block holds at least one part.  A pure function of its arguments,
    so that every rank derives the same assignment.  -> list of (first part, end part) per shard."""
    b = np.asarray(part_bases, dtype=np.int64)
    n = len(b)
    if n_shards < 1 or n < n_shards:
        raise ValueError(f'{n} index parts cannot be cut into {n_shards} non-empty shards')
    csum = np.concatenate([[0], np.cumsum(b)])
    total = int(csum[-1])
    cuts = [0]
    for s in range(1, n_shards):
        ideal = total * s / n_shards
        c = int(np.searchsorted(csum, ideal, side='left'))
        if c > 0 and (c > n or ideal - csum[c - 1] <= csum[c] - ideal):
            c -= 1
        cuts.append(min(max(c, cuts[-1] + 1), n - (n_shards - s)))
    cuts.append(n)
    return [(cuts[s], cuts[s + 1]) for s in range(n_shards)]


def owner_bounds(lengths, n_groups, n_shards):
    """Read ranges of a batch under the sharded layout: the batch is cut into n_groups base-balanced group ranges
    (shard_bounds), each group range into n_shards owner sub-ranges.  -> (group ranges, owned range per rank), all in batch
    indices; owned ranges are contiguous in rank order and may be empty."""
    lengths = np.asarray(lengths, dtype=np.int64)
    groups = shard_bounds(lengths, n_groups)
    owned = []
    for lo, hi in groups:
        owned += [(lo + a, lo + b) for a, b in shard_bounds(lengths[lo:hi], n_shards)]
    return groups, owned


def shard_groups(world, n_shards):
    """The process group of every read group's n_shards ranks (torch.distributed.new_group is collective: every rank creates
    every group, in the same order).  -> list of groups, index = read group; [None] * groups when not distributed or S == 1."""
    n_groups = world // n_shards
    import torch.distributed as dist
    if n_shards == 1 or not (dist.is_available() and dist.is_initialized()):
        return [None] * n_groups
    if n_groups == 1:
        return [dist.group.WORLD]
    return [dist.new_group(list(range(g * n_shards, (g + 1) * n_shards))) for g in range(n_groups)]


def exchange_bytes(blocks, group):
    """Variable-size all-to-all within `group`: blocks[j] (np.uint8) goes to the group's rank j.  -> the blocks received, index =
    sending rank in the group.  The sizes go first as int64 (all_to_all_single), then the payload with uneven splits; CPU tensors
    on gloo, device tensors on nccl (RCCL)."""
    import torch
    import torch.distributed as dist
    n = dist.get_world_size(group)
    if len(blocks) != n:
        raise ValueError(f'{len(blocks)} blocks for a group of {n} ranks')
    dev = torch.device('cpu')
    if dist.get_backend(group) == 'nccl':
        dev = torch.device('cuda', torch.cuda.current_device())
    blocks = [np.ascontiguousarray(b, dtype=np.uint8).reshape(-1) for b in blocks]
    send_n = torch.tensor([len(b) for b in blocks], dtype=torch.int64)
    recv_n = torch.zeros(n, dtype=torch.int64)
    if dev.type == 'cpu':
        dist.all_to_all_single(recv_n, send_n, group=group)
    else:
        r = recv_n.to(dev)
        dist.all_to_all_single(r, send_n.to(dev), group=group)
        recv_n = r.cpu()
    recv_sizes = [int(x) for x in recv_n.tolist()]
    send = torch.from_numpy(np.concatenate(blocks) if sum(len(b) for b in blocks) else np.zeros(0, dtype=np.uint8)).to(dev)
    recv = torch.empty(sum(recv_sizes), dtype=torch.uint8, device=dev)
    dist.all_to_all_single(recv, send, output_split_sizes=recv_sizes, input_split_sizes=[len(b) for b in blocks], group=group)
    out = recv.cpu().numpy() if dev.type != 'cpu' else recv.numpy()
    cut = np.cumsum(recv_sizes)[:-1]
    return [x.copy() for x in np.split(out, cut)]
