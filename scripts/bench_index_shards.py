"""Index parts sharded over ranks: per-step breakdown of align_and_assign over a ShardedIndex.

    python scripts/bench_index_shards.py --ranks N --shards S [--steps K --warmup W --parts P ...]

Starts N rank processes of itself (or runs as one rank under a launcher that sets RANK / WORLD_SIZE).  The target set is the
strain-rich synthetic set of bench.py --config strain (families of assemblies at 97-99.9 % identity beside random genomes),
generated on the GPU and cut into P index parts; rank r holds the parts of shard r % S and maps the batch of read group r // S.
Per step it prints Gbp/min over the world, bytes exchanged per read, the export / exchange / import / finish seconds next to the
mapping seconds (the slowest rank's), and the peak HBM per rank.

On a one-GPU box run it as a rehearsal: MPN_SINGLE_DEVICE=1 MPN_DIST_BACKEND=gloo puts every rank on cuda:0 and exchanges over
gloo.  The ranks then share one GPU, so the figures measure the overhead of the sharded layout, NOT how it scales; the output
says so.  bench.py stays the yardstick of the product path.
"""
import argparse
import json
import os
import random
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--ranks', type=int, default=2)
    ap.add_argument('--shards', type=int, default=2)
    ap.add_argument('--parts', type=int, default=4, help='index parts the target set is cut into (>= --shards)')
    ap.add_argument('--genomes', type=int, default=1200, help='targets: 1000 strain assemblies (10 families x 100) + random genomes')
    ap.add_argument('--genome-len', type=int, default=200_000)
    ap.add_argument('--reads-per-group', type=int, default=8000, help='reads per step per read group')
    ap.add_argument('--mean-len', type=int, default=6000)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--timeout', type=int, default=600, help='seconds the launcher waits for its ranks')
    return ap.parse_args(argv)


def launch(args):
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(args.ranks):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.ranks), LOCAL_WORLD_SIZE=str(args.ranks),
                   MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), MPN_RANKS_ON_NODE=str(args.ranks))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc, deadline = 0, time.time() + args.timeout
    try:   # a rank that fails ends the run: the others would wait in a collective
        while not rc and any(p.poll() is None for p in procs):
            if time.time() > deadline:
                rc = 124
                break
            time.sleep(0.5)
            rc = max([abs(p.returncode) for p in procs if p.returncode is not None] + [0])
        rc = rc or max(abs(p.returncode) for p in procs)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    sys.exit(rc)


def vram_bytes():
    """HBM this process holds, from the DRM fdinfo of its GPU file descriptors (the library allocates with hipMalloc, which
    torch's allocator statistics do not see).  -> bytes, or -1 where the kernel does not report it."""
    total, seen = 0, False
    try:
        fds = os.listdir('/proc/self/fdinfo')
    except OSError:
        return -1
    clients = set()
    for fd in fds:
        try:
            with open(f'/proc/self/fdinfo/{fd}') as f:
                info = dict(line.split(':', 1) for line in f.read().splitlines() if ':' in line)
        except (OSError, ValueError):
            continue
        key = 'drm-memory-vram' if 'drm-memory-vram' in info else 'vram mem' if 'vram mem' in info else None
        cid = info.get('drm-client-id', fd).strip()
        if key is None or cid in clients:     # (several descriptors may share one DRM client)
            continue
        clients.add(cid)
        val = info[key].split()
        total += int(val[0]) * {'KiB': 1024, 'MiB': 1 << 20, 'GiB': 1 << 30}.get(val[1] if len(val) > 1 else '', 1)
        seen = True
    return total if seen else -1


def log(*a):
    print('[bench_index_shards]', *a, file=sys.stderr, flush=True)


def main():
    args = parse_args()
    if 'WORLD_SIZE' not in os.environ and args.ranks > 1:
        launch(args)      # does not return
    import torch
    import torch.distributed as dist
    from megapath_nano_amd import dist as mdist, mapper, synth
    from megapath_nano_amd.pipeline import ShardedIndex, Taxonomy, align_and_assign
    backend = os.environ.get('MPN_DIST_BACKEND') or None
    single = os.environ.get('MPN_SINGLE_DEVICE') == '1'
    rank, world, local = mdist.init_from_env(backend=backend)
    if world != args.ranks:
        sys.exit(f'--ranks {args.ranks} but WORLD_SIZE={world}')
    group_id, shard = mdist.index_shard_layout(rank, world, args.shards)
    n_groups = world // args.shards
    device = torch.device('cuda', 0 if (world == 1 or single) else local)
    torch.cuda.set_device(device)
    torch.cuda.init()
    if rank == 0:
        from megapath_nano_amd import build
        build.build()
    mdist.barrier()

    # targets: every rank generates the same set, indexes only its own block of parts
    n, glen = args.genomes, args.genome_len
    n_fam, copies = 10, 100
    names, flat, lens = synth.make_genomes_device(20240901, n, glen, 0, device, families=(n_fam, copies, 0.97, 0.999))
    cut = [round(n * p / args.parts) for p in range(args.parts + 1)]
    blocks = mdist.assign_parts([(b - a) * glen for a, b in zip(cut, cut[1:])], args.shards)
    pa, pb = blocks[shard]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    parts = [mapper.Index.from_device(names[cut[p]:cut[p + 1]], flat.data_ptr() + cut[p] * glen, lens[cut[p]:cut[p + 1]])
             for p in range(pa, pb)]
    torch.cuda.synchronize()
    index_s = time.perf_counter() - t0
    groups = mdist.shard_groups(world, args.shards)
    sidx = ShardedIndex(parts, rank, world, args.shards, groups)

    # reads: one batch per read group and step, the same on every shard of the group
    weights = np.zeros(n)
    weights[:n_fam] = np.random.default_rng(7).lognormal(0.0, 1.0, size=n_fam)
    batches = []
    for s in range(args.warmup + args.steps):
        seed = 1000 * (group_id + 1) + s
        buf, off, rl = synth.make_reads_device(seed, flat, glen, args.reads_per_group, weights, device, mean_len=args.mean_len)
        torch.cuda.synchronize()
        rn = [f'g{group_id}s{s}r{i:07d}' for i in range(args.reads_per_group)]
        batches.append(mapper.PackedReads.from_arrays(rn, buf.cpu().numpy(), off.cpu().numpy(), rl.cpu().numpy()))
        del buf, off, rl
    del flat
    torch.cuda.empty_cache()
    tax = Taxonomy(np.arange(n, dtype=np.int32), n, np.arange(n, dtype=np.int32), n)
    opt = mapper.default_opt(best_n=50, pri_ratio=1.0)    # -N 50 -p 1 -x map-ont -c; every part applies its own -f cut-off
    red_device = None if (backend == 'gloo' or not torch.cuda.is_available()) else device
    allreduce = mdist.make_allreduce(red_device)
    rnd = random.Random(12345)
    rows, peak_vram = [], vram_bytes()
    for s, b in enumerate(batches):
        mdist.barrier()
        t0 = time.perf_counter()
        out = align_and_assign(sidx, opt, b, tax, allreduce=allreduce, rng=rnd, shard=(rank, world), use_device=False)
        step_s = time.perf_counter() - t0
        t = sidx.times
        lo, hi = t['owned']
        v = torch.tensor([step_s, t['map_s'], t['export_s'], t['exchange_s'], t['import_s'], t['finish_s']], dtype=torch.float64)
        c = torch.tensor([t['sent_bytes'], hi - lo, b.bases if shard == 0 else 0, out['n_rows']], dtype=torch.int64)
        if world > 1:
            if red_device is not None:
                v, c = v.to(red_device), c.to(red_device)
            dist.all_reduce(v, op=dist.ReduceOp.MAX)
            dist.all_reduce(c, op=dist.ReduceOp.SUM)
            v, c = v.cpu(), c.cpu()
        peak_vram = max(peak_vram, vram_bytes())
        if s >= args.warmup:
            rows.append((v.tolist(), c.tolist()))
            if rank == 0:
                step, mp, ex, xc, im, fi = v.tolist()
                sent, owned, bases, n_rows = c.tolist()
                log(f'step {s - args.warmup + 1}/{args.steps}: {bases / step * 60 / 1e9:.3f} Gbp/min, {sent / max(owned, 1):.0f} B/read '
                    f'exchanged; s (slowest rank): map {mp:.3f} export {ex:.3f} exchange {xc:.3f} import {im:.3f} finish {fi:.3f} '
                    f'step {step:.3f}; {n_rows} rows')
    peak = torch.tensor([peak_vram], dtype=torch.int64)
    hbm = [int(peak.item())]
    if world > 1:
        gathered = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
        if red_device is not None:
            peak = peak.to(red_device)
            gathered = [g.to(red_device) for g in gathered]
        dist.all_gather(gathered, peak)
        hbm = [int(g.item()) for g in gathered]
    sidx.close()
    mdist.barrier()
    if rank != 0:
        return
    K = max(1, len(rows))
    mean = lambda i: sum(r[0][i] for r in rows) / K  # noqa: E731
    tot = lambda i: sum(r[1][i] for r in rows)       # noqa: E731
    step_s = mean(0)
    rehearsal = single or (world > 1 and torch.cuda.device_count() < world)
    res = dict(metric='index_shards_gbp_per_min', ranks=world, shards=args.shards, groups=n_groups, parts=args.parts,
               index_gbp=n * glen / 1e9, reads_per_group=args.reads_per_group, steps=len(rows),
               gbp_per_min=tot(2) / K / step_s * 60 / 1e9 if step_s else 0.0,
               bytes_exchanged_per_read=tot(0) / max(tot(1), 1),
               s_per_step=dict(step=step_s, map=mean(1), export=mean(2), exchange=mean(3), import_=mean(4), finish=mean(5)),
               rows_per_step=tot(3) / K, index_build_s_rank0=index_s, peak_hbm_gb_per_rank=[h / 1e9 if h >= 0 else None for h in hbm],
               backend=dist.get_backend() if world > 1 else None,
               note=('ONE-GPU REHEARSAL: every rank shares cuda:0, so this measures the overhead of the sharded layout, not its '
                     'scaling' if rehearsal else 'one rank per GPU') + '; times are the slowest rank\'s per step')
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
