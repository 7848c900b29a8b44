"""What the step between species placement and assembly selection costs (megapath_nano_amd/placement.py, include/mpn_reads.h).

1. The read split: --reads reads of about --mean-len bases, scattered over --groups groups (a twentieth of the reads in two).
   Device time (HIP events inside the library, warm-up excluded) of the plan (mpn_reads_split_plan) and of the gather kernel
   (mpn_reads_split_gather, sources resident), the gather's algorithmic bytes per second -- 2 B per base moved, 4 B with qualities --
   beside the 6.29 TB/s a float4 copy reaches on the MI355X, and the wall time of the calls around them.
2. The same split done the only way there was before: per group a numpy gather on the host (PackedReads of the group's reads) and
   its upload.  The bytes of every group are compared with the device split's.
3. placement_to_assembly on a small strain-rich world (--species species with a species-ID assembly and --candidates further
   candidates each), reads resident: wall time of the whole step and of the mapping calls inside it.

One JSON line per part.  A machine without a GPU cannot run this: there is no fallback.

    python scripts/bench_placement.py
    python scripts/bench_placement.py --reads 2000 --groups 20 --no-map        # a rehearsal size
"""
import argparse
import gzip
import json
import os
import sys
import tempfile
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_COPY_TBS = 6.29      # MI355X, measured float4 copy (8.0 TB/s spec)


def make_batch(n_reads, mean_len, n_groups, quals, seed=1):
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.gamma(4.0, mean_len / 4.0, size=n_reads), 200, 8 * mean_len).astype(np.int32)
    off = np.zeros(n_reads, dtype=np.int64)
    off[1:] = np.cumsum(lens[:-1].astype(np.int64))
    total = int(off[-1] + lens[-1])
    buf = np.zeros(total + 16, dtype=np.uint8)
    buf[:total] = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, size=total, dtype=np.uint8)]
    qbuf = None
    if quals:
        qbuf = np.zeros(total + 16, dtype=np.uint8)
        qbuf[:total] = rng.integers(33, 74, size=total, dtype=np.uint8)
    group = rng.integers(0, n_groups, size=n_reads).astype(np.int32)
    twice = rng.random(n_reads) < 0.05
    mem_read = np.concatenate([np.arange(n_reads, dtype=np.int32), np.flatnonzero(twice).astype(np.int32)])
    mem_group = np.concatenate([group, (group[twice] + 1) % n_groups]).astype(np.int32)
    order = rng.permutation(len(mem_read))                       # the pairs come in no order
    return buf, qbuf, off, lens, mem_read[order], mem_group[order]


def median(xs):
    return float(np.median(xs))


def bench_split(a, torch, mapper):
    buf, qbuf, off, lens, mem_read, mem_group = make_batch(a.reads, a.mean_len, a.groups, a.quals)
    d_buf = torch.from_numpy(buf).cuda()
    d_qbuf = torch.from_numpy(qbuf).cuda() if a.quals else None
    out = dict(part='split', reads=a.reads, groups=a.groups, pairs=int(len(mem_read)), source_bases=int(lens.astype(np.int64).sum()), qualities=bool(a.quals))
    plan_ns, plan_wall = [], []
    for k in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        plan = mapper.device_split_plan(lens, mem_read, mem_group, a.groups)
        if k >= a.warmup:
            plan_wall.append(time.perf_counter() - t0)
            plan_ns.append(mapper.split_last_ns()[0])
    moved = int(lens[plan['out_read']].astype(np.int64).sum())
    sides = 2 if a.quals else 1
    d_out = torch.empty(plan['out_bytes'], dtype=torch.uint8, device='cuda')
    d_qout = torch.empty(plan['out_bytes'], dtype=torch.uint8, device='cuda') if a.quals else None
    gather_ns, gather_wall = [], []
    for k in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        mapper.device_split_gather(plan, buf, off, lens, d_out, qbuf, d_qout, dev_src=(d_buf, d_qbuf), want_host=False)
        if k >= a.warmup:
            gather_wall.append(time.perf_counter() - t0)
            gather_ns.append(mapper.split_last_ns()[1])
    t0 = time.perf_counter()
    h_out, h_qout = mapper.device_split_gather(plan, buf, off, lens, d_out, qbuf, d_qout, dev_src=(d_buf, d_qbuf), want_host=True)
    with_host_copy = time.perf_counter() - t0
    algorithmic = 2 * sides * moved
    out.update(output_reads=plan['n_out'], bases_moved=moved, out_bytes=plan['out_bytes'],
               plan_device_ms=round(median(plan_ns) / 1e6, 3), plan_device_ms_all=[round(x / 1e6, 3) for x in plan_ns], plan_wall_ms=round(median(plan_wall) * 1e3, 2),
               gather_kernel_ms=round(median(gather_ns) / 1e6, 3), gather_kernel_ms_all=[round(x / 1e6, 3) for x in gather_ns],
               gather_wall_ms=round(median(gather_wall) * 1e3, 2), gather_algorithmic_bytes=algorithmic,
               gather_TB_per_s=round(algorithmic / (median(gather_ns) / 1e9) / 1e12, 3), hbm_copy_TB_per_s=HBM_COPY_TBS,
               gather_share_of_hbm_copy=round(algorithmic / (median(gather_ns) / 1e9) / 1e12 / HBM_COPY_TBS, 3),
               gather_with_host_copy_wall_ms=round(with_host_copy * 1e3, 1))
    print(json.dumps(out), flush=True)

    # the route the parent commit offers: a numpy gather per group on the host, and the upload
    order = np.lexsort((mem_read, mem_group))
    key = np.unique(mem_group[order].astype(np.int64) << 32 | mem_read[order])
    g_of, r_of = (key >> 32).astype(np.int64), (key & 0xffffffff).astype(np.int64)
    first = np.searchsorted(g_of, np.arange(a.groups + 1))
    times, same = [], True
    for k in range(1 + max(1, a.calls // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kept = []
        for g in range(a.groups):
            reads = r_of[first[g]:first[g + 1]]
            seqs = [buf[off[r]:off[r] + lens[r]] for r in reads]
            qs = [qbuf[off[r]:off[r] + lens[r]] for r in reads] if a.quals else None
            p = mapper.PackedReads([''] * len(reads), seqs, device='cuda', quals=qs)
            kept.append(p if k == 0 else None)
        torch.cuda.synchronize()
        if k > 0:
            times.append(time.perf_counter() - t0)
        else:
            for g, p in enumerate(kept):
                b0, nb = int(plan['group_byte'][g]), p.bases
                same &= bool(np.array_equal(p.buf[:nb], h_out[b0:b0 + nb])) and (not a.quals or bool(np.array_equal(p.qbuf[:nb], h_qout[b0:b0 + nb])))
        del kept
    host_ms = median(times) * 1e3
    print(json.dumps(dict(part='host_route', reads=a.reads, groups=a.groups, host_gather_and_upload_wall_ms=round(host_ms, 1),
                          host_gather_and_upload_wall_ms_all=[round(x * 1e3, 1) for x in times],
                          device_plan_and_gather_wall_ms=round(median(plan_wall) * 1e3 + median(gather_wall) * 1e3, 2),
                          device_split_equals_host_route=same)), flush=True)


class Metadata:
    def __init__(self, table):
        self.t = table

    def _merge(self, assembly_list, cols, how):
        return assembly_list[['assembly_id']].merge(self.t[['assembly_id'] + cols].drop_duplicates(), on='assembly_id', how=how)

    def get_assembly_path(self, *, assembly_list, how='inner'):
        return self._merge(assembly_list, ['path'], how)

    def get_assembly_length(self, *, assembly_list, how='inner'):
        return self._merge(assembly_list, ['assembly_length'], how)

    def get_tax_id(self, *, assembly_list, how='inner'):
        return self._merge(assembly_list, ['tax_id', 'species_tax_id', 'genus_tax_id'], how)

    def get_sequence_tax_id(self, *, assembly_list, how='inner'):
        return self._merge(assembly_list, ['tax_id', 'species_tax_id', 'genus_tax_id', 'sequence_id'], how)


def bench_mapping(a, torch, mapper):
    from megapath_nano_amd import placement, synth
    rng = np.random.default_rng(9)
    rows, names, seqs, placed = [], [], [], []
    with tempfile.TemporaryDirectory(prefix='bench_placement') as d:
        for s in range(a.species):
            root = synth.random_genome(rng, a.genome_len, gc=float(rng.uniform(0.4, 0.6)))
            kinds = [('id', 0.98)] + [(f'c{k}', float(rng.uniform(0.97, 0.999))) for k in range(a.candidates)]
            made = []
            for kind, ident in kinds:
                aid, g = f'GCF_{s:03d}{kind}.1', synth.mutate_strain(rng, root, ident)
                made.append(g)
                with gzip.open(os.path.join(d, aid + '.fna.gz'), 'wb', compresslevel=1) as f:
                    f.write(b'>NZ_' + aid.encode() + b'\n' + bytes(g) + b'\n')
                rows.append(dict(assembly_id=aid, path=aid + '.fna.gz', assembly_length=len(g), tax_id=len(rows) + 1000, species_tax_id=500 + s, genus_tax_id=50,
                                 sequence_id='NZ_' + aid, kind=kind))
            for r in synth.make_reads(200 + s, [(None, made[1])], a.map_reads // a.species, mean_len=a.map_mean_len):
                names.append(f's{s}_{r["name"]}')
                seqs.append(bytes(r['seq']))
                placed.append(500 + s)
        table = pd.DataFrame(rows)
        order = rng.permutation(len(names))
        packed = mapper.PackedReads([names[i] for i in order], [seqs[i] for i in order], device='cuda')
        kw = dict(assembly_metadata=Metadata(table), global_options=dict(assembly_folder=d, min_alignment_score=0, alignerThreadOption='-t 8', mapping_only=a.mapping_only),
                  target_assembly_list=table[['assembly_id']], species_id_assembly_id=table[table['kind'] == 'id'][['assembly_id']],
                  species_list=pd.DataFrame({'species_tax_id': 500 + np.arange(a.species)}), read_id_species_id=pd.DataFrame({'read_id': names, 'species_tax_id': placed}))
        spent = {'map': 0.0, 'index': 0.0}
        real_map, real_index = mapper.map_batch_full, mapper.Index

        def timed_map(*args, **kwargs):
            t0 = time.perf_counter()
            try:
                return real_map(*args, **kwargs)
            finally:
                spent['map'] += time.perf_counter() - t0

        class TimedIndex(real_index):
            def __init__(self, *args, **kwargs):
                t0 = time.perf_counter()
                super().__init__(*args, **kwargs)
                spent['index'] += time.perf_counter() - t0
        walls = []
        try:
            mapper.map_batch_full, mapper.Index = timed_map, TimedIndex
            for k in range(1 + max(1, a.calls // 2)):
                spent['map'] = spent['index'] = 0.0
                t0 = time.perf_counter()
                align_list, n_cand = placement.placement_to_assembly(reads=[packed], **kw)
                walls.append(time.perf_counter() - t0)
        finally:
            mapper.map_batch_full, mapper.Index = real_map, real_index
        print(json.dumps(dict(part='placement_to_assembly', species=a.species, candidates_per_species=a.candidates, genome_len=a.genome_len, reads=len(names),
                              read_bases=int(packed.bases), mapping_only=bool(a.mapping_only), rows=int(len(align_list)), num_assembly_candidate=n_cand,
                              wall_ms_first=round(walls[0] * 1e3, 1), wall_ms_all=[round(x * 1e3, 1) for x in walls[1:]],
                              last_call_mapping_calls_ms=round(spent['map'] * 1e3, 1), last_call_index_builds_ms=round(spent['index'] * 1e3, 1),
                              last_call_mapping_ms_per_species=round(spent['map'] * 1e3 / a.species, 2))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=100_000)
    ap.add_argument('--mean-len', type=int, default=8000)
    ap.add_argument('--groups', type=int, default=200)
    ap.add_argument('--quals', action='store_true', help='carry qualities through the split (4 B per base moved instead of 2)')
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-split', action='store_true')
    ap.add_argument('--no-map', action='store_true')
    ap.add_argument('--species', type=int, default=20)
    ap.add_argument('--candidates', type=int, default=4)
    ap.add_argument('--genome-len', type=int, default=200_000)
    ap.add_argument('--map-reads', type=int, default=4000)
    ap.add_argument('--map-mean-len', type=int, default=4000)
    ap.add_argument('--mapping-only', action='store_true')
    a = ap.parse_args()
    import torch                                                     # PyTorch first, as bench.py does (megapath_nano_amd/_ffi.py hint())
    torch.cuda.init()
    from megapath_nano_amd import mapper
    if not a.no_split:
        bench_split(a, torch, mapper)
    if not a.no_map:
        bench_mapping(a, torch, mapper)


if __name__ == '__main__':
    main()
