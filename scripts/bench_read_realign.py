"""What the read realignment costs (megapath_nano_amd/read_realign.py), file to text, stage by stage, on two shapes:

    genome     150-base reads at 100x over a 4 Mbp contig (times --scale) with a SNP, a 3-base deletion or a 4-base insertion planted
               every 1000 bases; reads that meet an indel within 12 bases of an end are soft-clipped there, as a mapper leaves them
    amplicon   50 000 reads of 150 bases (times --scale) on a 3 kb contig with such a variant every 300 bases

    python scripts/bench_read_realign.py device [--scale S] [--shapes genome,amplicon]                          needs a GPU
    python scripts/bench_read_realign.py baseline <reference tree> --samtools PATH [--scale S] [--shapes ...]   CPU only

`device` times realign_file: the text resident (read, upload, inflate, flatten, walk), the device milliseconds of the three new calls
(records, support, assign) and of the consensus, the wall time of realign_windows (consensus and realigner, with their marshalling;
the realigner's own device time cannot be told apart: mpn_realign_batch keeps no device timer, and giving it one is a change to the
realigner, not to this stage -- realign_windows_s minus consensus_device_ms bounds it from above),
and the host's share (the records' checks, the per-read objects, the window rules, the fold, the flush and the text).  `baseline` runs
the reference's own realign_illumina_reads.py, unmodified, under CPython on the same files with a samtools built from the reference
tree outside this repository and tests/golden/dbg_standin.cpp as its graph library, on the CPU machine: the code under test is never
its own baseline.  Both print one JSON line per shape; text_md5 is that of the printed records, which the two modes must share."""
import argparse
import hashlib
import io
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
READ, INS = 150, 'GTCA'
SHAPES = dict(genome=dict(contig=4_000_000, reads=None, coverage=100, every=1000), amplicon=dict(contig=3000, reads=50_000, coverage=None, every=300))
DEVICE_MS = ('records_device_ms', 'support_device_ms', 'assign_device_ms', 'consensus_device_ms', 'inflate_device_ms', 'flatten_device_ms', 'walk_device_ms')
WALL = ('read', 'h2d', 'inflate', 'flatten', 'walk', 'records', 'support', 'host_reads', 'assign', 'marshal', 'realign_windows', 'fold_flush')


def write_shape(d, name, scale, seed=7):
    """-> (SAM path, FASTA path, contig length, reads)"""
    shape, rng = SHAPES[name], random.Random(seed)
    scaled = name == 'genome'
    length = max(int(shape['contig'] * scale), 3000) if scaled else shape['contig']
    n = int(length * shape['coverage'] / READ) if scaled else max(int(shape['reads'] * scale), 100)
    ctg = ''.join(rng.choices('ACGT', k=length))
    sites = list(range(shape['every'] // 2, length - 2 * READ, shape['every']))
    starts = sorted(rng.randrange(0, length - READ - 8) for _ in range(n))
    qual, lines = 'I' * READ, []
    every, half = shape['every'], shape['every'] // 2
    for k, pos in enumerate(starts):
        j = (pos + READ - 1 - half) // every                     # the last site at or before the read's last base
        s = half + every * j if j >= 0 else -1
        kind = j % 3
        if s < pos or s >= sites[-1] + 1 or s + 8 > pos + READ:
            cigar, seq = f'{READ}M', ctg[pos:pos + READ]
        else:
            o = s - pos
            if kind == 0:
                cigar, seq = f'{READ}M', ctg[pos:s] + 'ACGT'[('ACGT'.index(ctg[s]) + 1) % 4] + ctg[s + 1:pos + READ]
            elif kind == 1:                                      # the haplotype lacks ctg[s .. s + 3)
                seq = ctg[pos:s] + ctg[s + 3:pos + READ + 3]
                cigar = f'{o}M3D{READ - o}M' if 12 <= o < READ - 12 else (f'{o}M{READ - o}S' if o >= READ - 12 else None)
                if cigar is None:
                    cigar, pos = f'{o}S{READ - o}M', s + 3
            else:                                                # the haplotype has INS before ctg[s]
                seq = (ctg[pos:s] + INS + ctg[s:pos + READ])[:READ]
                cigar = f'{o}M4I{READ - o - 4}M' if 12 <= o < READ - 16 else (f'{o}M{READ - o}S' if o >= READ - 16 else None)
                if cigar is None:
                    cigar, pos = f'{o + 4}S{READ - o - 4}M', s
        lines.append((pos, f'q{k}\t{16 if k & 1 else 0}\t{name}\t{pos + 1}\t{60 if k % 7 else 30}\t{cigar}\t*\t0\t0\t{seq}\t{qual}\n'))
    lines.sort(key=lambda x: x[0])
    sam, fa = os.path.join(d, name + '.sam'), os.path.join(d, name + '.fa')
    with open(sam, 'w') as f:
        f.write(f'@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:{name}\tLN:{length}\n')
        f.writelines(l for _, l in lines)
    with open(fa, 'w') as f:
        f.write(f'>{name}\n' + ''.join(ctg[i:i + 60] + '\n' for i in range(0, length, 60)))
    return sam, fa, length, n


def device(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_read_realign.py device needs a GPU')
    from megapath_nano_amd import bam, read_realign
    for name in args.shapes.split(','):
        with tempfile.TemporaryDirectory() as d:
            sam, fa, length, n = write_shape(d, name, args.scale)
            bam_fn = os.path.join(d, name + '.bam')
            # (the records stay in the order of the SAM file, which is sorted by position: the names count records in file order)
            bam.sam_to_sorted_bam(sam, bam_fn, index=False, sort_keys=lambda tid, pos, rev: np.arange(len(tid)))
            runs = []
            for _ in range(args.repeat + 1):                     # (the first run warms the library and the allocator up)
                timings, out = {}, io.BytesIO()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = read_realign.realign_file(bam_fn, fa, name, out, timings=timings)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                records = b''.join(l for l in out.getvalue().splitlines(keepends=True) if not l.startswith(b'@'))
                runs.append((wall, timings, got, hashlib.md5(records).hexdigest()))
            wall, timings, got, size = min(runs[1:], key=lambda r: r[0])
            res = dict(shape=name, scale=args.scale, contig=length, records=n, wall_s=round(wall, 3), text_md5=size, **got)
            res.update({k: round(timings.get(k, 0.0), 3) for k in DEVICE_MS})
            res.update({k + '_s': round(timings.get(k, 0.0), 3) for k in WALL})
            res['walls_all'] = [round(r[0], 3) for r in runs]
            print(json.dumps(res), flush=True)


def baseline(args):
    samtools = os.path.abspath(args.samtools)
    src = os.path.join(args.reference, 'bin', 'realignment')
    here = os.path.join(ROOT, 'tests', 'golden')
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(os.path.join(src, 'realign_illumina_reads.py'), d)
        shutil.copytree(os.path.join(src, 'intervaltree'), os.path.join(d, 'intervaltree'))
        os.makedirs(os.path.join(d, 'realign'))
        r = os.path.join(src, 'realign')
        subprocess.check_call(['gcc', '-O2', '-fPIC', '-w', '-c', '-o', os.path.join(d, 'ssw_c.o'), os.path.join(r, 'ssw.c')])
        subprocess.check_call(['g++', '-std=c++14', '-O2', '-fPIC', '-w', '-shared', '-o', os.path.join(d, 'realign', 'realigner'),
                               os.path.join(r, 'realigner.cpp'), os.path.join(r, 'ssw_cpp.cpp'), os.path.join(d, 'ssw_c.o')])
        subprocess.check_call(['g++', '-std=c++17', '-O2', '-fPIC', '-shared', '-o', os.path.join(d, 'realign', 'debruijn_graph'),
                               os.path.join(here, 'dbg_standin.cpp')])
        for name in args.shapes.split(','):
            sam, fa, length, n = write_shape(d, name, args.scale)
            bam_fn = os.path.join(d, name + '.bam')
            subprocess.check_call([samtools, 'view', '-b', '-o', bam_fn, sam])
            subprocess.check_call([samtools, 'index', bam_fn])
            subprocess.check_call([samtools, 'faidx', fa])
            t0 = time.perf_counter()
            text = subprocess.run([sys.executable, os.path.join(d, 'realign_illumina_reads.py'), '--samtools', samtools, '--bam_fn', bam_fn, '--ref_fn', fa,
                                   '--ctgName', name, '--read_fn', 'PIPE'], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
            wall = time.perf_counter() - t0
            records = [l for l in text.decode().splitlines() if not l.startswith('@')]
            print(json.dumps(dict(shape=name, scale=args.scale, contig=length, records=n, wall_s=round(wall, 2), reads=len(records),
                                  text_md5=hashlib.md5(''.join(l + '\n' for l in records).encode()).hexdigest())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest='mode', required=True)
    for mode in ('device', 'baseline'):
        p = sub.add_parser(mode)
        if mode == 'baseline':
            p.add_argument('reference')
            p.add_argument('--samtools', required=True)
        p.add_argument('--scale', type=float, default=1.0)
        p.add_argument('--shapes', default='genome,amplicon')
        p.add_argument('--repeat', type=int, default=2)
    args = ap.parse_args()
    device(args) if args.mode == 'device' else baseline(args)


if __name__ == '__main__':
    main()
