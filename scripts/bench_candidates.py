"""What the candidate extraction costs from a sorted BAM to the candidate lines (megapath_nano_amd/candidates.py), stage by stage:
wall time of reading, upload, inflate, flatten, walk, the per-record table, the counts, the candidate table and the formatting, and
the device time of the kernels by HIP events.  Two shapes, both a synthetic sorted BAM of reads with their alignments
(synth.aligned_read: the ONT error mix) written with bam.write_bam:

    amplicon   50 000 reads of 1 kb on a 3 kb contig: two tiles, every one split into record slices that add with atomics
    genome     8 kb reads at 50x over 4 Mbp: two thousand tiles with a workgroup each, which store without atomics

Every shape runs once to warm up and then --repeat times.  Then the counts kernel alone at several slice sizes (the records of a
tile one workgroup takes), the host build of the same arithmetic (scripts/pileup_host_check.cpp, g++ -O2, one thread) on the same
text and the same taken records, and with --restate the plain-Python restatement of the tests (tests/pileup_ref.py) on the same
file.  --no-device runs only what needs no GPU (the files are seeded: the same on every machine).

One JSON line.  The device part cannot run without a GPU: there is no fallback.

    python scripts/bench_candidates.py
    python scripts/bench_candidates.py --scale 0.02        # a rehearsal size
"""
import argparse
import io
import json
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = dict(amplicon=dict(contig=3_000, read_len=1_000, reads=50_000), genome=dict(contig=4_000_000, read_len=8_000, reads=25_000))
SLICES = (64, 128, 512, 2048, 1 << 30)


def write_shape(d, name, shape, scale, seed=20):
    """-> (bam path, fasta path, bases, records).  Starts are uniform; the amplicon's reads may start anywhere a read of their length fits."""
    from megapath_nano_amd import bam, synth
    rng = np.random.default_rng(seed)
    n_reads = max(10, int(shape['reads'] * scale))
    genome = synth.random_genome(rng, shape['contig'])
    starts = np.sort(rng.integers(0, shape['contig'] - shape['read_len'] + 1, size=n_reads))
    ref_id = {name: 0}

    def records():
        for i, s in enumerate(starts.tolist()):
            cigar, seq = synth.aligned_read(rng, genome, s, shape['read_len'])
            yield bam.encode_record([f'r{i}', '16' if i & 1 else '0', name, str(s + 1), '60', cigar, '*', '0', '0', seq.decode(), '*'], ref_id)

    bam_fn, ref_fn = os.path.join(d, name + '.bam'), os.path.join(d, name + '.fa')
    bam.write_bam(bam_fn, f'@SQ\tSN:{name}\tLN:{len(genome)}\n', [name], [len(genome)], records(), level=1)
    with open(ref_fn, 'wb') as f:
        f.write(b'>' + name.encode() + b'\n' + genome.tobytes() + b'\n')
    return bam_fn, ref_fn, n_reads * shape['read_len'], n_reads


def spread(values):
    return dict(mean=round(statistics.fmean(values), 4), sd=round(statistics.pstdev(values), 4), min=round(min(values), 4), max=round(max(values), 4),
                n=len(values))


def device_runs(name, bam_fn, ref_fn, repeat):
    import torch
    from megapath_nano_amd import candidates
    runs, lines = [], None
    for k in range(repeat + 1):
        timings, out = {}, io.BytesIO()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = candidates.extract_variant_candidates(bam_fn, ref_fn, name, out=out, timings=timings)
        torch.cuda.synchronize()
        timings['wall'] = time.perf_counter() - t0
        assert lines in (None, out.getvalue())            # the same bytes from run to run
        lines = out.getvalue()
        if k:
            runs.append(timings)
    keys = sorted(set().union(*runs))
    res = dict(lines=n, wall_s=spread([r['wall'] for r in runs]), stages={k: round(statistics.fmean(r.get(k, 0) for r in runs), 4) for k in keys})
    res['count_path'] = 'sliced: atomic adds to HBM' if runs[0]['sliced_tiles'] else 'plain: one workgroup per tile, no atomics'
    # the counts kernel alone: the whole pile-up again at each slice size, its device time summed over the texts of the file
    sweep = {}
    for s in SLICES:
        ms, sliced = [], 0
        for k in range(repeat + 1):
            timings = {}
            p = candidates.pileup(bam_fn, name, timings=timings, slice_records=s)
            sliced = p.sliced_tiles
            if k:
                ms.append(timings.get('counts_device_ms', 0))
        sweep['all' if s == 1 << 30 else str(s)] = dict(counts_device_ms=spread(ms), sliced_tiles=sliced)
    res['slice_sweep'] = sweep
    return res, lines


def host_check(d, bam_fn, name, n_pos):
    """the serial host build on the same text and the same taken records -> wall seconds (the file read and written included)"""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import bam_in_ref
    exe = os.path.join(d, 'pileup_host_check')
    subprocess.run(['g++', '-O2', '-std=c++17', '-o', exe, os.path.join(ROOT, 'scripts', 'pileup_host_check.cpp')], check=True)
    with open(bam_fn, 'rb') as f:
        text = bam_in_ref.inflate(f.read())
    rows, last = [], None
    for r in bam_in_ref.walk(text):
        pos, = struct.unpack_from('<i', text, r['off'] + 8)
        rows.append(struct.pack('<qii', r['off'], 1, int(last is None or pos > last)))
        last = pos
    src, dst = os.path.join(d, 'cases.bin'), os.path.join(d, 'results.bin')
    with open(src, 'wb') as f:
        f.write(struct.pack('<I', 1) + struct.pack('<QqqddI', len(text), 0, n_pos, 4.0, 0.125, len(rows)) + text + b'A' * n_pos + b''.join(rows))
    t0 = time.perf_counter()
    subprocess.run([exe, src, dst], check=True)
    return round(time.perf_counter() - t0, 3)


def restate(bam_fn, ref_fn, name):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import bam_in_ref
    import pileup_ref
    t0 = time.perf_counter()
    with open(bam_fn, 'rb') as f:
        text = bam_in_ref.inflate(f.read())
    with open(ref_fn) as f:
        seq = f.read().split('\n')[1]
    lines = pileup_ref.lines(name, pileup_ref.candidates(pileup_ref.counts(text, name, 0), seq, None, None, 0.125, 4))
    return round(time.perf_counter() - t0, 2), lines.encode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=('amplicon', 'genome', 'both'), default='both')
    ap.add_argument('--scale', type=float, default=1.0, help='fraction of the reads of each shape')
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--restate', action='store_true', help='also time the plain-Python restatement (minutes at full size)')
    ap.add_argument('--no-device', action='store_true', help='only the host build and the restatement: runs without a GPU')
    args = ap.parse_args()
    if not args.no_device:
        import torch
        if not torch.cuda.is_available():
            sys.exit('bench_candidates.py needs a GPU (or --no-device)')
    res = {}
    for name in (('amplicon', 'genome') if args.shape == 'both' else (args.shape,)):
        with tempfile.TemporaryDirectory() as d:
            t0 = time.perf_counter()
            bam_fn, ref_fn, bases, reads = write_shape(d, name, SHAPES[name], args.scale)
            out = dict(reads=reads, bases=bases, contig=SHAPES[name]['contig'], bam_bytes=os.path.getsize(bam_fn), write_s=round(time.perf_counter() - t0, 1))
            lines = None
            if not args.no_device:
                out['device'], lines = device_runs(name, bam_fn, ref_fn, args.repeat)
            out['host_check_wall_s'] = host_check(d, bam_fn, name, SHAPES[name]['contig'])
            if args.restate:
                out['restatement_wall_s'], want = restate(bam_fn, ref_fn, name)
                out['restatement_lines'] = want.count(b'\n')
                if lines is not None:
                    out['agree'] = bool(want == lines)
            res[name] = out
            print(json.dumps({name: out}), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
