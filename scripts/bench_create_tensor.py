"""What the tensor creation costs from a sorted BAM to the lines Clair's network reads (megapath_nano_amd/clair_tensor.py), stage by
stage: getting the text resident (read, upload, inflate, flatten, walk, the per-record tables), the join, the centre flags, the
host's sampling, the fill, the emission and the download -- wall time, and the device time of the kernels by HIP events.  The two
shapes of scripts/bench_candidates.py, here with qualities (uniform 3 .. 40), both a synthetic sorted BAM of reads with their
alignments (synth.aligned_read: the ONT error mix) written with bam.write_bam:

    amplicon   50 000 reads of 1 kb on a 3 kb contig: every centre is a deep one (flags over tens of thousands of reads, a set, a
               draw of as many numbers, 100 tensors)
    genome     8 kb reads at 50x over 4 Mbp: a hundred thousand shallow centres, one tensor each

The candidates are those the project's own extraction finds (candidates.extract_variant_candidates).  On the amplicon the random
errors of 50 000 reads pass no threshold and it finds none: that run is reported as it is, and the deep path is then measured on
--spaced positions, evenly spread, which is said in the output.

Every shape runs once to warm up and then --repeat times.  Baselines, the only ones there are without samtools: the host build of
the same arithmetic (scripts/tensor_host_check.cpp, g++ -O2, one thread: record facts, join test, flag and fill of EVERY read that
joins a centre over ranges bisected as the device's are -- on a deep centre that is more filling than the 100 x 100 reads the device
fills, and no sampling or text), and the plain-Python restatement of the tests (tests/tensor_ref.py) on a subsample (a file of a
part of the reads), where the device's bytes are also compared with it.  --no-device runs only what needs no GPU.

One JSON line.  The device part cannot run without a GPU: there is no fallback.

    python scripts/bench_create_tensor.py
    python scripts/bench_create_tensor.py --scale 0.02        # a rehearsal size
"""
import argparse
import io
import json
import os
import random
import statistics
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SHAPES = dict(amplicon=dict(contig=3_000, read_len=1_000, reads=50_000, sub_every=50), genome=dict(contig=4_000_000, read_len=8_000, reads=25_000, sub_every=0))
SUB_GENOME = 40_000       # the subsample of the genome shape: the reads that start before this position


def write_shape(d, name, shape, scale, seed=21):
    """-> (bam path, fasta path, subsample bam path, genome bytes, records)"""
    from megapath_nano_amd import bam, synth
    rng = np.random.default_rng(seed)
    n_reads = max(10, int(shape['reads'] * scale))
    genome = synth.random_genome(rng, shape['contig'])
    starts = np.sort(rng.integers(0, shape['contig'] - shape['read_len'] + 1, size=n_reads))
    ref_id = {name: 0}
    recs, sub = [], []
    for i, s in enumerate(starts.tolist()):
        cigar, seq = synth.aligned_read(rng, genome, s, shape['read_len'])
        qual = (rng.integers(3, 41, size=len(seq)).astype(np.uint8) + 33).tobytes().decode()
        rec = bam.encode_record([f'r{i}', '16' if i & 1 else '0', name, str(s + 1), '60', cigar, '*', '0', '0', seq.decode(), qual], ref_id)
        recs.append(rec)
        if (shape['sub_every'] and i % shape['sub_every'] == 0) or (not shape['sub_every'] and s < SUB_GENOME):
            sub.append(rec)
    bam_fn, ref_fn, sub_fn = os.path.join(d, name + '.bam'), os.path.join(d, name + '.fa'), os.path.join(d, name + '.sub.bam')
    header = f'@SQ\tSN:{name}\tLN:{len(genome)}\n'
    bam.write_bam(bam_fn, header, [name], [len(genome)], recs, level=1)
    bam.write_bam(sub_fn, header, [name], [len(genome)], sub, level=1)
    with open(ref_fn, 'wb') as f:
        f.write(b'>' + name.encode() + b'\n' + genome.tobytes() + b'\n')
    return bam_fn, ref_fn, sub_fn, genome.tobytes(), n_reads


def spread(values):
    return dict(mean=round(statistics.fmean(values), 4), sd=round(statistics.pstdev(values), 4), min=round(min(values), 4), max=round(max(values), 4),
                n=len(values))


def own_candidates(name, bam_fn, ref_fn):
    from megapath_nano_amd import candidates
    out = io.BytesIO()
    candidates.extract_variant_candidates(bam_fn, ref_fn, name, out=out)
    return np.array([int(l.split()[1]) for l in out.getvalue().splitlines()], dtype=np.int64)


def device_runs(name, bam_fn, ref_fn, positions, repeat, seed=1):
    import torch
    from megapath_nano_amd import clair_tensor
    runs, text = [], None
    for k in range(repeat + 1):
        timings, out = {}, io.BytesIO()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = clair_tensor.create_tensor(bam_fn, ref_fn, positions, name, rng=random.Random(seed), out=out, timings=timings)
        torch.cuda.synchronize()
        timings['wall'] = time.perf_counter() - t0
        assert text in (None, out.getvalue())            # the same bytes from run to run
        text = out.getvalue()
        if k:
            runs.append(timings)
    keys = sorted(set().union(*runs))
    return dict(centres=len(positions), lines=n, text_bytes=len(text), wall_s=spread([r['wall'] for r in runs]),
                stages={k: round(statistics.fmean(r.get(k, 0) for r in runs), 4) for k in keys}), text


def host_check(d, bam_fn, genome, positions, opt='-O2'):
    """the serial host build on the same text, the records the stage takes and the same ranges -> (seconds it spent on the centres,
    wall seconds with its files)"""
    import bam_in_ref
    from megapath_nano_amd import clair_tensor
    exe = os.path.join(d, 'tensor_host_check')
    subprocess.run(['g++', opt, '-std=c++17', '-o', exe, os.path.join(ROOT, 'scripts', 'tensor_host_check.cpp')], check=True)
    with open(bam_fn, 'rb') as f:
        text = bam_in_ref.inflate(f.read())
    offs, pos, span = [], [], []
    for r in bam_in_ref.walk(text):
        o = r['off']
        p, = struct.unpack_from('<i', text, o + 8)
        n_cigar, = struct.unpack_from('<H', text, o + 16)
        ops = struct.unpack_from('<%dI' % n_cigar, text, o + 36 + r['l_read_name'])
        offs.append(o)
        pos.append(p)
        span.append(sum(w >> 4 for w in ops if (w & 15) in (0, 2, 7, 8)))
    c0 = np.asarray(positions, dtype=np.int64) - 1
    begin, end = clair_tensor.join_ranges(pos, span, c0)
    src, dst = os.path.join(d, 'cases.bin'), os.path.join(d, 'results.bin')
    with open(src, 'wb') as f:
        f.write(struct.pack('<I', 1) + struct.pack('<QqQiII', len(text), 0, len(genome), 1, len(offs), len(c0)) + text + genome)
        f.write(np.asarray(offs, dtype='<i8').tobytes())
        tri = np.zeros(len(c0), dtype=[('c0', '<i4'), ('b', '<u4'), ('e', '<u4')])
        tri['c0'], tri['b'], tri['e'] = c0, begin, end
        f.write(tri.tobytes())
    t0 = time.perf_counter()
    p = subprocess.run([exe, src, dst], check=True, capture_output=True, text=True)
    return float(p.stderr.split()[1]), round(time.perf_counter() - t0, 3)


def restate(sub_fn, genome, name, positions, seed=1):
    import bam_in_ref
    import tensor_ref
    t0 = time.perf_counter()
    with open(sub_fn, 'rb') as f:
        text = bam_in_ref.inflate(f.read())
    lines = tensor_ref.lines(text, genome.decode(), [int(p) for p in positions], name, rng=random.Random(seed))
    return round(time.perf_counter() - t0, 2), lines.encode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=('amplicon', 'genome', 'both'), default='both')
    ap.add_argument('--scale', type=float, default=1.0, help='fraction of the reads of each shape')
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--spaced', type=int, default=30, help='positions the amplicon is measured on when the extraction finds fewer')
    ap.add_argument('--no-restate', action='store_true', help='leave the plain-Python restatement out')
    ap.add_argument('--no-device', action='store_true', help='only the host build and the restatement: runs without a GPU')
    args = ap.parse_args()
    if not args.no_device:
        import torch
        if not torch.cuda.is_available():
            sys.exit('bench_create_tensor.py needs a GPU (or --no-device)')
    res = {}
    for name in (('amplicon', 'genome') if args.shape == 'both' else (args.shape,)):
        shape = SHAPES[name]
        with tempfile.TemporaryDirectory() as d:
            t0 = time.perf_counter()
            bam_fn, ref_fn, sub_fn, genome, reads = write_shape(d, name, shape, args.scale)
            out = dict(reads=reads, contig=shape['contig'], bam_bytes=os.path.getsize(bam_fn), write_s=round(time.perf_counter() - t0, 1))
            spaced = np.linspace(100, shape['contig'] - 100, args.spaced).astype(np.int64)
            if args.no_device:
                positions, out['positions'] = spaced, 'spaced (no device: the extraction did not run)'
            else:
                positions = own_candidates(name, bam_fn, ref_fn)
                out['own_candidates'] = len(positions)
                out['positions'] = 'the extraction\'s own'
                if len(positions) < args.spaced:
                    out['device_own_candidates'] = device_runs(name, bam_fn, ref_fn, positions, 1)[0]
                    positions, out['positions'] = spaced, f'{args.spaced} evenly spaced (the extraction found {out["own_candidates"]})'
                out['device'], _ = device_runs(name, bam_fn, ref_fn, positions, args.repeat)
            out['host_check_centres_s'], out['host_check_wall_s'] = host_check(d, bam_fn, genome, positions)
            sub = positions[positions < SUB_GENOME][:2000] if name == 'genome' else positions
            out['subsample'] = dict(bam_bytes=os.path.getsize(sub_fn), centres=len(sub))
            if not args.no_device:
                dev, text = device_runs(name, sub_fn, ref_fn, sub, 1)
                out['subsample']['device_wall_s'] = dev['wall_s']['mean']
                out['subsample']['lines'] = dev['lines']
            out['subsample']['host_check_centres_s'] = host_check(d, sub_fn, genome, sub)[0]
            if not args.no_restate:
                out['subsample']['restatement_wall_s'], want = restate(sub_fn, genome, name, sub)
                if not args.no_device:
                    out['subsample']['agree'] = bool(want == text)
            res[name] = out
            print(json.dumps({name: out}), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
