"""What the decoding of Clair's probabilities into VCF records costs (megapath_nano_amd/clair_call.py): the pile-up look-ups
(mpn_call_indels: the BAM streamed to HBM once more, the events of all sites), the decoding (mpn_call_decode), the host's formatting
of the lines, and the whole call -- wall time, and the device time of the kernels by HIP events.  The two shapes of
scripts/bench_create_tensor.py (its files, its positions, the tensors the project's own stage builds from them):

    genome     8 kb reads at 50x over 4 Mbp: a hundred thousand shallow sites
    amplicon   50 000 reads of 1 kb on a 3 kb contig: every site's column is cut by the 250 rule

The probabilities are drawn (seeded): a share --indel-share of the sites is peaked on an indel class (a gt21 of 10 .. 20, a
hetero- or homozygous genotype, lengths away from 0), the others on a SNP or reference class, so that the stated share asks for
look-ups; --pysam_for_all_indel_bases is on, as the reference's driver has it.

Beside it: the plain-Python restatement of the tests (tests/clair_call_ref.py: the closed form of the column, the spelling, the
look-ups and output_with) on a stated subsample of the sites, where the device's lines are also compared with it.  The reference
script and pysam are not run.  One JSON line.  The device part cannot run without a GPU: there is no fallback.

    python scripts/bench_clair_call.py
    python scripts/bench_clair_call.py --scale 0.02        # a rehearsal size
"""
import argparse
import io
import json
import os
import random
import statistics
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


def draw_probs(n, indel_share, seed=3):
    rng = np.random.default_rng(seed)
    p = rng.random((n, 90), dtype=np.float32) * 0.01
    indel = rng.random(n) < indel_share
    for i in range(n):
        if indel[i]:
            p[i, rng.integers(10, 21)] += 1
            p[i, 21 + rng.integers(1, 3)] += 1
            for base in (24, 57):
                v = int(rng.integers(1, 17)) * (1 if rng.random() < 0.5 else -1)
                p[i, base + 16 + v] += 1
        else:
            p[i, rng.integers(0, 10)] += 1
            p[i, 21 + rng.integers(0, 3)] += 1
            p[i, 24 + 16] += 1
            p[i, 57 + 16] += 1
    for a, b in ((0, 21), (21, 24), (24, 57), (57, 90)):
        p[:, a:b] /= p[:, a:b].sum(axis=1, keepdims=True)
    return p, int(indel.sum())


def sam_reads(bam_fn):
    """the records of a BAM file as the restatement wants them: (flag, pos0, cigar, seq)"""
    import bam_in_ref
    with open(bam_fn, 'rb') as f:
        text = bam_in_ref.inflate(f.read())
    letters = np.frombuffer(b'=ACMGRSVTWYHKDBN', dtype=np.uint8)
    out = []
    for r in bam_in_ref.walk(text):
        o = r['off']
        pos, = struct.unpack_from('<i', text, o + 8)
        n_cigar, flag = struct.unpack_from('<HH', text, o + 16)
        l_seq, = struct.unpack_from('<i', text, o + 20)
        at = o + 36 + r['l_read_name']
        ops = struct.unpack_from('<%dI' % n_cigar, text, at)
        packed = np.frombuffer(text, dtype=np.uint8, count=(l_seq + 1) // 2, offset=at + 4 * n_cigar)
        codes = np.stack([packed >> 4, packed & 15], axis=1).reshape(-1)[:l_seq]
        out.append((flag, pos, [('MIDNSHP=X'[w & 15], w >> 4) for w in ops], letters[codes].tobytes().decode()))
    return out


def spread(values):
    return dict(mean=round(statistics.fmean(values), 4), min=round(min(values), 4), max=round(max(values), 4), n=len(values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=('amplicon', 'genome', 'both'), default='both')
    ap.add_argument('--scale', type=float, default=1.0, help='fraction of the reads of each shape')
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--spaced', type=int, default=30, help='positions the amplicon is measured on when the extraction finds fewer')
    ap.add_argument('--indel-share', type=float, default=0.3, help='share of the sites whose probabilities are peaked on an indel class')
    ap.add_argument('--restate-sites', type=int, default=200, help='sites of the subsample the restatement runs on (the amplicon: a fortieth)')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_clair_call.py needs a GPU')
    import bench_create_tensor as bct
    import clair_call_ref as ref
    from megapath_nano_amd import candidates, clair_call, clair_tensor
    res = {}
    for name in (('genome', 'amplicon') if args.shape == 'both' else (args.shape,)):
        shape = bct.SHAPES[name]
        with tempfile.TemporaryDirectory() as d:
            bam_fn, ref_fn, _, genome, reads = bct.write_shape(d, name, shape, args.scale)
            positions = bct.own_candidates(name, bam_fn, ref_fn)
            out = dict(reads=reads, contig=shape['contig'], own_candidates=len(positions), positions='the extraction\'s own')
            if len(positions) < args.spaced:
                positions = np.linspace(100, shape['contig'] - 100, args.spaced).astype(np.int64)
                out['positions'] = f'{args.spaced} evenly spaced (the extraction found {out["own_candidates"]})'
            centres, block, strings = clair_tensor.tensors(bam_fn, ref_fn, positions, name, rng=random.Random(1))
            probs_host, n_indel = draw_probs(len(centres), args.indel_share)
            probs = torch.from_numpy(probs_host).cuda()
            out.update(tensors=len(centres), indel_peaked=n_indel)
            sites = np.unique(np.asarray(centres, dtype=np.int64))
            runs, text = [], None
            for k in range(args.repeat + 1):
                timings = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                events = clair_call.indel_events(bam_fn, name, sites, len(genome), timings=timings)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                rows, alleles, status = clair_call.decode(centres, block, probs, strings, events, genome, pysam_for_all_indel_bases=True)
                t2 = time.perf_counter()
                lines = clair_call.format_rows(name, centres, rows, alleles, 100)
                t3 = time.perf_counter()
                whole = io.BytesIO()
                clair_call.call_variants(bam_fn, ref_fn, name, centres, block, probs, strings, whole, qual=100, pysam_for_all_indel_bases=True)
                torch.cuda.synchronize()
                t4 = time.perf_counter()
                assert whole.getvalue().decode().splitlines() == lines and text in (None, whole.getvalue())
                text = whole.getvalue()
                if k:
                    runs.append(dict(events_wall_s=t1 - t0, events_device_ms=timings.get('indels_device_ms', 0), decode_wall_s=t2 - t1,
                                     decode_device_ms=clair_call.last_device_ms()[1], format_s=t3 - t2, call_variants_wall_s=t4 - t3))
            out['device'] = {k: spread([r[k] for r in runs]) for k in runs[0]}
            out.update(records=len(lines), events=int(events.off[-1]), left_out=int((status == clair_call.LONG_KEY).sum()))
            # ---- the restatement on a subsample of the sites
            n_sub = min(len(centres), args.restate_sites if name == 'genome' else max(1, args.restate_sites // 40))
            pick = np.linspace(0, len(centres) - 1, n_sub).astype(np.int64).tolist()
            t0 = time.perf_counter()
            all_reads = sam_reads(bam_fn)
            t1 = time.perf_counter()
            seq = genome.decode()
            cells = block.reshape(len(centres), -1).cpu().numpy()
            want = []
            for i in pick:
                lo = int(centres[i])
                near = [r for r in all_reads if lo - 70000 <= r[1] <= lo]
                got = ref.output_with(name, lo, strings[i], cells[i], probs_host[i], ref.closed_sequences(near, lo), lambda a, b: seq[a:b], True, False,
                                      False, 100, 'legacy')
                want.append(got[0] if got is not None else None)
            t2 = time.perf_counter()
            by_site = {}
            for row, line in zip(rows, lines):
                by_site[int(row['site'])] = line
            out['restatement'] = dict(sites=n_sub, parse_reads_s=round(t1 - t0, 2), sites_s=round(t2 - t1, 2),
                                      agree=bool(all(by_site.get(i) == w for i, w in zip(pick, want))))
            res[name] = out
            print(json.dumps({name: out}), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
