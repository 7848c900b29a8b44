"""What it costs to get the reads of a FASTQ file into a resident mapper.PackedReads: the host path (fastx.iter_fastx behind
aligner.iter_read_batches, MPN_READ_INGEST=host) beside the device path (MPN_READ_INGEST=device: ingest.iter_fastq_read_batches) on the
same files, stage by stage -- read, host-to-device copy, inflate, flatten, scan, gather, device-to-host copy.

One synthetic FASTQ of ONT-like reads (synth.make_reads on seeded genomes, qualities a random walk like a basecaller's) is written in
three forms: plain, gzip (one stream, level 1) and BGZF (blocks of 0xff00 bytes of text made with zlib, as htslib cuts them).  After
the ingest of each form, Align() is called once per setting on the query list of all three forms.

One JSON line: per form and setting the wall time and the CPU-seconds of the whole process, the device path's wall time per stage with
the device times of the kernels by HIP events, whether the two settings gave the same batches, and the Align() call's wall time and
whether its table is the same.  A machine without a GPU cannot run this: there is no fallback.

    python scripts/bench_read_ingest.py
    python scripts/bench_read_ingest.py --reads 300 --mean-len 3000        # a rehearsal size
"""
import argparse
import gzip
import json
import os
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BLOCK = 0xff00
EOF_BLOCK = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')
FORMS = ('plain', 'gzip', 'bgzf')


def bgzf_block(payload, level=1):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    data = c.compress(payload) + c.flush()
    return (b'\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0' + struct.pack('<H', len(data) + 25) + data +
            struct.pack('<II', zlib.crc32(payload) & 0xffffffff, len(payload)))


def write_world(d, n_reads, mean_len, n_genomes, genome_len, threads, seed=1):
    """the genomes as assemblies, the reads as FASTQ in the three forms -> (paths by form, metadata table, bases)"""
    import pandas as pd
    from megapath_nano_amd import synth
    rng = np.random.default_rng(seed)
    gen = synth.make_genomes(seed + 10, n_genomes, genome_len, strain_pairs=1)
    rows = []
    for i, (name, seq) in enumerate(gen):
        p = os.path.join(d, f'asm{i}.fna.gz')
        with open(p, 'wb') as f:
            f.write(gzip.compress(b'>' + name.encode() + b'\n' + bytes(seq) + b'\n', 1))
        rows.append(dict(assembly_id=f'GCF_{i:09d}.1', path=os.path.basename(p), assembly_length=len(seq), tax_id=1000 + i, species_tax_id=500 + i,
                         genus_tax_id=50, sequence_id=name))
    text, bases = bytearray(), 0
    for r in synth.make_reads(seed + 11, gen, n_reads, mean_len=mean_len):
        n = len(r['seq'])
        qual = (np.clip(20 + np.cumsum(rng.integers(-2, 3, size=n)), 2, 50) + 33).astype(np.uint8)
        text += b'@' + r['name'].encode() + b' runid=bench ch=%d\n' % (bases % 512) + bytes(r['seq']) + b'\n+\n' + qual.tobytes() + b'\n'
        bases += n
    text = bytes(text)
    paths = {form: os.path.join(d, form, 'reads.fq' + ('' if form == 'plain' else '.gz')) for form in FORMS}
    for p in paths.values():
        os.makedirs(os.path.dirname(p))
    with open(paths['plain'], 'wb') as f:
        f.write(text)
    with open(paths['gzip'], 'wb') as f:
        f.write(gzip.compress(text, 1))
    with open(paths['bgzf'], 'wb') as f, ThreadPoolExecutor(threads) as pool:
        for block in pool.map(bgzf_block, [text[a:a + BLOCK] for a in range(0, len(text), BLOCK)]):
            f.write(block)
        f.write(EOF_BLOCK)
    return paths, pd.DataFrame(rows), bases, len(text)


def ingest_once(path, mode, batch_bases):
    """file -> resident batches under MPN_READ_INGEST=mode -> (batches, stats)"""
    import torch
    from megapath_nano_amd import aligner, fastx, ingest
    os.environ['MPN_READ_INGEST'] = mode
    timings = {}
    torch.cuda.synchronize()
    c0, t0 = time.process_time(), time.perf_counter()
    if mode == 'device':       # what aligner.iter_read_batches does for one '@' file, with the stage clock handed in
        kind, stream, first = fastx.open_query(path)
        assert first == b'@', (path, kind, first)
        with stream:
            batches = list(ingest.iter_fastq_read_batches(stream, batch_bases, 'cuda', timings, form=kind))
    else:
        batches = list(aligner.iter_read_batches([path], batch_bases, device='cuda'))
    torch.cuda.synchronize()
    wall, cpu = time.perf_counter() - t0, time.process_time() - c0
    return batches, dict(wall_s=round(wall, 4), cpu_s=round(cpu, 4), stages={k: round(v, 4) for k, v in sorted(timings.items())})


def same_batches(a, b):
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x.names != y.names or not (np.array_equal(x.lens, y.lens) and np.array_equal(x.buf, y.buf) and np.array_equal(x.qbuf, y.qbuf)):
            return False
        if not np.array_equal(y.dev[0].cpu().numpy(), x.buf):
            return False
    return True


class Metadata:
    """The joins Align() uses, over an in-memory table."""

    def __init__(self, table):
        self.t = table

    def get_assembly_path(self, *, assembly_list, how='inner'):
        return assembly_list.merge(self.t[['assembly_id', 'path']].drop_duplicates(), on='assembly_id', how=how)

    def get_assembly_length(self, *, assembly_list, how='inner'):
        return assembly_list.merge(self.t[['assembly_id', 'assembly_length']].drop_duplicates(), on='assembly_id', how=how)

    def get_sequence_tax_id(self, *, assembly_list, how='inner'):
        return assembly_list.merge(self.t[['assembly_id', 'tax_id', 'species_tax_id', 'genus_tax_id', 'sequence_id']], on='assembly_id', how=how)


def align_once(d, table, paths, mode):
    import pandas as pd
    import torch
    from megapath_nano_amd import aligner
    os.environ['MPN_READ_INGEST'] = mode
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = aligner.Align(assembly_metadata=Metadata(table), global_options=dict(assembly_folder=d, min_alignment_score=0, debug=False),
                        temp_dir_name=d, log_file=None, query_filename_list=pd.DataFrame({'path': [paths[f] for f in FORMS]}),
                        target_assembly_list=table[['assembly_id']].drop_duplicates().copy(),
                        aligner_options=['-t', '4', '-N', '50', '-p', '1', '-x', 'map-ont'])      # no PAF prefix: the table only
    torch.cuda.synchronize()
    return got, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=10_000)
    ap.add_argument('--mean-len', type=int, default=8000)
    ap.add_argument('--genomes', type=int, default=4)
    ap.add_argument('--genome-len', type=int, default=2_000_000)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--batch-bases', type=int, default=200_000_000)
    ap.add_argument('--repeat', type=int, default=2, help='timed runs of either path after one warm-up')
    ap.add_argument('--no-align', action='store_true')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_read_ingest.py needs a GPU')
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        paths, table, bases, text_bytes = write_world(d, args.reads, args.mean_len, args.genomes, args.genome_len, args.threads)
        res = dict(reads=args.reads, bases=bases, text_bytes=text_bytes, file_bytes={f: os.path.getsize(p) for f, p in paths.items()},
                   write_s=round(time.perf_counter() - t0, 2))
        print(json.dumps(dict(written=res)), file=sys.stderr, flush=True)
        res['agree'] = True
        for form in FORMS:
            out = {}
            for mode in ('host', 'device'):
                ingest_once(paths[form], mode, args.batch_bases)               # warm-up: code objects, pinned and device allocations
                runs = [ingest_once(paths[form], mode, args.batch_bases) for _ in range(args.repeat)]      # the two settings alternate per form
                out[mode] = min((r[1] for r in runs), key=lambda s: s['wall_s'])
                out[mode]['wall_all_runs_s'] = [r[1]['wall_s'] for r in runs]
                out[mode + '_batches'] = runs[-1][0]
                del runs
            res['agree'] = bool(res['agree'] and same_batches(out.pop('host_batches'), out.pop('device_batches')))
            out['gbp_per_min'] = {m: round(bases / out[m]['wall_s'] * 60 / 1e9, 2) for m in ('host', 'device')}
            res[form] = out
            print(json.dumps({form: out}), file=sys.stderr, flush=True)
        if not args.no_align:
            align = {}
            for mode in ('host', 'device', 'host', 'device'):
                got, wall = align_once(d, table, paths, mode)
                align.setdefault(mode + '_wall_s', []).append(round(wall, 3))
                align[mode + '_rows'] = len(got)
                align.setdefault('tables', {})[mode] = got
            tables = align.pop('tables')
            align['same_table'] = bool(tables['host'].reset_index(drop=True).equals(tables['device'].reset_index(drop=True)))
            align['query_gbp'] = round(3 * bases / 1e9, 3)
            res['align_three_forms'] = align
    print(json.dumps(res))


if __name__ == '__main__':
    main()
