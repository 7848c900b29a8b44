"""What it costs to get a target set from .fna.gz files to a built index: the host path (fastx: gzip.GzipFile + the readline loop,
mapper.Index) against MPN_TARGET_INGEST=device (megapath_nano_amd/ingest.py: mpn_gzip_inflate + mpn_fasta_scan +
mpn_index_build_device), on N seeded genomes of --genome-len bases written at zlib level 6 in 80-column lines.

Per N (--small, --large) one JSON line: wall time of both paths from files to built index, the host path split into reading and
index build, the device path into read (files -> pinned buffer), H2D, inflate, scan and index build (wall, with the device times of
the two kernels by HIP events beside them).  One more line times a single stream alone: the decode rate of ONE wave, which is what
MPN_INGEST_MAX_STREAM is derived from.  A machine without a GPU cannot run this: there is no fallback.

    python scripts/bench_ingest.py
    python scripts/bench_ingest.py --small 2 --large 4 --genome-len 200000        # a rehearsal size
"""
import argparse
import gzip
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_genomes(d, n, length, seed=1):
    rng = np.random.default_rng(seed)
    paths = []
    for i in range(n):
        seq = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, size=length, dtype=np.uint8)].tobytes()
        p = os.path.join(d, f'GCF_{i:09d}.1_genomic.fna.gz')
        with gzip.open(p, 'wb', compresslevel=6) as f:
            f.write(b'>NZ_BENCH%05d.1 synthetic genome %d\n' % (i, i))
            f.write(b''.join(seq[a:a + 80] + b'\n' for a in range(0, length, 80)))
        paths.append(p)
    return paths


def host_path(paths, batch_bases):
    from megapath_nano_amd import aligner, mapper
    t0 = time.perf_counter()
    read_s = index_s = 0.0
    shape = []
    parts = aligner.iter_target_parts(aligner.iter_target_records(paths), batch_bases)
    while True:
        t = time.perf_counter()
        part = next(parts, None)
        read_s += time.perf_counter() - t
        if part is None:
            break
        t = time.perf_counter()
        idx = mapper.Index(part, k=15, w=10)
        index_s += time.perf_counter() - t
        shape.append((list(idx.names), idx.lens.tolist(), int(idx.n_minimizers)))
        idx.close()
        del part
    return dict(total_s=time.perf_counter() - t0, read_inflate_parse_s=read_s, index_s=index_s), shape


def device_path(paths, batch_bases):
    import torch
    from megapath_nano_amd import ingest
    timings, shape = {}, []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for idx in ingest.iter_target_parts_device(paths, batch_bases, k=15, w=10, timings=timings):
        shape.append((list(idx.names), idx.lens.tolist(), int(idx.n_minimizers)))
        idx.close()
    total = time.perf_counter() - t0
    out = dict(total_s=total)
    out.update({(k if k.endswith('_ms') else k + '_s'): v for k, v in timings.items()})
    return out, shape


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', type=int, default=8)
    ap.add_argument('--large', type=int, default=64)
    ap.add_argument('--genome-len', type=int, default=4_000_000)
    ap.add_argument('--batch-bases', type=int, default=4_000_000_000)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from megapath_nano_amd import ingest
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        paths = write_genomes(d, max(args.small, args.large), args.genome_len)
        gz_bytes = [os.path.getsize(p) for p in paths]
        print(json.dumps(dict(part='files', n=len(paths), genome_len=args.genome_len, gz_bytes_mean=int(np.mean(gz_bytes)),
                              write_s=round(time.perf_counter() - t0, 2))), flush=True)
        device_path(paths[:1], args.batch_bases)         # warm-up: library load, first launches, pinned allocator
        for n in (args.small, args.large):
            host, want = host_path(paths[:n], args.batch_bases)
            dev, got = device_path(paths[:n], args.batch_bases)
            print(json.dumps(dict(part='ingest', n_files=n, bases=n * args.genome_len, same_index=got == want,
                                  host={k: round(v, 4) for k, v in host.items()}, device={k: round(v, 4) for k, v in dev.items()},
                                  speedup=round(host['total_s'] / dev['total_s'], 2))), flush=True)
        # one stream alone: a launch of one wave
        for _ in range(2):
            t = {}
            inf = ingest.inflate_files(paths[:1], timings=t)
        ms = t['inflate_device_ms']
        print(json.dumps(dict(part='single_stream', gz_bytes=gz_bytes[0], text_bytes=int(inf.length[0]), status=int(inf.status[0]),
                              inflate_device_ms=round(ms, 3), gz_mb_per_s=round(gz_bytes[0] / ms / 1e3, 2),
                              text_mb_per_s=round(int(inf.length[0]) / ms / 1e3, 2))), flush=True)


if __name__ == '__main__':
    main()
