"""What the read filter costs from a FASTQ file to the filtered file and the statistics table: the host path (MPN_READ_INGEST unset:
the whole file as bytes, parse_fastx, mpn_fastq_qsum_batch on the concatenated qualities, assemble) beside the device path
(fastq_filter.filter_stream: the text in HBM, mpn_fastq_scan / heads / qsum_rows / emit) on the same files, with the device path's wall
time stage by stage and the device time of its kernels by HIP events.

One synthetic FASTQ of ONT-like reads (Gamma-distributed lengths, qualities a random walk like a basecaller's, headers with a
comment) is written in three forms: plain, gzip (one stream, level 1) and BGZF (blocks of 0xff00 bytes of text made with zlib).
The options are the pipeline's: -q 7 -l 500 -h 50 -t 30.  Every setting runs once to warm up and then --repeat times, the two
settings in turns; mean, standard deviation, minimum and maximum are given.  Then the sums kernel alone on the plain text:
mpn_fastq_qsum_rows with and without the ordering by length (ten launches each, in turns), next to mpn_fastq_qsum_batch on the
same qualities (whose call includes joining and uploading them).

One JSON line.  A machine without a GPU cannot run this: there is no fallback.

    python scripts/bench_read_filter.py
    python scripts/bench_read_filter.py --reads 2000        # a rehearsal size
"""
import argparse
import gzip
import io
import json
import os
import statistics
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
OPTIONS = dict(min_quality=7, min_length=500, head_crop=50, tail_crop=30)


def bgzf_block(payload, level=1):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    data = c.compress(payload) + c.flush()
    return (b'\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0' + struct.pack('<H', len(data) + 25) + data +
            struct.pack('<II', zlib.crc32(payload) & 0xffffffff, len(payload)))


def write_reads(d, n_reads, mean_len, threads, seed=18):
    """-> (paths by form, bases, bytes of text)"""
    rng = np.random.default_rng(seed)
    lens = np.maximum(rng.gamma(2.0, mean_len / 2.0, size=n_reads).astype(np.int64), 20)
    acgt = np.frombuffer(b'ACGT', dtype=np.uint8)
    parts = []
    for i, n in enumerate(lens.tolist()):
        # a basecaller's qualities: a walk around a per-read level, so that some reads fail -q 7
        level = rng.uniform(4, 24)
        qual = (np.clip(level + np.cumsum(rng.integers(-2, 3, size=n)), 1, 50) + 33).astype(np.uint8)
        parts.append(b'@read%07d runid=bench ch=%d\n' % (i, i % 512) + acgt[rng.integers(0, 4, size=n)].tobytes() + b'\n+\n' + qual.tobytes() + b'\n')
    text = b''.join(parts)
    del parts
    paths = {form: os.path.join(d, 'reads.' + form) for form in FORMS}
    with open(paths['plain'], 'wb') as f:
        f.write(text)
    with open(paths['gzip'], 'wb') as f:
        f.write(gzip.compress(text, 1))
    with open(paths['bgzf'], 'wb') as f, ThreadPoolExecutor(threads) as pool:
        for block in pool.map(bgzf_block, [text[a:a + BLOCK] for a in range(0, len(text), BLOCK)]):
            f.write(block)
        f.write(EOF_BLOCK)
    return paths, int(lens.sum()), len(text)


def filter_once(path, mode, d):
    """file -> filtered file + statistics file under one setting -> (stats, the two files' bytes)"""
    import torch
    from megapath_nano_amd import fastq_filter as ff
    out_path, info_path = os.path.join(d, 'kept.fq'), os.path.join(d, 'read_info.tsv')
    timings = {}
    torch.cuda.synchronize()
    c0, t0 = time.process_time(), time.perf_counter()
    with open(out_path, 'wb') as out, open(info_path, 'wb') as info:
        if mode == 'device':
            with io.BufferedReader(open(path, 'rb', buffering=0), buffer_size=1 << 20) as stream:
                ff.filter_stream(stream, out, info, timings=timings, **OPTIONS)
        else:           # what bin/mpn-nanofastq does with the knob unset
            os.environ.pop('MPN_READ_INGEST', None)
            with open(path, 'rb') as f:
                o, i, _ = ff.filter_fastx(f.read(), **OPTIONS)
            out.write(o)
            info.write(i)
    torch.cuda.synchronize()
    wall, cpu = time.perf_counter() - t0, time.process_time() - c0
    with open(out_path, 'rb') as f, open(info_path, 'rb') as g:
        produced = (f.read(), g.read())
    return dict(wall_s=wall, cpu_s=cpu, stages=timings), produced


def spread(values):
    return dict(mean=round(statistics.fmean(values), 4), sd=round(statistics.pstdev(values), 4), min=round(min(values), 4), max=round(max(values), 4),
                n=len(values))


def sums_alone(path, repeat):
    """the sums of the plain text's reads three ways -> device ms of mpn_fastq_qsum_rows (ordered, unordered), wall of all three calls"""
    import torch
    from megapath_nano_amd import fastq_filter as ff, ingest
    with open(path, 'rb') as f:
        data = f.read()
    text = torch.from_numpy(np.frombuffer(data + b'\0' * 16, dtype=np.uint8).copy()).cuda()
    rows, consumed, status, _ = ingest.fastq_scan(text, len(data), True)
    assert consumed == len(data) and status == ingest.OK
    h, t, m = OPTIONS['head_crop'], OPTIONS['tail_crop'], OPTIONS['min_length']
    res, ref = {}, None
    variants = (('rows_by_length', True), ('rows_as_scanned', False))
    ms, wall = {key: [] for key, _ in variants}, {key: [] for key, _ in variants}
    for k in range(max(repeat, 10) + 1):                  # the two orders alternate, launch by launch; the first pair warms up
        for key, by_length in variants:
            t0 = time.perf_counter()
            got = ff.qsum_rows(text, len(data), rows, h, t, m, by_length=by_length)
            if k:
                wall[key].append(time.perf_counter() - t0)
                ms[key].append(ff.last_filter_device_ms()[1])
            ref = got if ref is None else ref
            assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1])
    for key, _ in variants:
        res[key] = dict(device_ms=spread(ms[key]), call_wall_s=spread(wall[key]))
    quals = [data[a:a + l] for a, l in zip(rows['qual_off'].tolist(), rows['len'].tolist())]
    wall = []
    for k in range(repeat + 1):
        t0 = time.perf_counter()
        total, cropped = ff.qsums(quals, h, t, m)
        if k:
            wall.append(time.perf_counter() - t0)
    res['qsum_batch'] = dict(call_wall_s=spread(wall), note='joins and uploads the qualities; its kernel is not timed on its own')
    res['same_doubles'] = bool(np.array_equal(ref[0], total) and np.array_equal(ref[1], cropped))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=50_000)
    ap.add_argument('--mean-len', type=int, default=8000)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--repeat', type=int, default=3, help='timed runs of either path after one warm-up')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_read_filter.py needs a GPU')
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        paths, bases, text_bytes = write_reads(d, args.reads, args.mean_len, args.threads)
        res = dict(reads=args.reads, bases=bases, text_bytes=text_bytes, file_bytes={f: os.path.getsize(p) for f, p in paths.items()},
                   options=OPTIONS, write_s=round(time.perf_counter() - t0, 2), agree=True)
        print(json.dumps(dict(written=res)), file=sys.stderr, flush=True)
        for form in FORMS:
            out, produced, timed = {}, {}, {'host': [], 'device': []}
            for k in range(args.repeat + 1):                           # the two settings alternate, run by run
                for mode in ('host', 'device'):
                    stats, produced[mode] = filter_once(paths[form], mode, d)
                    if k:                                              # the first pair warms up: code objects, pinned and device allocations, the page cache
                        timed[mode].append(stats)
            for mode in ('host', 'device'):
                runs = timed[mode]
                out[mode] = dict(wall_s=spread([r['wall_s'] for r in runs]), cpu_s=spread([r['cpu_s'] for r in runs]))
                if mode == 'device':
                    keys = sorted(set().union(*[r['stages'] for r in runs]))
                    out[mode]['stages'] = {k: round(statistics.fmean(r['stages'].get(k, 0) for r in runs), 4) for k in keys}
            res['agree'] = bool(res['agree'] and produced['host'] == produced['device'])
            out['kept_bytes'], out['info_lines'] = len(produced['host'][0]), produced['host'][1].count(b'\n')
            out['host_over_device'] = round(out['host']['wall_s']['mean'] / out['device']['wall_s']['mean'], 2)
            res[form] = out
            del produced
            print(json.dumps({form: out}), file=sys.stderr, flush=True)
        res['sums_alone'] = sums_alone(paths['plain'], args.repeat)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
