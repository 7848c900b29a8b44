"""What nanosplit costs from FASTQ files to the output files: the host path (MPN_READ_INGEST unset: iter_fastx_full, every wanted
record in Python lists, mapper.split_reads, a Python loop that formats the files) beside the device path (MPN_READ_INGEST=device:
the text in HBM, mpn_fastq_scan / heads / name_lookup, the numpy plan, mpn_fastq_emit in rounds) on the same files and the same read
list, with the device path's wall time stage by stage and the device time of its kernels by HIP events.

One synthetic FASTQ of ONT-like reads (Gamma-distributed lengths, UUID ids with a comment) is written in three forms: plain, gzip (one
stream, level 1) and BGZF (blocks of 0xff00 bytes of text made with zlib).  Every read is listed for one of ten outputs, a tenth of
them for a second one.  Every setting runs once to warm up and then --repeat times, the two settings in turns; mean, standard
deviation, minimum and maximum are given.  The same list then goes through fastx.subseq, host and device, on the plain form.  Last,
the lookup alone: --lookup-reads records of 200 bases with UUID ids, all of them listed, in a text that is made on the host and
uploaded whole; the set's construction (host) and ten launches of mpn_fastq_name_lookup (HIP events, and the call's wall time).

One JSON line.  A machine without a GPU cannot run this: there is no fallback.

    python scripts/bench_nanosplit.py
    python scripts/bench_nanosplit.py --reads 2000 --lookup-reads 50000        # a rehearsal size
"""
import argparse
import gzip
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
N_OUT = 10
HEX = np.frombuffer(b'0123456789abcdef', dtype=np.uint8)


def bgzf_block(payload, level=1):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    data = c.compress(payload) + c.flush()
    return (b'\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0' + struct.pack('<H', len(data) + 25) + data +
            struct.pack('<II', zlib.crc32(payload) & 0xffffffff, len(payload)))


def uuids(rng, n):
    """-> uint8 [n, 36]: 8-4-4-4-12 hex digits"""
    a = HEX[rng.integers(0, 16, size=(n, 36))]
    a[:, [8, 13, 18, 23]] = ord('-')
    return a


def write_reads(d, n_reads, mean_len, threads, seed=19):
    """-> (paths by form, the ids, bases, bytes of text)"""
    rng = np.random.default_rng(seed)
    lens = np.maximum(rng.gamma(2.0, mean_len / 2.0, size=n_reads).astype(np.int64), 20)
    acgt = np.frombuffer(b'ACGT', dtype=np.uint8)
    ids = [bytes(u) for u in uuids(rng, n_reads)]
    parts = []
    for i, n in enumerate(lens.tolist()):
        qual = rng.integers(35, 75, size=n).astype(np.uint8)
        parts.append(b'@' + ids[i] + b' runid=bench ch=%d\n' % (i % 512) + acgt[rng.integers(0, 4, size=n)].tobytes() + b'\n+\n' + qual.tobytes() + b'\n')
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
    return paths, ids, int(lens.sum()), len(text)


def write_list(d, ids, out_dir):
    path = os.path.join(d, 'list.tsv')
    with open(path, 'wb') as f:
        for i, rid in enumerate(ids):
            f.write(rid + b'\t' + os.fsencode(os.path.join(out_dir, 'out_%d.fq' % (i % N_OUT))) + b'\n')
            if i % 10 == 3:
                f.write(rid + b'\t' + os.fsencode(os.path.join(out_dir, 'out_%d.fq' % ((i + 5) % N_OUT))) + b'\n')
    return path


def timed(fn):
    import torch
    torch.cuda.synchronize()
    c0, t0 = time.process_time(), time.perf_counter()
    got = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, time.process_time() - c0, got


def set_mode(mode):
    if mode == 'device':
        os.environ['MPN_READ_INGEST'] = 'device'
    else:
        os.environ.pop('MPN_READ_INGEST', None)


def split_once(lst, path, mode, out_dir):
    """files -> output files under one setting -> (stats, a digest of the output files)"""
    import hashlib
    from megapath_nano_amd import fastx
    set_mode(mode)
    timings = {}
    wall, cpu, written = timed(lambda: fastx.nanosplit(lst, [path], timings=timings))
    digest = hashlib.sha256()
    for p, k in written:
        with open(p, 'rb') as f:
            digest.update(b'%d %d ' % (k, os.path.getsize(p)) + hashlib.sha256(f.read()).digest())
    return dict(wall_s=wall, cpu_s=cpu, stages=timings), (digest.hexdigest(), sum(k for _, k in written), sum(os.path.getsize(p) for p, _ in written))


def subseq_once(path, names, mode, d):
    import hashlib
    from megapath_nano_amd import fastx
    set_mode(mode)
    out_path = os.path.join(d, 'subseq.fq')

    def run():
        with open(out_path, 'wb') as out:
            return fastx.subseq(path, names, out)
    wall, cpu, n = timed(run)
    with open(out_path, 'rb') as f:
        return dict(wall_s=wall, cpu_s=cpu), (hashlib.sha256(f.read()).hexdigest(), n)


def spread(values):
    return dict(mean=round(statistics.fmean(values), 4), sd=round(statistics.pstdev(values), 4), min=round(min(values), 4), max=round(max(values), 4),
                n=len(values))


def in_turns(run, repeat):
    """run(mode) -> (stats, what it produced), host and device in turns; the first pair warms up: code objects, pinned and device
    allocations, the page cache -> (timed stats by mode, whether the two always produced the same)"""
    kept, agree = {'host': [], 'device': []}, True
    for k in range(repeat + 1):
        produced = {}
        for mode in ('host', 'device'):
            stats, produced[mode] = run(mode)
            if k:
                kept[mode].append(stats)
        agree = agree and produced['host'] == produced['device']
    return kept, agree, produced['host']


def summary(kept):
    out = {}
    for mode, runs in kept.items():
        out[mode] = dict(wall_s=spread([r['wall_s'] for r in runs]), cpu_s=spread([r['cpu_s'] for r in runs]))
        if mode == 'device' and 'stages' in runs[0]:
            keys = sorted(set().union(*[r['stages'] for r in runs]))
            out[mode]['stages'] = {k: round(statistics.fmean(r['stages'].get(k, 0) for r in runs), 4) for k in keys}
    out['host_over_device'] = round(out['host']['wall_s']['mean'] / out['device']['wall_s']['mean'], 2)
    return out


def lookup_alone(n, launches=10, seed=20):
    """n records of 200 bases, every id listed (in another order) -> the set's construction and the lookup's launches"""
    import torch
    from megapath_nano_amd import fastq_filter as ff
    rng = np.random.default_rng(seed)
    width = 1 + 36 + 1 + 200 + 3 + 200 + 1
    text = np.empty((n, width), dtype=np.uint8)
    text[:, 0] = ord('@')
    text[:, 1:37] = uuids(rng, n)
    text[:, 37] = text[:, 238] = text[:, 240] = text[:, 441] = ord('\n')
    text[:, 38:238] = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, size=(n, 200), dtype=np.int8)]
    text[:, 239] = ord('+')
    text[:, 241:441] = ord('I')
    order = rng.permutation(n)
    names = [bytes(u) for u in text[order, 1:37]]
    heads = np.zeros(n, dtype=ff.FASTQ_HEAD)
    heads['off'], heads['id_len'], heads['comment_len'] = np.arange(n, dtype=np.int64) * width + 1, 36, -1
    d_text = torch.from_numpy(np.concatenate([text.reshape(-1), np.zeros(16, dtype=np.uint8)])).cuda()
    t0 = time.perf_counter()
    name_set = ff.NameSet(names)
    create_s = time.perf_counter() - t0
    want = np.empty(n, dtype=np.int64)
    want[order] = np.arange(n)
    ms, wall, same = [], [], True
    for k in range(launches + 1):                        # the first launch warms up
        wall0, _, found = timed(lambda: ff.fastq_name_lookup(d_text, n * width, heads, name_set))
        if k:
            wall.append(wall0)
            ms.append(ff.last_lookup_device_ms())
        same = same and bool(np.array_equal(found, want))       # (random ids of 128 bits: equal ones are not expected)
    name_set.close()
    return dict(reads=n, text_bytes=n * width, set_create_s=round(create_s, 3), device_ms=spread(ms), call_wall_s=spread(wall), all_found=same,
                note='the call uploads 16 bytes of head per record and downloads 4; create builds the table on the host and uploads it')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=50_000)
    ap.add_argument('--mean-len', type=int, default=8000)
    ap.add_argument('--lookup-reads', type=int, default=2_000_000)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--repeat', type=int, default=3, help='timed runs of either path after one warm-up')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_nanosplit.py needs a GPU')
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        paths, ids, bases, text_bytes = write_reads(d, args.reads, args.mean_len, args.threads)
        out_dir = os.path.join(d, 'out')
        os.makedirs(out_dir)
        lst = write_list(d, ids, out_dir)
        res = dict(reads=args.reads, bases=bases, text_bytes=text_bytes, file_bytes={f: os.path.getsize(p) for f, p in paths.items()},
                   outputs=N_OUT, write_s=round(time.perf_counter() - t0, 2), agree=True)
        print(json.dumps(dict(written=res)), file=sys.stderr, flush=True)
        for form in FORMS:
            kept, agree, produced = in_turns(lambda mode: split_once(lst, paths[form], mode, out_dir), args.repeat)
            out = summary(kept)
            out['records_written'], out['bytes_written'] = produced[1], produced[2]
            res['agree'] = bool(res['agree'] and agree)
            res[form] = out
            print(json.dumps({form: out}), file=sys.stderr, flush=True)
        names = [rid.decode() for rid in ids]
        kept, agree, produced = in_turns(lambda mode: subseq_once(paths['plain'], names, mode, d), args.repeat)
        res['subseq_plain'] = dict(summary(kept), records_written=produced[1])
        res['agree'] = bool(res['agree'] and agree)
        print(json.dumps({'subseq_plain': res['subseq_plain']}), file=sys.stderr, flush=True)
    res['lookup_alone'] = lookup_alone(args.lookup_reads)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
