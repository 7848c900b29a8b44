"""What it costs to get the reads of an unaligned BAM file into a mapper.PackedReads: the device path (ingest.iter_bam_read_batches:
framing, H2D, mpn_gzip_inflate_device, mpn_bam_flatten, mpn_bam_walk, mpn_bam_decode, one download) stage by stage, beside the
same blocks inflated by zlib on the host -- on 1 thread and on --threads threads -- and decoded with numpy.

The file is --reads seeded reads of --mean-len mean length (log-normal), Phred qualities drawn like a basecaller's (a random walk
between 2 and 50), every tenth stored reversed, written at zlib level 1 in blocks of 0xff00 bytes as htslib cuts them.

One JSON line: per path the wall time and the host CPU-seconds of the whole process (time.process_time: all threads), the device
path's wall time per stage with the device times of the kernels by HIP events, the walk's device time per record, and whether the
two paths agree.  A machine without a GPU cannot run this: there is no fallback.

    python scripts/bench_bam_ingest.py
    python scripts/bench_bam_ingest.py --reads 2000 --mean-len 3000        # a rehearsal size
"""
import argparse
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


def bgzf_block(payload, level=1):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    data = c.compress(payload) + c.flush()
    return (b'\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0' + struct.pack('<H', len(data) + 25) + data +
            struct.pack('<II', zlib.crc32(payload) & 0xffffffff, len(payload)))


def write_ubam(path, n_reads, mean_len, threads, seed=1):
    """-> (bases, bytes of BAM text)"""
    rng = np.random.default_rng(seed)
    lens = np.maximum(200, rng.lognormal(np.log(mean_len) - 0.32, 0.8, size=n_reads)).astype(np.int64)
    codes = np.array([1, 2, 4, 8], dtype=np.uint8)
    text_bytes, pending = 0, bytearray(b'BAM\1' + struct.pack('<i', 25) + b'@HD\tVN:1.6\tSO:unsorted\n\0\0' + struct.pack('<i', 0))
    with open(path, 'wb') as f, ThreadPoolExecutor(threads) as pool:
        def drain(everything):
            nonlocal pending, text_bytes
            n_full = len(pending) // BLOCK
            cut = len(pending) if everything else n_full * BLOCK
            view = bytes(pending[:cut])
            for block in pool.map(bgzf_block, [view[a:a + BLOCK] for a in range(0, cut, BLOCK)]):
                f.write(block)
            text_bytes += cut
            del pending[:cut]
        for i, n in enumerate(lens.tolist()):
            nib = codes[rng.integers(0, 4, size=n + (n & 1), dtype=np.uint8)]
            packed = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8)
            if n & 1:
                packed[-1] &= 0xf0
            qual = np.clip(20 + np.cumsum(rng.integers(-2, 3, size=n)), 2, 50).astype(np.uint8)
            name = b'%08x-bench-read-%07d\0' % (seed, i)
            body = struct.pack('<iiBBHHHiiii', -1, -1, len(name), 0, 4680, 0, 4 | (0x10 if i % 10 == 9 else 0), n, -1, -1, 0) + name
            pending += struct.pack('<i', len(body) + len(packed) + n) + body + packed.tobytes() + qual.tobytes()
            if len(pending) >= 256 * BLOCK:
                drain(False)
        drain(True)
        f.write(EOF_BLOCK)
    return int(lens.sum()), text_bytes


def device_path(path, batch_bases):
    import torch
    from megapath_nano_amd import ingest
    timings = {}
    torch.cuda.synchronize()
    c0, t0 = time.process_time(), time.perf_counter()
    batches = list(ingest.iter_bam_read_batches(path, batch_bases, timings=timings))
    torch.cuda.synchronize()
    wall, cpu = time.perf_counter() - t0, time.process_time() - c0
    return batches, dict(wall_s=wall, cpu_s=cpu, stages={k: round(v, 4) for k, v in sorted(timings.items())})


FWD = np.frombuffer(b'=ACMGRSVTWYHKDBN', dtype=np.uint8)
REV = np.frombuffer(b'=TGKCYSBAWRDMHVN', dtype=np.uint8)


def host_path(path, threads):
    """zlib per block on `threads` threads, then a struct walk and a numpy decode -> ((bases, quals) joined, stats)"""
    c0, t0 = time.process_time(), time.perf_counter()
    raw = open(path, 'rb').read()
    spans, p = [], 0
    while p < len(raw):
        size = int.from_bytes(raw[p + 16:p + 18], 'little') + 1
        spans.append((p + 18, p + size - 8))
        p += size
    t1 = time.perf_counter()
    view = memoryview(raw)
    inflate = lambda ab: zlib.decompress(view[ab[0]:ab[1]], -15)  # noqa: E731
    if threads == 1:
        parts = [inflate(s) for s in spans]
    else:
        with ThreadPoolExecutor(threads) as pool:
            parts = list(pool.map(inflate, spans, chunksize=64))
    text = b''.join(parts)
    t2 = time.perf_counter()
    arr = np.frombuffer(text, dtype=np.uint8)
    l_text, = struct.unpack_from('<i', text, 4)
    p = 12 + l_text          # (the file of this benchmark has no references)
    seqs, quals, n = [], [], 0
    while p < len(text):
        block_size, = struct.unpack_from('<i', text, p)
        l_name = text[p + 12]
        n_cigar, flag, l_seq = struct.unpack_from('<HHi', text, p + 16)
        s = p + 36 + l_name + 4 * n_cigar
        q = s + (l_seq + 1) // 2
        packed = arr[s:q]
        nib = np.empty(2 * len(packed), dtype=np.uint8)
        nib[0::2], nib[1::2] = packed >> 4, packed & 15
        if flag & 0x10:
            seqs.append(REV[nib[:l_seq][::-1]])
            quals.append(arr[q:q + l_seq][::-1] + 33)
        else:
            seqs.append(FWD[nib[:l_seq]])
            quals.append(arr[q:q + l_seq] + 33)
        n += 1
        p += 4 + block_size
    out = (np.concatenate(seqs), np.concatenate(quals))
    t3 = time.perf_counter()
    return out, dict(wall_s=t3 - t0, cpu_s=time.process_time() - c0, read_frame_s=t1 - t0, inflate_s=t2 - t1, walk_decode_s=t3 - t2, records=n,
                     blocks=len(spans))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=100_000)
    ap.add_argument('--mean-len', type=int, default=8000)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--batch-bases', type=int, default=200_000_000)
    ap.add_argument('--repeat', type=int, default=2, help='timed runs of the device path after one warm-up')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_bam_ingest.py needs a GPU')
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'reads.bam')
        t0 = time.perf_counter()
        bases, text_bytes = write_ubam(path, args.reads, args.mean_len, args.threads)
        res = dict(reads=args.reads, bases=bases, text_bytes=text_bytes, file_bytes=os.path.getsize(path), write_s=round(time.perf_counter() - t0, 2))
        print(json.dumps(dict(written=res)), file=sys.stderr, flush=True)
        device_path(path, args.batch_bases)                    # warm-up: code objects, pinned and device allocations
        runs = []
        for _ in range(args.repeat):
            batches, stats = device_path(path, args.batch_bases)
            runs.append(stats)
        best = min(runs, key=lambda r: r['wall_s'])
        res['device'] = best
        res['device_wall_all_runs_s'] = [round(r['wall_s'], 3) for r in runs]
        records = best['stages']['records']
        res['walk_us_per_record'] = round(1e3 * best['stages']['walk_device_ms'] / max(records, 1), 4)
        res['walk_launches'] = best['stages']['walk_launches']
        total = sum(int(b.bases) for b in batches)
        got_seq = np.concatenate([b.buf[:b.bases] for b in batches])
        got_qual = np.concatenate([b.qbuf[:b.bases] for b in batches])
        del batches
        for threads in (1, args.threads):
            (seq, qual), stats = host_path(path, threads)
            res[f'zlib_{threads}_threads'] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in stats.items()}
            res['agree'] = bool(res.get('agree', True) and total == len(seq) == bases and np.array_equal(seq, got_seq) and np.array_equal(qual, got_qual))
            del seq, qual
    print(json.dumps(res))


if __name__ == '__main__':
    main()
