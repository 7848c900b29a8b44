"""BGZF compression of the payload blocks of a BAM: the device call (mpn_bgzf_compress, both copies included) beside zlib levels 1
and 6 on a thread pool, and the kernels' own time by HIP events.

The blocks are those the BAM writer forms (bam.BgzfWriter's blocking: a record does not straddle blocks) from the records of
--reads synthetic mapped reads (8 kb mean, random ACGT, qualities 5..29, a CIGAR of ~L/7 operations, NM/ms/AS/nn/tp/cm/s1/s2/de/rl
tags as the mapper writes them), or the payloads of an existing file (--bam).  They go to the device --batch at a time, as the
writer hands them over.  One warm-up pass over the first batch, then --rounds timed passes over everything, device and zlib
alternating; the median is reported.

  python scripts/bench_bgzf.py [--reads 100000] [--bam x.bam] [--batch 256] [--threads 16] [--rounds 3]
"""
import argparse
import ctypes as ct
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Sink:
    def write(self, b):
        return len(b)


def synthetic_payloads(n_reads, mean_len, seed):
    from megapath_nano_amd import bam
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.gamma(4.0, mean_len / 4.0, size=n_reads).astype(np.int64), 500, 60000)
    packed_tab = np.array([a << 4 | b for a in (1, 2, 4, 8) for b in (1, 2, 4, 8)], dtype=np.uint8)
    pos = np.sort(rng.integers(0, 25_000_000, size=n_reads))
    payloads = []
    w = bam.BgzfWriter(_Sink(), compress_blocks=lambda p: (payloads.extend(p), [b''] * len(p))[1])
    for i in range(n_reads):
        L = int(lens[i])
        n_ops = max(1, L // 7) | 1
        ops = np.empty(n_ops, dtype=np.uint32)
        ops[0::2] = rng.integers(1, 30, size=(n_ops + 1) // 2).astype(np.uint32) << 4            # M
        ops[1::2] = rng.integers(1, 4, size=n_ops // 2).astype(np.uint32) << 4 | rng.integers(1, 3, size=n_ops // 2).astype(np.uint32)   # I / D
        name = b'read%07d\0' % int(rng.integers(0, n_reads))
        aux = (b'NMS' + struct.pack('<H', L // 10) + b'msS' + struct.pack('<H', L) + b'ASS' + struct.pack('<H', L) + b'nnC\0tpAP' +
               b'cmS' + struct.pack('<H', L // 20) + b's1S' + struct.pack('<H', L // 2) + b's2C\0def' + struct.pack('<f', 0.1) + b'rlC\0')
        rec = (struct.pack('<iiBBHHHiiii', int(pos[i]) // 5_000_000, int(pos[i]) % 5_000_000, len(name), 60, 4681, n_ops, 16 * (i & 1), L, -1, -1, 0) +
               name + ops.tobytes() + packed_tab[rng.integers(0, 16, size=(L + 1) // 2)].tobytes() +
               rng.integers(5, 30, size=L, dtype=np.uint8).tobytes() + aux)
        w.flush_try(4 + len(rec))
        w.write(struct.pack('<i', len(rec)) + rec)
    w.close()
    return payloads


def bam_payloads(path):
    import zlib
    raw = open(path, 'rb').read()
    p, out = 0, []
    while p < len(raw):
        bsize = struct.unpack_from('<H', raw, p + 16)[0] + 1
        data = zlib.decompress(raw[p + 18:p + bsize - 8], -15)
        if data:
            out.append(data)
        p += bsize
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=100000)
    ap.add_argument('--mean-len', type=int, default=8000)
    ap.add_argument('--bam', default=None)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    try:
        import torch      # the order of megapath_nano_amd/_ffi.py hint(): PyTorch initialises the GPU first
        torch.cuda.init()
    except ImportError:
        pass
    from concurrent.futures import ThreadPoolExecutor
    from megapath_nano_amd import _ffi, bam
    lib = _ffi.lib()
    lib.mpn_bgzf_last_device_ms.argtypes = [ct.c_void_p, ct.c_void_p]
    lib.mpn_bgzf_last_device_ms.restype = None
    t0 = time.perf_counter()
    payloads = bam_payloads(args.bam) if args.bam else synthetic_payloads(args.reads, args.mean_len, 7)
    n_bytes = sum(len(p) for p in payloads)
    print(f'{len(payloads)} blocks, {n_bytes / 1e9:.3f} GB of payload ({time.perf_counter() - t0:.1f} s to make)', file=sys.stderr, flush=True)
    batches = [payloads[k:k + args.batch] for k in range(0, len(payloads), args.batch)]
    pool = ThreadPoolExecutor(args.threads)
    dms, pms = ct.c_double(), ct.c_double()

    def device(mode):
        size = dev = pack = 0.0
        t = time.perf_counter()
        for b in batches:
            size += sum(len(x) for x in bam.device_bgzf_blocks(b, mode))
            lib.mpn_bgzf_last_device_ms(ct.byref(dms), ct.byref(pms))
            dev += dms.value
            pack += pms.value
        return time.perf_counter() - t, size, dev, pack

    def host(level):
        size = 0
        t = time.perf_counter()
        for b in batches:
            size += sum(len(x) for x in pool.map(lambda p: bam._bgzf_block(p, level), b))
        return time.perf_counter() - t, size

    bam.device_bgzf_blocks(batches[0])      # warm-up: library, first allocations
    rows = {'device_auto': [], 'device_no_match': [], 'zlib1': [], 'zlib6': []}
    for _ in range(args.rounds):
        rows['device_auto'].append(device(bam.BGZF_AUTO))
        rows['zlib1'].append(host(1))
        rows['device_no_match'].append(device(bam.BGZF_NO_MATCH))
        rows['zlib6'].append(host(6))
    out = {'blocks': len(payloads), 'payload_bytes': n_bytes, 'batch': args.batch, 'threads': args.threads, 'rounds': args.rounds,
           'source': args.bam or f'synthetic, {args.reads} reads'}
    for k, v in rows.items():
        med = sorted(v)[len(v) // 2]
        out[k] = {'wall_s_per_gb': round(med[0] / n_bytes * 1e9, 3), 'min_wall_s_per_gb': round(min(x[0] for x in v) / n_bytes * 1e9, 3),
                  'compressed_bytes': int(med[1]), 'ratio': round(med[1] / n_bytes, 4)}
        if len(med) > 2:
            out[k]['kernel_s_per_gb'] = round(med[2] / 1e3 / n_bytes * 1e9, 4)
            out[k]['pack_kernel_s_per_gb'] = round(med[3] / 1e3 / n_bytes * 1e9, 4)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
