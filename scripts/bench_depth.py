"""Time of mpn_depth_by_key (host pointers in and out: the call INCLUDES its uploads and downloads and ends in a stream
synchronise) beside the numpy statement host_depth_by_key on the same input, on seeded intervals shaped like a run's alignment
table: lengths log-normal around 6 kb, 18 000 assemblies x 1-3 sequences of 4 Mbp, half of the intervals on 10 assemblies, a
spike-like depth range per assembly.  One JSON line per size.

    python scripts/bench_depth.py                       # 0.5 M intervals (one bench step's hits) and 20 M (a whole run)
    python scripts/bench_depth.py --sizes 20000000 --calls 3 --no-host      # the device calls alone, e.g. under rocprofv3
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from megapath_nano_amd import abundance  # noqa: E402


def make(n, seed=1):
    rng = np.random.default_rng(seed)
    n_asm, seq_len = 18000, 4_000_000
    per = rng.integers(1, 4, size=n_asm)
    key_group = np.repeat(np.arange(n_asm), per).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(per)[:-1]])
    hot = rng.choice(n_asm, size=10, replace=False)
    asm = np.where(rng.random(n) < 0.5, hot[rng.integers(0, 10, size=n)], rng.integers(0, n_asm, size=n))
    key = (first[asm] + rng.integers(0, 3, size=n) % per[asm]).astype(np.int32)
    length = np.maximum(50, rng.lognormal(np.log(6000), 0.6, size=n)).astype(np.int64)
    start = rng.integers(0, seq_len - 100, size=n).astype(np.int64)
    end = start + length                                           # some cross the sequence end and are clipped
    key_len = np.full(len(key_group), seq_len, dtype=np.int64)
    # depth > mean + 6 sqrt(mean) of each assembly, as the spike filter asks
    bp = np.bincount(asm, weights=length.astype(np.float64), minlength=n_asm) / (per * seq_len)
    lo = (np.maximum(1, (bp + 6 * np.sqrt(bp)).astype(np.int64)) + 1).astype(np.int32)
    hi = np.full(n_asm, 2 ** 31 - 1, dtype=np.int32)
    return dict(key=key, start=start, end=end, key_len=key_len, key_group=key_group, n_groups=n_asm, depth_lo=lo, depth_hi=hi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='500000,20000000')
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--no-host', action='store_true', help='skip the numpy statement (and the comparison with it)')
    a = ap.parse_args()
    try:                                                            # PyTorch first, as bench.py does (megapath_nano_amd/_ffi.py hint())
        import torch
        torch.cuda.init()
    except ImportError:
        pass
    for n in (int(x) for x in a.sizes.split(',')):
        arg = make(n)
        for _ in range(a.warmup):
            dev = abundance.device_depth_by_key(**arg)
        times = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            dev = abundance.device_depth_by_key(**arg)
            times.append(time.perf_counter() - t0)
        out = {'intervals': n, 'events': 2 * n, 'rows': int(len(dev[0][0])), 'bed_rows': int(len(dev[1][0])), 'span_bp': int(dev[2].sum()),
               'device_call_ms_median': round(float(np.median(times)) * 1e3, 2), 'device_call_ms_all': [round(t * 1e3, 2) for t in times]}
        if not a.no_host:
            t0 = time.perf_counter()
            host = abundance.host_depth_by_key(**arg)
            out['host_numpy_ms'] = round((time.perf_counter() - t0) * 1e3, 2)
            out['device_equals_host'] = bool(all(np.array_equal(x, y) for x, y in zip(list(dev[0]) + list(dev[1]) + [dev[2]],
                                                                                      list(host[0]) + list(host[1]) + [host[2]])))
            # what the byte count of DESIGN section 4 needs: the points, i.e. the distinct (key, position) pairs of the events
            e = np.minimum(arg['end'], arg['key_len'][arg['key']])
            on = arg['start'] < e
            k = arg['key'].astype(np.int64) << 32                   # (an interval that contributes nothing leaves its events at 0)
            out['points'] = int(len(np.unique(np.concatenate([k | np.where(on, arg['start'], 0), k | np.where(on, e, 0)]))))
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
