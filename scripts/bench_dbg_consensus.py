"""What the de Bruijn graph consensus costs, windows to haplotypes (realigner.consensus_batch -> mpn_dbg_consensus_batch), beside the
serial host build of the same rules (scripts/dbg_host_check.cpp over csrc/dbg_core.h, g++ -O2, one core) -- the only baseline there
is: the reference's library needs Boost and cannot be built.

Workload (seeded): --windows windows of 160 .. 1000 bases, 200 reads of 150 .. 250 bases at 0.5 % substitution errors, every second
read from an alternative haplotype with one to three planted variants (SNP, 3-base insertion, 2-base deletion), a few low-quality
positions per read.  The device's answers are compared with the host build's on every window.  One JSON line.  The device part
cannot run without a GPU: there is no fallback.

    python scripts/bench_dbg_consensus.py [--windows 2000] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def make_window(rng):
    n = int(rng.integers(160, 1001))
    ref = rng.integers(0, 4, n).astype(np.uint8)
    alt = list(ref)
    for v in range(int(rng.integers(1, 4))):
        at = (v + 1) * n // 5 + int(rng.integers(0, 20))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            alt[at] = (alt[at] + 1) % 4
        elif kind == 1:
            alt[at:at] = [int(x) for x in rng.integers(0, 4, 3)]
        else:
            del alt[at:at + 2]
    alt = np.array(alt, dtype=np.uint8)
    lut = np.frombuffer(b'ACGT', dtype=np.uint8)
    reads, bad = [], []
    for i in range(200):
        src = alt if i % 2 else ref
        m = min(int(rng.integers(150, 251)), len(src))
        s = int(rng.integers(0, len(src) - m + 1))
        r = src[s:s + m].copy()
        err = rng.random(m) < 0.005
        r[err] = (r[err] + rng.integers(1, 4, int(err.sum()))) % 4
        reads.append(lut[r].tobytes().decode())
        bad.append({int(x) for x in rng.integers(0, m, int(rng.integers(0, 4)))})
    return lut[ref].tobytes().decode(), reads, bad


def spread(values):
    return dict(median=round(statistics.median(values), 4), min=round(min(values), 4), max=round(max(values), 4), n=len(values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=2000)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    import dbg_cases as dc
    rng = np.random.default_rng(28)
    windows = [make_window(rng) for _ in range(a.windows)]
    bases = sum(len(w[0]) + sum(len(r) for r in w[1]) for w in windows)
    out = dict(windows=a.windows, reads=200 * a.windows, bases=bases)
    with tempfile.TemporaryDirectory() as tmp:
        exe = dc.build_host_check(tmp, optimised=True)
        # the host build starts every window with the table the device would give it (the same rule as dbg_kernels.hip)
        cases = os.path.join(tmp, 'bench_cases.bin')
        with open(cases, 'wb') as f:
            f.write(dc.pack(windows, slots=16384, grow=1))
        host = [json.loads(subprocess.run([exe, 'time', cases], check=True, capture_output=True, text=True).stdout) for _ in range(a.rounds)]
        out['host_serial_s'] = spread([h['ms'] / 1e3 for h in host])
        want = dc.host_run(exe, tmp, windows, slots=16384)
    try:
        import torch
        torch.cuda.init()
    except ImportError:
        pass
    from megapath_nano_amd import realigner
    wins = [dict(ref=r, reads=rd, bad=bad) for r, rd, bad in windows]
    walls, devs, marshal, first = [], [], [], None
    for k in range(a.rounds + 1):
        t0 = time.perf_counter()
        m = realigner._dbg_window_array(wins)
        marshal.append(time.perf_counter() - t0)
        rc, got, redone = realigner.consensus_call(wins, marshalled=m)
        t1 = time.perf_counter()
        assert rc == 0
        assert first in (None, got)                     # identical from run to run
        first = got
        if k:                                           # the first call also loads the code object
            walls.append(t1 - t0)
            devs.append(realigner.consensus_device_ms() / 1e3)
    assert [(s, k, h) for s, k, h in got] == [(s, k, h) for s, k, h, _ in want], 'device and host build differ'
    out.update(device_wall_s=spread(walls), of_which_ctypes_marshalling_s=spread(marshal[1:]), device_kernel_s=spread(devs), windows_redone=redone,
               haplotypes=sum(len(h) for _, _, h in got), k_raised=sum(1 for _, k, _ in got if k > 10),
               empty=sum(1 for _, _, h in got if not h),
               speedup_wall=round(out['host_serial_s']['median'] / statistics.median(walls), 1),
               speedup_kernel=round(out['host_serial_s']['median'] / statistics.median(devs), 1))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
