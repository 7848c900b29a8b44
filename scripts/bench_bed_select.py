"""Wall time of abundance.select_alignment_by_bed with device=True beside device=False on the same seeded input: 2 M alignments
against a BED of 1 M intervals over 20 000 (assembly, sequence) keys, spread evenly (intervals of up to 8 kb that
cover about a twentieth of every sequence; half of the alignments lie on 20 keys).  The call is split into its parts -- the pandas / numpy factorisation of the id columns, the
covered base pairs (mpn_cover_by_bed, uploads and the download included, or the numpy statement), the fraction and the row
selection -- so that the line says where the time goes.  One JSON line.

    python scripts/bench_bed_select.py
    python scripts/bench_bed_select.py --calls 3 --no-host      # the device calls alone, e.g. under rocprofv3
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from megapath_nano_amd import abundance  # noqa: E402


def make(n_align, n_bed, n_keys, seed=1):
    rng = np.random.default_rng(seed)
    n_asm, seq_len = n_keys // 2, 4_000_000
    asm_of = np.array([f'GCF_{i:09d}.1' for i in range(n_asm)], dtype=object)
    seq_of = np.array([f'NZ_CP{i:06d}.1' for i in range(n_keys)], dtype=object)            # key k: assembly k // 2, sequence k
    bk = rng.integers(0, n_keys, size=n_bed)
    bs = rng.integers(0, seq_len, size=n_bed).astype(np.int64)
    bed = pd.DataFrame({'sequence_id': seq_of[bk], 'start': bs, 'end': bs + rng.integers(1, 8000, size=n_bed), 'assembly_id': asm_of[bk // 2]})
    ak = np.where(rng.random(n_align) < 0.5, rng.integers(0, 20, size=n_align), rng.integers(0, n_keys, size=n_align))
    a_from = rng.integers(0, seq_len - 100, size=n_align).astype(np.int64)
    length = np.maximum(50, rng.lognormal(np.log(6000), 0.6, size=n_align)).astype(np.int64)
    al = pd.DataFrame({'read_id': np.arange(n_align), 'assembly_id': asm_of[ak // 2], 'sequence_id': seq_of[ak], 'sequence_from': a_from,
                       'sequence_to': a_from + length})
    return al, bed


def parts(al, bed, device):
    """the body of select_alignment_by_bed(max_overlap=50), timed part by part"""
    t = [time.perf_counter()]
    b_asm, b_seq = abundance._bed_ids(bed)
    code, n_pairs = abundance._pair_codes(np.concatenate([b_asm, abundance._str_objects(al['assembly_id'])]),
                                          np.concatenate([b_seq, abundance._str_objects(al['sequence_id'])]))
    t.append(time.perf_counter())
    q_start, q_end = al['sequence_from'].to_numpy(dtype=np.int64), al['sequence_to'].to_numpy(dtype=np.int64)
    cover = abundance.device_cover_by_bed if device else abundance.host_cover_by_bed
    covered = cover(code[:len(bed)], bed['start'].to_numpy(dtype=np.int64), bed['end'].to_numpy(dtype=np.int64), code[len(bed):], q_start, q_end, n_pairs)
    t.append(time.perf_counter())
    out = al[abundance.overlap_fraction(covered, q_end - q_start) <= 0.5]
    t.append(time.perf_counter())
    return [round((b - a) * 1e3, 2) for a, b in zip(t[:-1], t[1:])], len(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--alignments', type=int, default=2_000_000)
    ap.add_argument('--bed', type=int, default=1_000_000)
    ap.add_argument('--keys', type=int, default=20000)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--no-host', action='store_true', help='skip device=False (and the comparison with it)')
    a = ap.parse_args()
    try:                                                            # PyTorch first, as bench.py does (megapath_nano_amd/_ffi.py hint())
        import torch
        torch.cuda.init()
    except ImportError:
        pass
    al, bed = make(a.alignments, a.bed, a.keys)
    kw = dict(align_list=al, bed=bed, max_overlap=50)
    for _ in range(a.warmup):
        dev = abundance.select_alignment_by_bed(device=True, **kw)
    times = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        dev = abundance.select_alignment_by_bed(device=True, **kw)
        times.append(time.perf_counter() - t0)
    split, _ = parts(al, bed, True)
    out = {'alignments': a.alignments, 'bed_intervals': a.bed, 'keys': a.keys, 'selected': int(len(dev)),
           'device_true_ms_median': round(float(np.median(times)) * 1e3, 1), 'device_true_ms_all': [round(t * 1e3, 1) for t in times],
           'device_true_parts_ms': dict(zip(['factorise_ids', 'cover_by_bed', 'fraction_and_rows'], split))}
    if not a.no_host:
        t0 = time.perf_counter()
        host = abundance.select_alignment_by_bed(device=False, **kw)
        out['device_false_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        out['device_false_parts_ms'] = dict(zip(['factorise_ids', 'cover_by_bed', 'fraction_and_rows'], parts(al, bed, False)[0]))
        out['device_equals_host'] = bool(dev.equals(host))
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
