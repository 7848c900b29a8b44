"""Wall time of abundance.align_list_to_best_align_list with device=True beside device=False on the same seeded, strain-rich table:
about 8 rows a read on 1000 assemblies in species of 100 strains, scores from four adjacent values, so that most reads share
their top score between several assemblies.  Two sizes: about 4 M rows / 500 000 reads, and a tenth of that.  Median of --calls
after --warmup; the call is also split into its parts -- the string coding of read_id and assembly_id, the candidates
(mpn_best_candidates or its numpy statement, transfers included), the abundance statistic over the one-candidate rows, the draws
(random.random on the host), the weighted pick and building the frame.  One JSON line per size.

    python scripts/bench_best_align.py
    python scripts/bench_best_align.py --reference /root/reference/bin/megapath_nano.py     # also the reference's pandas function, small size
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from megapath_nano_amd import abundance  # noqa: E402

PARTS = ['string_codes', 'candidates', 'abundance_statistic', 'draws', 'weighted_pick', 'frame']


def make(n_reads, n_asm=1000, seed=1):
    rng = np.random.default_rng(seed)
    per_read = rng.integers(4, 13, size=n_reads)                     # 8 rows a read on average
    read = np.repeat(np.arange(n_reads), per_read)
    n = len(read)
    species = rng.integers(0, n_asm // 100, size=n_reads)[read]      # a read hits strains of one species
    asm = species * 100 + rng.integers(0, 100, size=n)
    asm_of = np.array([f'GCF_{i:09d}.1' for i in range(n_asm)], dtype=object)
    read_of = np.array([f'read_{i:08d}' for i in range(n_reads)], dtype=object)
    s0 = rng.integers(0, 3_000_000, size=n).astype(np.int64)
    length = np.maximum(200, rng.lognormal(np.log(5000), 0.5, size=n)).astype(np.int64)
    order = rng.permutation(n)
    al = pd.DataFrame({'read_id': read_of[read], 'read_length': 8000, 'assembly_id': asm_of[asm], 'sequence_id': asm_of[asm], 'sequence_length': 4_000_000,
                       'sequence_from': s0, 'sequence_to': s0 + length, 'match': length - 50, 'edit_dist': 50,
                       'alignment_score': 9000 + rng.integers(0, 4, size=n), 'alignment_score_tiebreaker': rng.random(n)}).iloc[order].reset_index(drop=True)
    lens = pd.DataFrame({'assembly_id': asm_of, 'assembly_length': 4_000_000})
    return al, lens


def parts(al, lens, device):
    """the body of align_list_to_best_align_list, timed part by part"""
    t = [time.perf_counter()]
    reads, rc = abundance._codes(al['read_id'])
    asms, ac = abundance._codes(al['assembly_id'])
    t.append(time.perf_counter())
    tiebreak = al['alignment_score_tiebreaker'].to_numpy(dtype=np.float64)
    cand_row, cand_read, count, _ = (abundance.device_best_candidates if device else abundance.host_best_candidates)(
        rc, ac, al['alignment_score'].to_numpy(dtype=np.int64), tiebreak, len(reads), len(asms))
    t.append(time.perf_counter())
    alone = count[cand_read] == 1
    stat = abundance.align_stat_by_assembly_id(al.iloc[cand_row[alone]], lens, None, device=device)
    weight_of = np.zeros(len(asms), dtype=np.int64)
    weight_of[pd.Index(asms).get_indexer(stat['assembly_id'].to_numpy())] = stat['adjusted_total_aligned_bp'].to_numpy(dtype=np.int64)
    weight = weight_of[ac[cand_row]]
    t.append(time.perf_counter())
    draw = np.zeros(len(cand_row))
    draw[~alone] = [random.random() for _ in range(int((~alone).sum()))]
    t.append(time.perf_counter())
    new, winner = (abundance.device_pick_weighted if device else abundance.host_pick_weighted)(cand_read, weight, tiebreak[cand_row], draw, len(reads))
    t.append(time.perf_counter())
    out = al.iloc[cand_row[winner]].copy()
    out['alignment_score_tiebreaker'] = new[winner]
    t.append(time.perf_counter())
    return dict(zip(PARTS, [round((b - a) * 1e3, 1) for a, b in zip(t[:-1], t[1:])])), int(alone.sum()), int(len(cand_row))


def timed(fn, calls, warmup):
    for _ in range(warmup):
        out = fn()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, round(float(np.median(times)) * 1e3, 1), [round(x * 1e3, 1) for x in times]


def reference_function(path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden'))
    import make_best_align_golden as g
    g.REFERENCE = path
    return g.load_reference(), g.Log()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, nargs='*', default=[50_000, 500_000])
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--no-host', action='store_true', help='skip device=False (and the comparison with it)')
    ap.add_argument('--no-device', action='store_true', help='skip device=True (a machine without a GPU)')
    ap.add_argument('--reference', help="path of the reference's bin/megapath_nano.py: time its function on the smallest size")
    a = ap.parse_args()
    if not a.no_device:
        try:                                                        # PyTorch first, as bench.py does (megapath_nano_amd/_ffi.py hint())
            import torch
            torch.cuda.init()
        except ImportError:
            pass
    for k, n_reads in enumerate(sorted(a.reads)):
        al, lens = make(n_reads)
        out = {'rows': int(len(al)), 'reads': n_reads, 'assemblies': 1000}
        results = {}
        for name, device, skip in (('device_true', True, a.no_device), ('device_false', False, a.no_host)):
            if skip:
                continue

            def call():
                random.seed(7)
                return abundance.align_list_to_best_align_list(align_list=al, assembly_length=lens, device=device)
            results[name], out[name + '_ms_median'], out[name + '_ms_all'] = timed(call, a.calls, a.warmup)
            random.seed(7)
            out[name + '_parts_ms'], out['reads_with_one_candidate'], out['candidates'] = parts(al, lens, device)
        if len(results) == 2:
            out['device_equals_host'] = bool(results['device_true'].equals(results['device_false']))
        if a.reference and k == 0:
            ref, log = reference_function(a.reference)
            t0 = time.perf_counter()
            random.seed(7)
            best = ref.align_list_to_best_align_list(assembly_metadata=lens, log=log, align_list=al)
            out['reference_pandas_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
            if results:
                ours = next(iter(results.values()))
                out['reference_equals_ours'] = bool(list(best.index) == list(ours.index) and
                                                    np.array_equal(best['alignment_score_tiebreaker'].to_numpy(), ours['alignment_score_tiebreaker'].to_numpy()))
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
