"""Wall time of abundance.assembly_selection with device=True beside device=False on the same seeded tables: about 8 rows a read on
1000 assemblies in ten species of 100 strains, scores from 40 adjacent values, a species table and an assembly table of the same
size.  Two sizes: about 4 M rows in all, and about 1 M.  Median of --calls after --warmup; the work is also split into its parts --
the string coding of read_id and assembly_id (np.unique), the device calls or their numpy statements (mpn_good_rows,
mpn_sum_by_key, mpn_cover_by_group, transfers included) and everything else (pandas: the merges, the concat, iloc, the picks).
One JSON line per size.

    python scripts/bench_assembly_selection.py
    python scripts/bench_assembly_selection.py --no-device        # a machine without a GPU: the host form alone
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

CALLS = ['device_good_rows', 'host_good_rows', 'device_sum_by_key', 'host_sum_by_key', 'device_cover_by_group', 'host_cover_by_group']


def make(n_reads, n_asm=1000, seed=1, prefix='read'):
    rng = np.random.default_rng(seed)
    per_read = rng.integers(4, 13, size=n_reads)                     # 8 rows a read on average
    read = np.repeat(np.arange(n_reads), per_read)
    n = len(read)
    species = rng.integers(0, n_asm // 100, size=n_reads)[read]      # a read hits strains of one species
    asm = species * 100 + rng.integers(0, 100, size=n)
    asm_of = np.array([f'GCF_{i:09d}.1' for i in range(n_asm)], dtype=object)
    read_of = np.array([f'{prefix}_{i:08d}' for i in range(n_reads)], dtype=object)
    s0 = rng.integers(0, 3_000_000, size=n).astype(np.int64)
    length = np.maximum(200, rng.lognormal(np.log(5000), 0.5, size=n)).astype(np.int64)
    order = rng.permutation(n)
    return pd.DataFrame({'read_id': read_of[read], 'read_length': 8000, 'assembly_id': asm_of[asm], 'sequence_id': asm_of[asm], 'sequence_length': 4_000_000,
                         'sequence_from': s0, 'sequence_to': s0 + length, 'match': length - 50, 'edit_dist': 50,
                         'alignment_score': 9000 + rng.integers(0, 40, size=n), 'alignment_score_tiebreaker': rng.random(n),
                         'species_tax_id': 1 + species}).iloc[order].reset_index(drop=True)


def inputs(n_reads, n_asm=1000):
    species, assembly = make(n_reads, n_asm, seed=1), make(n_reads, n_asm, seed=2)
    assembly.index = assembly.index + len(species)
    asm_of = [f'GCF_{i:09d}.1' for i in range(n_asm)]
    tax = pd.DataFrame({'assembly_id': asm_of, 'tax_id': np.arange(n_asm) + 1000, 'species_tax_id': 1 + np.arange(n_asm) // 100, 'genus_tax_id': 1, 'genus_height': 2})
    placed = species.drop_duplicates('read_id')[['read_id', 'species_tax_id']]
    return dict(species_align_list=species, assembly_align_list=assembly, species_list=pd.DataFrame({'species_tax_id': np.arange(1, n_asm // 100 + 1)}),
                read_id_species_id=placed, assembly_ID_min_average_depth=0.1, good_align_threshold=99.8,
                assembly_length=pd.DataFrame({'assembly_id': asm_of, 'assembly_length': 4_000_000}), assembly_tax=tax)


class Clock:
    """adds up the time spent inside chosen functions of the abundance module"""
    def __init__(self):
        self.spent, self.saved = {}, {}

    def wrap(self, name, label):
        fn = self.saved[name] = getattr(abundance, name)

        def timed(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                self.spent[label] = self.spent.get(label, 0.0) + time.perf_counter() - t0
        setattr(abundance, name, timed)

    def restore(self):
        for name, fn in self.saved.items():
            setattr(abundance, name, fn)


def parts(kw, device):
    """one call with the string coding and the device calls (or their numpy statements) clocked; the rest is pandas"""
    clock = Clock()
    clock.wrap('_codes', 'string_codes')
    for name in CALLS:
        clock.wrap(name, 'device_calls' if device else 'numpy_statements')
    t0 = time.perf_counter()
    try:
        abundance.assembly_selection(device=device, **kw)
    finally:
        clock.restore()
    total = time.perf_counter() - t0
    out = {k: round(v * 1e3, 1) for k, v in clock.spent.items()}
    out['pandas'] = round((total - sum(clock.spent.values())) * 1e3, 1)
    return out


def timed(fn, calls, warmup):
    for _ in range(warmup):
        out = fn()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, round(float(np.median(times)) * 1e3, 1), [round(x * 1e3, 1) for x in times]


def same(a, b):
    return all(getattr(a, f).equals(getattr(b, f)) for f in ('align_list', 'best_align_list', 'good_align_list', 'align_stat', 'assembly_list', 'species_align_stat'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, nargs='*', default=[62_500, 250_000], help='reads per table; a table has about 8 rows a read')
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--no-host', action='store_true', help='skip device=False (and the comparison with it)')
    ap.add_argument('--no-device', action='store_true', help='skip device=True (a machine without a GPU)')
    a = ap.parse_args()
    if not a.no_device:
        try:                                                        # PyTorch first, as bench.py does (megapath_nano_amd/_ffi.py hint())
            import torch
            torch.cuda.init()
        except ImportError:
            pass
    for n_reads in sorted(a.reads):
        kw = inputs(n_reads)
        out = {'rows': int(len(kw['species_align_list']) + len(kw['assembly_align_list'])), 'reads_per_table': n_reads, 'assemblies': 1000}
        results = {}
        for name, device, skip in (('device_true', True, a.no_device), ('device_false', False, a.no_host)):
            if skip:
                continue
            results[name], out[name + '_ms_median'], out[name + '_ms_all'] = timed(lambda: abundance.assembly_selection(device=device, **kw), a.calls, a.warmup)
            out[name + '_parts_ms'] = parts(kw, device)
        first = next(iter(results.values()))
        out.update(selected_rows=int(len(first.align_list)), good_rows=int(len(first.good_align_list)), assemblies_picked=int(len(first.assembly_list)),
                   species_reached=first.num_species_reached_min_average_depth)
        if len(results) == 2:
            out['device_equals_host'] = bool(same(results['device_true'], results['device_false']))
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
