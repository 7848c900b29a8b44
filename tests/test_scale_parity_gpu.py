"""GPU parity (-m gpu) at the scale where the seeding regime of the bench workload appears (VERDICT r2 #1a).

The species-placement call of the reference maps against the whole RefSeq target set (/root/reference/bin/lib/aligner.py:219-231,
/root/reference/bin/megapath_nano.py:1262-1275, `-N 50 -p 1 -x map-ont`).  Two target sets are indexed on the GPU and by the
CPU oracle (oracle/mm2_oracle.c, built on the host cores with OpenMP):

  * 250 genomes x 4 Mbp = 1 Gbp incl. 10 strain copies at 99 % identity, k = 15 (map-ont): 64-bit offsets, a 2^26 bucket table,
    the `-f 2e-4` cut-off computed on each side from its own index (they must agree);
  * 100 genomes x 4 Mbp at k = 11: the k-mer space is saturated like the 15-mer space is at 20 Gbp (tens of index positions
    per read minimizer, a three-digit `-f` cut-off), so that long reads overfill the stray-hit filter's counters.

>= 200 sampled reads incl. several >= 30 kb must give PAF text identical to the oracle's, and every line goes through the
independent checker (tests/paf_check.py).
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import paf_check

pytestmark = pytest.mark.gpu


def build_world(n_genomes, glen, strain_pairs, k, seed, n_reads, n_long):
    import torch
    from megapath_nano_amd import mapper, synth
    from oracle import mm2_bindings as mb
    dev = torch.device('cuda', 0)
    os.environ.setdefault('OMP_NUM_THREADS', str(min(16, os.cpu_count() or 1)))
    names, flat, lens = synth.make_genomes_device(seed, n_genomes, glen, strain_pairs, dev)
    torch.cuda.synchronize()
    gidx = mapper.Index.from_device(names, flat.data_ptr(), lens, k=k)
    host = flat.view(n_genomes, glen).cpu().numpy()
    del flat
    torch.cuda.empty_cache()
    gen = [(names[i], host[i]) for i in range(n_genomes)]
    oidx = mb.Index(gen, k=k)
    # community: a few genomes incl. a strain pair; reads of ordinary length + forced long ones (>= 30 kb)
    w = np.zeros(n_genomes)
    w[[0, 1, 2, 3, n_genomes - strain_pairs]] = [4, 2, 1, 1, 2]
    reads = synth.make_reads(seed + 1, gen, n_reads, mean_len=8000, weights=w)
    long_reads = synth.make_reads(seed + 2, gen, n_long, mean_len=45000, min_len=33000, weights=w)
    for i, r in enumerate(long_reads):
        r['name'] = f'long{i:03d}'
    return gen, reads + long_reads, gidx, oidx


def compare(gen, reads, gidx, oidx, k, min_mid_occ):
    from megapath_nano_amd import mapper
    from oracle import mm2_bindings as mb
    mid_g, mid_o = gidx.mid_occ(), oidx.mid_occ()
    assert mid_g == mid_o, f'-f cut-off differs: GPU {mid_g}, oracle {mid_o}'
    assert mid_g >= min_mid_occ, mid_g
    gopt = mapper.default_opt(best_n=50, pri_ratio=1.0, k=k)
    oopt = mb.default_opt(best_n=50, pri_ratio=1.0)
    gopt.mid_occ = oopt.mid_occ = mid_g
    names, seqs = [r['name'] for r in reads], [r['seq'] for r in reads]
    got = mapper.map_batch(gidx, gopt, names, seqs)
    stats = mapper.last_stats()
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        want = list(ex.map(lambda r: mb.map_read(oidx, oopt, r['name'], r['seq'])[2], reads))
    by = {}
    for line in got.splitlines(keepends=True):
        by.setdefault(line.split('\t', 1)[0], []).append(line)
    n_lines = 0
    for r, w_ in zip(reads, want):
        assert ''.join(by.get(r['name'], [])) == w_, (r['name'], len(r['seq']))
        n_lines += w_.count('\n')
    assert sum(1 for w_ in want if w_) >= 0.97 * len(reads)
    # the independent checker over every line (only the targets that were hit are turned into strings)
    hit = {l.split('\t')[5] for l in got.splitlines()}
    gd = {n_: bytes(s_).decode() for n_, s_ in gen if n_ in hit}
    rd = {n_: bytes(s_).decode() for n_, s_ in zip(names, seqs)}
    st = paf_check.check_paf(got, rd, gd, best_n=50, fast=True)
    assert st['lines'] == n_lines and st['as_equal'] >= 0.98 * st['lines']
    return stats, n_lines


def test_one_gbp_index_matches_oracle(libmpn, oracle_built):
    gen, reads, gidx, oidx = build_world(250, 4_000_000, 10, 15, 20240901, 200, 8)
    try:
        assert gidx.n_minimizers > 150_000_000 and sum(len(r['seq']) >= 30000 for r in reads) >= 8
        stats, n_lines = compare(gen, reads, gidx, oidx, 15, 5)
        assert n_lines >= len(reads)
    finally:
        gidx.close()
        oidx.close()


def test_saturated_seed_space_matches_oracle(libmpn, oracle_built):
    """k = 11 over 400 Mbp: ~35 index positions per k-mer, i.e. the regime of 15-mers at 20 Gbp -- the read minimizers find
    tens of hits each, the -f cut-off is in the hundreds and the long reads have more hits than the filter has counters."""
    gen, reads, gidx, oidx = build_world(100, 4_000_000, 4, 11, 777, 200, 6)
    try:
        stats, n_lines = compare(gen, reads, gidx, oidx, 11, 60)
        hits_per_mz = stats['anchors'] / max(stats['minimizers'], 1)
        assert hits_per_mz >= 15, hits_per_mz                      # the bench workload has 26
        assert stats['anchors_emitted'] < stats['anchors']         # the stray-hit filter did drop hits
        longest = max(len(r['seq']) for r in reads)
        assert longest >= 30000 and longest * 0.18 * hits_per_mz > 82000   # more hits than the filter's slots per table
    finally:
        gidx.close()
        oidx.close()


def test_strain_rich_target_set_matches_oracle(libmpn, oracle_built):
    """The regime of the bench headline in small: 40 assemblies of each of 3 community genomes at 97-99.9 % identity beside 30
    unrelated genomes (150 x 600 kb), `-N 50 -p 1`: every read has dozens of loci, i.e. dozens of chain ends (the backtrack runs a
    lane per end), dozens of chains per read in hit_select_kernel (rank sorts, secondaries within the score window; nothing here counts a long
    join: mm_join_long and the edges of the selection have a stage test of their own, test_hit_select_gpu.py), many alignments per read.  PAF identical to the oracle for 120 reads incl. long ones; then the same target set as THREE index
    parts through mpn_map_batch_parts against the oracle's split-index merge."""
    import torch
    from megapath_nano_amd import mapper, synth
    from oracle import mm2_bindings as mb
    dev = torch.device('cuda', 0)
    glen, n_fam, copies, n_rand = 600_000, 3, 40, 30
    n = n_rand + n_fam * copies
    names, flat, lens = synth.make_genomes_device(4711, n, glen, 0, dev, families=(n_fam, copies, 0.97, 0.999))
    torch.cuda.synchronize()
    host = flat.view(n, glen).cpu().numpy()
    gen = [(names[i], host[i]) for i in range(n)]
    gidx = mapper.Index.from_device(names, flat.data_ptr(), lens)
    cut = [0, 50, 100, n]
    gparts = [mapper.Index.from_device(names[a:b], flat.data_ptr() + a * glen, lens[a:b]) for a, b in zip(cut, cut[1:])]
    del flat
    torch.cuda.empty_cache()
    os.environ.setdefault('OMP_NUM_THREADS', str(min(16, os.cpu_count() or 1)))
    oidx = mb.Index(gen)
    oparts = [mb.Index(gen[a:b]) for a, b in zip(cut, cut[1:])]
    w = np.zeros(n)
    w[:n_fam] = [3, 2, 1]
    reads = synth.make_reads(99, gen, 100, mean_len=6000, weights=w) + synth.make_reads(98, gen, 20, mean_len=30000, min_len=20000, weights=w)
    for i, r in enumerate(reads):
        r['name'] = f'sr{i:04d}'
    names_r, seqs = [r['name'] for r in reads], [r['seq'] for r in reads]
    try:
        gopt, oopt = mapper.default_opt(best_n=50, pri_ratio=1.0), mb.default_opt(best_n=50, pri_ratio=1.0)
        got = mapper.map_batch(gidx, gopt, names_r, seqs)
        stats = mapper.last_stats()
        with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
            want = list(ex.map(lambda r: mb.map_read(oidx, oopt, r['name'], r['seq'])[2], reads))
        by = {}
        for line in got.splitlines(keepends=True):
            by.setdefault(line.split('\t', 1)[0], []).append(line)
        for r, w_ in zip(reads, want):
            assert ''.join(by.get(r['name'], [])) == w_, (r['name'], len(r['seq']))
        assert stats['chains'] >= 20 * len(reads), stats['chains']            # dozens of chains per read ...
        assert stats['alignments'] >= 5 * len(reads), stats['alignments']     # ... and many hits kept
        assert stats['reads_hits_on_host'] == 0
        # three resident parts in one call, merged like --split-prefix
        sp = mb.SplitIndex(oparts)
        packed = mapper.PackedReads(names_r, seqs)
        h = mapper.Hits(packed)
        h.add_parts(gparts, gopt)
        paf, _, cols = h.finish(gopt, want_paf=True, want_cols=True)
        h.close()
        want_s = [sp.map_read(oopt, n_, s_) for n_, s_ in zip(names_r, seqs)]
        by = {}
        for line in paf.splitlines(keepends=True):
            by.setdefault(line.split('\t', 1)[0], []).append(line)
        for r, w_ in zip(reads, want_s):
            assert ''.join(by.get(r['name'], [])) == w_, ('parts', r['name'], len(r['seq']))
        # an accumulator that was told there would be no text refuses to make some
        h2 = mapper.Hits(packed, want_text=False)
        h2.add_parts(gparts, gopt)
        _, _, cols2 = h2.finish(gopt, want_paf=False, want_cols=True)
        assert all(np.array_equal(cols[k], cols2[k]) for k in cols)
        with pytest.raises(Exception):
            h2.finish(gopt, want_paf=True, want_cols=False)
        h2.close()
        sp.close()
    finally:
        gidx.close()
        oidx.close()
        for x in gparts + oparts:
            x.close()
