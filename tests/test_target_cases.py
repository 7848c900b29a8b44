"""What the worlds of target_cases.py are for, asserted on the CPU oracle alone (no GPU): the GPU parity tests of
test_index_targets_gpu.py compare with the oracle, and a world that had lost its runs, its repeats or its mapped reads would let
them pass on nothing."""
import numpy as np
import pytest

import target_cases as tc


def paf_lines(oidx, reads, **kw):
    from oracle import mm2_bindings as mb
    opt = mb.default_opt(best_n=50, pri_ratio=1.0, **kw)
    return {r['name']: [l.split('\t') for l in mb.map_read(oidx, opt, r['name'], r['seq'])[2].splitlines()] for r in reads}


@pytest.mark.parametrize('variant', ['mult16', 'plus1'])
def test_dirty_world_hits_contain_the_runs(oracle_built, variant):
    from oracle import mm2_bindings as mb
    gen, reads, facts = tc.dirty_world(variant)
    lens = [len(s) for _, s in gen]
    assert facts['total'] == sum(lens) and facts['total'] % 16 == (0 if variant == 'mult16' else 1) and gen[-1][1][-1] == ord('N')
    assert lens[:5] == [0, tc.K - 1, tc.K, tc.K + tc.W - 1, 37] and 120000 < facts['total'] < 140000
    assert lens[facts['n_tail']] % 16 != 0 and facts['n_head'] == facts['n_tail'] + 1
    off = np.concatenate([[0], np.cumsum(lens)])
    t, s, e = facts['named_runs']['16_word']
    assert (off[t] + s) % 16 == 0 and e - s == 16
    t, s, e = facts['named_runs']['at15']
    assert (off[t] + s) % 16 == 15
    assert sorted((off[facts['word_n']] + p) % 32 for p in facts['word_n_pos']) == [0, 15, 16, 31]
    assert len(facts['iupac']) == 30 and bytes(gen[facts['big']][1][facts['lower'][0]:facts['lower'][1]]).islower()
    oidx = mb.Index(gen)   # builds with the empty and the sub-k targets present
    by = paf_lines(oidx, reads)
    oidx.close()
    for key, nn in facts['expect_nn'].items():
        t, s, e = facts['named_runs'][key]
        assert (s, e) in facts['runs'][t] and e - s == int(key)
        lines = by[facts['read_for'][key]]
        assert len(lines) == 1 and lines[0][5] == gen[t][0] and int(lines[0][7]) < s and e < int(lines[0][8]), (key, lines)
        assert f'nn:i:{nn}' in lines[0], (key, lines[0][12:])
    assert len(by[facts['read_for']['1500']]) >= 2
    t, s, e = facts['head_run']
    head = any(f[5] == gen[t][0] and int(f[7]) == e for f in by[facts['read_for']['head']])
    t, s, e = facts['tail_run']
    tail = any(f[5] == gen[t][0] and int(f[8]) == s for f in by[facts['read_for']['tail']])
    assert head or tail
    assert all(by[r['name']] for r in reads), [r['name'] for r in reads if not by[r['name']]]
    assert any(f[4] == '-' for v in by.values() for f in v) and any(f[4] == '+' for v in by.values() for f in v)


def test_repeat_world_mid_occ_regimes(oracle_built):
    from oracle import mm2_bindings as mb
    gen, reads, facts = tc.repeat_world()
    mz = np.concatenate([mb.sketch(s, tc.W, tc.K, i) for i, (_, s) in enumerate(gen)])
    counts = np.sort(np.unique(mz[:, 0] >> np.uint64(8), return_counts=True)[1])
    assert (len(mz), len(counts)) == (facts['n_minimizers'], facts['n_keys'])
    oidx = mb.Index(gen)
    got = {f: oidx.mid_occ(f) for f in facts['mid_occ']}
    oidx.close()
    for f, want in facts['mid_occ'].items():
        assert int(counts[int(np.uint32((1. - float(np.float32(f))) * len(counts)))]) + 1 == got[f] == want, f
    lo, mid, hi = sorted(v - 1 for v in got.values())   # the selected occurrence counts
    assert lo < 1024 <= mid <= 65534 < hi                 # LDS bins | global-atomic bins | the open bin of the GPU's histogram


def test_many_targets_world_reads_map(oracle_built):
    from oracle import mm2_bindings as mb
    gen, reads, facts = tc.many_targets_world()
    lens = np.array([len(s) for _, s in gen])
    assert len(gen) == 5000 and lens.max() <= 700 and 1_500_000 < lens.sum() < 2_000_000
    assert all(lens[i] == 0 for i in facts['empty']) and all(1 <= lens[i] <= 14 for i in facts['tiny'])
    assert len(facts['family']) == 40 and all(lens[i] == 500 for i in facts['family']) and len(reads) == 60
    oidx = mb.Index(gen)
    by = paf_lines(oidx, reads)
    oidx.close()
    assert sum(1 for v in by.values() if v) >= 55
    assert max(len(v) for n, v in by.items() if n.startswith('fam')) >= 10   # a family read hits many of its 40 near-copies
