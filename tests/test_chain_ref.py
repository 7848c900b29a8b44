"""CPU tests of the chaining restatement (chain_ref.py) that test_chain_stage_gpu.py holds the chaining kernels to: on every family of
chain_cases.py it equals the oracle's mmo_chain on the (score, count) words and the chained anchors, its chain records equal the
oracle's mm_cal_fuzzy_len (reached through mmo_hits_from_chains, one chain at a time, so that nothing is merged or dropped), and
its record of mechanisms shows that every family reaches what it was built for."""
import numpy as np
import pytest

from chain_cases import FAMILIES, ITER_EDGES, RANDOM_SETS, families
from chain_ref import COUNTERS, chain_ref


@pytest.fixture(scope='module')
def fams():
    return families()


@pytest.fixture(scope='module')
def refs(fams):
    """chain_ref of every read of every case, computed once and left unchanged"""
    return {name: [[chain_ref(c.opt, r) for r in c.reads] for c in cases] for name, cases in fams.items()}


def total(results, key):
    return sum(res[3][key] for res in results)


@pytest.mark.parametrize('family', FAMILIES)
def test_ref_equals_oracle(oracle_built, fams, refs, family):
    from oracle import mm2_bindings as mb
    n_chains = 0
    for c, want in zip(fams[family], refs[family]):
        oopt = mb.default_opt(**c.opt)
        for i, (r, (u, b, recs, _)) in enumerate(zip(c.reads, want)):
            ou, ob = mb.chain(oopt, r)
            assert [int(v) for v in ou] == u, (c.name, i)
            assert np.array_equal(ob, b), (c.name, i)
            k = 0
            for uc, rec in zip(u, recs):
                cnt = uc & 0xffffffff
                ch = b[k:k + cnt]
                k += cnt
                regs, _ = mb.hits_from_chains(oopt, 15, None, 1 << 30, [uc], ch)
                assert len(regs) == 1 and regs[0]['cnt'] == cnt
                assert rec == (int(ch[0, 0]), int(ch[0, 1]), int(ch[-1, 0]), int(ch[-1, 1]), regs[0]['mlen'], regs[0]['blen']), (c.name, i, rec)
            assert k == len(b)
            n_chains += len(u)
    assert n_chains > 0


def test_families_reach_their_mechanisms(fams, refs):
    by = {c.name: res for name in FAMILIES for c, res in zip(fams[name], refs[name])}
    d = by['diag'][0]
    assert len(d[0]) == 1 and d[3]['skip_break'] >= 250                  # the walk breaks on nearly every anchor
    g = by['grid'][0]
    assert g[3]['skip_break'] >= 1 and g[3]['far128'] >= 1000 and g[3]['far_tile'] >= 1000
    for v in (50, 63, 64, 65, 127, 128, 129):
        assert by['grid iter %d' % v][0][3]['iter_cut'] >= 1000
    assert by['grid skip 0'][0][3]['skip_break'] > g[3]['skip_break'] and by['grid iter 129'][0][3]['far128'] >= 1000
    # the jittered lattice: the options change the chains
    j = by['jittered'][0]
    assert j[3]['far128'] >= 1000 and j[3]['skip_break'] >= 500
    for name in ('jittered skip 0', 'jittered skip 3', 'jittered iter 50'):
        assert by[name][0][0] != j[0], name
    # the predecessor exactly N back is out of reach at max_chain_iter N - 1 and in reach from N
    pair = lambda name: [(u >> 32, u & 0xffffffff) for u in by[name][0][0]]  # noqa: E731
    for n in ITER_EDGES:
        assert pair('iter edge %d at %d' % (n, n - 1)) == [(150, 10)] and by['iter edge %d at %d' % (n, n - 1)][0][3]['iter_cut'] >= 1
        assert pair('iter edge %d at %d' % (n, n)) == [(165, 11)] and pair('iter edge %d at %d' % (n, n + 1)) == [(165, 11)]
    # 60 anchors at steps of 30 000 000 (each sees two predecessors in range), 30 at steps of exactly max_gap, 20 at steps of 20
    assert sorted(pair('widest gap')) == [(15 * 20, 20), (15 * 30, 30), (15 * 60, 60)]
    assert by['peak'][0][3]['peak_back'] >= 1
    t4, t6, tc, tc4 = by['trunk']
    assert len(t4[0]) == 1 and t4[3]['stop_taken'] == 1 and t4[3]['sub_reject'] == 1 and t4[3]['branch'] >= 1
    assert len(t6[0]) == 2 and t6[3]['stop_taken'] == 1 and t6[3]['sub_reject'] == 0
    assert min(t6[0]) >> 32 == 54                                        # the branch keeps its score less the trunk's at the fork
    # C's two anchors score 400 and fail min_cnt; D stops at C's first anchor, which stays taken, and is kept with its score less 200
    assert tc[3]['cnt_reject'] == 1 and tc[3]['discarded_taken_hit'] == 1 and len(tc[0]) == 2 and min(tc[0]) & 0xffffffff == 6
    assert tc4[3]['cnt_reject'] == 1 and tc4[3]['discarded_taken_hit'] == 1 and tc4[3]['sub_reject'] == 1 and len(tc4[0]) == 2
    rnd = [res for s in range(RANDOM_SETS) for res in by['random %d' % s]]
    for key in COUNTERS:
        assert total(rnd, key) >= 1, key
    assert total(rnd, 'discarded_taken_hit') >= 4
    m, m46 = by['many ends'][0], by['many ends 46'][0]
    assert m[3]['n_ends'] == 600 and len(m[0]) == 600 and m46[3]['n_ends'] == 150 and len(m46[0]) == 150
    one, two = by['big segment']
    assert one[3]['n_ends'] >= 65 and one[3]['stop_taken'] >= 65 and len(one[0]) == 1 and len(two[0]) == 2
    # per read 500 segments of each size; the step of exactly max_gap is beyond the band width and cuts one segment's chain in two:
    # of read 0 a segment of three (nothing is left), of read 1 one of four (three are), of read 2 one of two
    chains = lambda name: [len(r[0]) for r in by[name]]  # noqa: E731
    for mc in (1, 2, 3):
        assert chains('compaction min_cnt %d' % mc) == [999, 1000, 1000]            # (two anchors score 30, below min_chain_score)
    assert chains('compaction min_cnt 4') == [500, 499, 500] and chains('compaction min_cnt 5') == [0, 0, 0]
    # at min_chain_score 10 every piece is a chain: one more per read; with min_cnt 2 the cut segment of two (read 2) leaves none
    assert chains('compaction min_cnt 1 score 10') == [1501, 1501, 1501] and chains('compaction min_cnt 2 score 10') == [1500, 1500, 1499]
    # 32 segments, eight of each size; the cut takes one anchor off a segment of 100, 63, 64 and 65 in turn
    assert [sum(chains('compaction saturated %d' % mc)) for mc in (64, 65, 100)] == [32 - 9, 32 - 17, 7]
    assert [total(by['compaction saturated %d' % mc], 'cnt_reject') for mc in (64, 65, 100)] == [9, 17, 25]
    ts = by['targets and strands']
    assert len(ts[0][0]) == 14 and len(ts[1][0]) == 2 and all(int(y) >> 40 for r in ts for y in r[1][:, 1])
    gc = by['gap cost']
    # two anchors alone part where the step costs more than it gains; the runs of seven to either side of the step chain across every
    # offset, and the step's cost, 0 .. 85 and some at an average seed length of 16.33, shows in the score
    assert all(len(r[0]) > 501 for r in gc[:3]) and len(gc[3][0]) == 501 and all(u & 0xffffffff == 14 for u in gc[3][0])
    assert len({(u >> 32) for u in gc[3][0]}) >= 80
    e = by['edges']
    assert [len(r[0]) for r in e[:9]] == [0, 0, 0, 1, 1, 1, 1, 1, 1] and [len(r[0]) for r in e[9:]] == [2, 2, 0] and len(by['edges min_cnt 1'][11][0]) == 70

    fp = by['far peak'][0]
    assert fp[3]['far128'] >= 1 and fp[3]['peak_back'] == 1 and [(u >> 32, u & 0xffffffff) for u in fp[0]] == [(15 * 30, 30)]
    link = by['far peak'][1]
    assert link[3]['far128'] >= 1 and [(u >> 32, u & 0xffffffff) for u in link[0]] == [(15 * 36 - 9, 36)]   # (50 off: 7 + (5 >> 1))
    with_lone, without = by['strays']
    assert len(with_lone[0]) == 2 and len(without[0]) == 1                     # (the dropped anchors' seed lengths count)
    eg = by['exact gap']
    assert [u & 0xffffffff for u in eg[0][0]] == [4] and [u & 0xffffffff for u in eg[1][0]] == [270]


def test_every_counter_is_reached(refs):
    everything = [res for cases in refs.values() for case in cases for res in case]
    for key in COUNTERS:
        assert total(everything, key) >= 1, key
