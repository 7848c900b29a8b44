"""CPU tests of the restatement the seed-stage tests compare the kernels with (seed_ref.py) and of the cases they run (seed_cases.py):
collect against the oracle's collect_anchors on a small world, fed with the oracle's own sketch and index table; the NumPy forms
against the loops; the filter's superset chain sketch_rule >= bin_rule >= needed on every read of every family and on seeded random
position sets; and every case reaching what it is named for, so that a case that stops reaching its path fails here, without a GPU."""
import ctypes as ct

import numpy as np
import pytest

from seed_cases import FAMILIES, STD_KNOBS, families, reference, stepped
from seed_ref import MadeIndex, U64, bin_rule, collect, collect_np, needed, sketch_rule, sort_anchors


@pytest.fixture(scope='module')
def fams():
    return families()


def test_collect_equals_the_oracle(oracle_built):
    from map_cases import small_world
    from oracle import mm2_bindings as mb
    gen, reads = small_world()
    oidx = mb.Index(gen)
    L = mb.lib()
    L.mmo_idx_get.argtypes = [ct.c_void_p, ct.c_uint64, ct.POINTER(ct.POINTER(ct.c_uint64))]
    L.mmo_idx_get.restype = ct.c_int64
    try:
        n_hits = 0
        for r in reads:
            mv = mb.sketch(r['seq'], 10, 15, 0)
            table = {}
            for h in {int(x) >> 8 for x in mv[:, 0]}:
                p = ct.POINTER(ct.c_uint64)()
                t = L.mmo_idx_get(oidx.h, h, ct.byref(p))
                if t:
                    table[h] = [int(p[j]) for j in range(t)]
            index = MadeIndex(15, oidx.lens, table)
            for mid_occ in (oidx.mid_occ(), 3):
                want, rep = mb.collect_anchors(oidx, mid_occ, mv, len(r['seq']))
                for fn in (collect, collect_np):
                    a, n_a, rl, ss = fn(index, mv, len(r['seq']), mid_occ)
                    assert n_a == len(want) and rl == rep and np.array_equal(a, want), (r['name'], mid_occ, fn.__name__)
                    assert ss == int((want[:, 1] >> U64(32) & U64(0xff)).sum())
                n_hits += len(want)
        assert n_hits > 5000
    finally:
        oidx.close()


def test_numpy_forms_equal_the_loops(fams):
    seen = 0
    for name in FAMILIES:
        for c in fams[name]:
            for mz, qlen in c.reads:
                got = collect_np(c.index, mz, qlen, c.opt['mid_occ'])
                if got[1] > 20000:
                    continue
                want = collect(c.index, mz, qlen, c.opt['mid_occ'])
                assert got[1:] == want[1:] and np.array_equal(got[0], want[0]), (name, c.name)
                seen += got[1]
    assert seen > 50000


def supersets(where, a, max_gap, min_cnt, knobs=({}, dict(flt_round2=1))):
    nd, br = needed(a, max_gap, min_cnt), bin_rule(a, max_gap, min_cnt)
    assert (br >= nd).all(), where + ('bin_rule misses %d needed hits' % int((nd & ~br).sum()),)
    for kn in knobs:
        sk = sketch_rule(a, max_gap, min_cnt, kn.get('flt_round2', 0))
        assert (sk >= br).all(), where + (kn, 'sketch_rule misses %d hits of bin_rule' % int((br & ~sk).sum()))
    return int(nd.sum()), int(br.sum())


@pytest.mark.parametrize('family', FAMILIES)
def test_filter_keeps_a_superset_on_every_case(fams, family):
    for c in fams[family]:
        for kn in STD_KNOBS[:1] + tuple(c.knobs) + (dict(flt_round2=1),):
            for i, r in enumerate(reference(c, kn)):
                nd, br = needed(r['a'], c.opt['max_gap'], c.opt['min_cnt']), bin_rule(r['a'], c.opt['max_gap'], c.opt['min_cnt'])
                assert (br >= nd).all() and (r['keep'] >= br).all(), (family, c.name, kn, i)
                if c.opt['min_cnt'] <= 1:
                    assert r['keep'].all()


def test_filter_keeps_a_superset_on_random_position_sets():
    rng = np.random.default_rng(7)
    n_hits = n_needed = n_dropped = 0
    for it in range(600):
        min_cnt, max_gap = int(rng.integers(1, 7)), int(rng.choice([1, 2, 7, 100, 300, 5000, 40000]))
        words = []
        for rid in range(int(rng.integers(1, 4))):
            for strand in (0, 1):
                n = int(rng.integers(0, 60))
                words += [strand << 63 | rid << 32 | p for p in stepped(rng, n, int(rng.integers(0, 1 << 20)), max_gap, 1 << 30)]
        a = sort_anchors(np.array([(x, 15 << 32 | j) for j, x in enumerate(words)], dtype=U64).reshape(-1, 2))
        nd, br = supersets((it, min_cnt, max_gap), a, max_gap, min_cnt)
        n_hits, n_needed, n_dropped = n_hits + len(a), n_needed + nd, n_dropped + len(a) - br
    assert n_hits > 50000 and n_needed > 10000 and n_dropped > 1000


@pytest.mark.parametrize('family', FAMILIES)
def test_cases_reach_what_they_are_named_for(fams, family):
    assert fams[family]
    for c in fams[family]:
        assert c.opt['min_cnt'] == 1 or family in ('walk', 'rounds'), c.name
        x = c.index                                       # what the entry's validation asks of an index and of minimizers
        rid, p = (x.pos >> U64(32)).astype(np.int64), ((x.pos & U64(0xffffffff)) >> U64(1)).astype(np.int64)
        assert (np.diff(x.keys.astype(np.int64)) > 0).all() and (x.keys < U64(1 << 2 * x.k)).all() and (rid < len(x.lens)).all(), c.name
        assert (p < np.asarray(x.lens, dtype=np.int64)[rid]).all(), c.name
        for mz, qlen in c.reads:
            span, last = (mz[:, 0] & U64(0xff)).astype(np.int64), ((mz[:, 1] & U64(0xffffffff)) >> U64(1)).astype(np.int64)
            assert (span >= 1).all() and (span <= last + 1).all() and (last < qlen).all() and (np.diff(last) >= 0).all(), c.name
            assert (mz[:, 0] >> U64(8) < U64(1 << 2 * x.k)).all(), c.name
        c.reach(c, reference(c))
