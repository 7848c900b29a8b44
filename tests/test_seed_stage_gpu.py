"""GPU tests (-m gpu) of the seed half of the mapper (csrc/map_kernels.h: seed_lookup_kernel, seed_prefix_kernel, scan_i64x2_kernel,
seed_order_kernel, seed_filter_kernel, scan_i64_kernel, seed_read_off_kernel, seed_emit_kernel, anchor_msd_kernel,
anchor_window_sort_kernel, anchor_bitonic_list_kernel<1024>, <4096>, seg_sort_list_kernel<4>) through its stage entry point
mpn_seed_anchors_batch, which runs the function the mapper runs (seed_enqueue) on a made index and made minimizers.  Per read the
counts and the sorted anchor array itself are compared with the plain restatement of seed_ref.py: integers, no tolerances.
test_seed_ref.py pins that restatement to the oracle's collect_anchors and asserts that the families of seed_cases.py reach what they
are here for.  Every family runs with the mapper's launch values, with one block and with three per launch, with one workgroup of the
filter, and with the filter's second round on every read; cases that share their options also run as one batch."""
import numpy as np
import pytest

from seed_cases import FAMILIES, STD_KNOBS, families, merged, reference
from seed_ref import U64, list_counts, needed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib(libmpn):
    return libmpn


@pytest.fixture(scope='module')
def fams():
    return families()


@pytest.fixture(scope='module')
def refs(fams):
    """reference(case, knobs) by (case name, flt_round2): computed once per distinct second-round threshold and left unchanged"""
    memo = {}

    def get(family, c, knobs):
        key = (family, c.name, knobs.get('flt_round2', 0))
        if key not in memo:
            memo[key] = reference(c, knobs)
        return memo[key]
    return get


def run(c, knobs, cap=None):
    from megapath_nano_amd import mapper
    off = np.zeros(len(c.reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(mz) for mz, _ in c.reads])
    mz = np.concatenate([mz for mz, _ in c.reads]) if c.reads else np.zeros((0, 2), dtype=U64)
    x = c.index
    return mapper.seed_anchors_batch(x.k, x.lens, x.keys, x.key_off, x.pos, mapper.default_opt(**c.opt), off, mz, [q for _, q in c.reads], cap=cap, **knobs)


def rows(a):
    """(n, 2) words -> n records that compare as wholes"""
    return np.ascontiguousarray(a).view([('x', U64), ('y', U64)]).reshape(-1)


def check(where, c, want, got, counts):
    assert len(got) == len(want), where
    sizes = []
    for i, (w, g) in enumerate(zip(want, got)):
        at = where + ('read %d' % i,)
        assert (g['n_anchor'], g['rep_len'], g['span_sum']) == (w['n_anchor'], w['rep_len'], w['span_sum']), at + ('counts',)
        a, x, y = g['a'], g['a'][:, 0], g['a'][:, 1] & U64(0xffffffff)
        assert ((x[1:] > x[:-1]) | ((x[1:] == x[:-1]) & (y[1:] > y[:-1]))).all(), at + ('not strictly ascending in (x, low half of y)',)
        full = w['a']
        if len(a):                        # every anchor is, bit for bit, an anchor of collect
            v, f = rows(a), rows(full)
            assert np.isin(v, f).all(), at + ('%d anchors that collect does not give' % int((~np.isin(v, f)).sum()),)
        nd = needed(full, c.opt['max_gap'], c.opt['min_cnt'])
        exp = full[w['keep']]
        if not np.array_equal(a, exp):
            v, e, n = rows(a), rows(exp), rows(full[nd])
            assert False, at + ('%d anchors, %d expected; %d of them missing, %d beyond them; %d of the %d the compaction needs missing' % (
                len(a), len(exp), int((~np.isin(e, v)).sum()), int((~np.isin(v, e)).sum()), int((~np.isin(n, v)).sum()), len(n)),)
        assert (w['keep'] >= nd).all(), at
        if c.opt['min_cnt'] <= 1:
            assert len(a) == w['n_anchor'], at
        sizes += [int(s) for s in w['sizes']]
    assert counts['n_list'] == list_counts(sizes), where + ('work lists',)
    assert counts['walked'] == sum(sum(w['rounds']) for w in want), where + ('hits walked',)


def knob_id(k):
    return '-'.join('%s%d' % kv for kv in sorted(k.items())) or 'mapper'


@pytest.mark.parametrize('knobs', STD_KNOBS, ids=knob_id)
@pytest.mark.parametrize('family', FAMILIES)
def test_family_equals_ref(lib, fams, refs, family, knobs):
    for c in fams[family]:
        got, counts = run(c, knobs)
        check((family, c.name, knobs), c, refs(family, c, knobs), got, counts)


def test_cases_own_knobs(lib, fams, refs, family='rounds'):
    """a second-round threshold between two reads' hit counts, three persistent workgroups for 300 reads, the saturated read counted twice"""
    seen = 0
    for c in fams[family]:
        for knobs in c.knobs:
            got, counts = run(c, knobs)
            check((family, c.name, knobs), c, refs(family, c, knobs), got, counts)
            seen += 1
    assert seen >= 5


def test_reaches_every_work_list(lib, fams, refs):
    """which list a family fills is recorded here: the three size classes of the sort are all reached, and by the cases made for them"""
    seen = {}
    for c in fams['sort']:
        seen[c.name] = run(c, {})[1]['n_list']
    assert seen['sizes-small'] == (4, 0, 0) and seen['sizes-1024'] == (2, 1, 0) and seen['sizes-4096'] == (0, 2, 1) and seen['sizes-9000'] == (0, 0, 1)
    assert all(seen['straddle-17-at-%d' % at] == (1, 0, 0) and seen['straddle-16-at-%d' % at] == (0, 0, 0) for at in (1008, 1023, 1024))


@pytest.mark.parametrize('knobs', [{}, dict(grid_cap=1, flt_wgs=1)], ids=knob_id)
def test_all_reads_as_one_batch(lib, fams, knobs):
    """the reads of all cases with one option set in one batch over one index: a read's anchors do not depend on its neighbours or on the
    windows the batch is cut into"""
    groups = {}
    for name in FAMILIES:
        for c in fams[name]:
            if sum(len(mz) for mz, _ in c.reads) < 1500:             # (the saturated read is a batch of its own already)
                groups.setdefault(tuple(sorted(c.opt.items())), []).append(c)
    assert max(len(g) for g in groups.values()) > 15
    for key, g in groups.items():
        if len(g) < 2:
            continue
        m = merged(g)
        got, counts = run(m, knobs)
        check((key, knobs), m, reference(m, knobs), got, counts)


def test_fed_on_to_the_chaining_stage(lib, fams, refs):
    """the identical-chains claim of the filter: what it keeps, chained by mpn_chain_batch, gives the chains of the restatement of the
    chaining run on ALL the hits (every seed of these cases is 15 long, so the average seed length is the same over either set)"""
    from chain_ref import chain_ref, options
    from megapath_nano_amd import mapper
    n_chains = n_dropped = 0
    for family in ('walk', 'rounds'):
        for c in fams[family]:
            want = refs(family, c, {})
            pick = [i for i, w in enumerate(want) if 0 < w['n_anchor'] <= 1000]
            got, _ = run(c, {})
            opt = options(max_gap=c.opt['max_gap'], min_cnt=c.opt['min_cnt'], min_chain_score=20)
            off = np.concatenate([[0], np.cumsum([len(got[i]['a']) for i in pick])]).astype(np.int64)
            chains = mapper.chain_batch(mapper.default_opt(**opt), off, np.concatenate([got[i]['a'] for i in pick] + [np.zeros((0, 2), dtype=U64)]))
            for i, g in zip(pick, chains):
                assert (want[i]['a'][:, 1] >> U64(32) & U64(0xff) == U64(15)).all()
                u, b = chain_ref(opt, want[i]['a'])[:2]
                assert [int(v) for v in g['u']] == u and np.array_equal(g['b'], b), (family, c.name, i)
                n_chains += len(u)
                n_dropped += want[i]['n_anchor'] - len(got[i]['a'])
    assert n_chains >= 8 and n_dropped > 500


def test_equals_the_mappers_own_path(lib):
    """the mapper's own sketch and its exported index through the stage entry, then through the chaining entry, against what
    seed_chain_batch makes of the same reads: the entry runs what the mapper runs"""
    from map_cases import small_world
    from megapath_nano_amd import mapper
    gen, reads = small_world()
    gidx = mapper.Index(gen)
    try:
        seqs = [r['seq'] for r in reads]
        mzs = mapper.sketch_batch(seqs)
        keys, key_off, pos = gidx.export()
        off = np.concatenate([[0], np.cumsum([len(m) for m in mzs])]).astype(np.int64)
        for kw in ({}, dict(min_cnt=2, max_gap=300, max_chain_skip=3, bw=100)):
            want = mapper.seed_chain_batch(gidx, mapper.default_opt(**kw), seqs)
            got, _ = mapper.seed_anchors_batch(15, gidx.lens, keys, key_off, pos, mapper.default_opt(mid_occ=gidx.mid_occ(), **kw), off, np.concatenate(mzs),
                                               [len(s) for s in seqs])
            a_off = np.concatenate([[0], np.cumsum([len(g['a']) for g in got])]).astype(np.int64)
            chains = mapper.chain_batch(mapper.default_opt(**kw), a_off, np.concatenate([g['a'] for g in got]))
            assert sum(len(w['u']) for w in want) > len(reads) // 2
            for r, w, g, ch in zip(reads, want, got, chains):
                assert (g['n_anchor'], g['rep_len']) == (w['n_anchor'], w['rep_len']), (r['name'], kw)
                assert np.array_equal(ch['u'], w['u']) and np.array_equal(ch['b'], w['b']), (r['name'], kw)
    finally:
        gidx.close()


def test_empty_batch_and_a_capacity_too_small(lib, fams, refs):
    from megapath_nano_amd import _ffi, mapper
    c = fams['emit'][0]
    assert run(c._replace(reads=[]), {}) == ([], dict(n_list=(0, 0, 0), walked=0))
    want = refs('emit', c, {})
    total = sum(w['n_anchor'] for w in want)
    with pytest.raises(_ffi.MpnError, match='rc=-3') as e:
        run(c, {}, cap=total - 1)
    assert [int(v) for v in e.value.partial['n_anchor']] == [w['n_anchor'] for w in want]
    assert [int(v) for v in e.value.partial['anchor_off']] == [0] + [int(v) for v in np.cumsum([w['n_anchor'] for w in want])]
    got, counts = run(c, {}, cap=total)
    check(('exact capacity',), c, want, got, counts)
    assert mapper.last_stats()['anchors'] == total


def test_bad_input_is_refused_before_any_launch(lib, fams, refs):
    from megapath_nano_amd import _ffi, mapper
    c = fams['emit'][0]
    got, counts = run(c, {})
    check(('sound',), c, refs('emit', c, {}), got, counts)
    # the counters of the sound call stand for as long as nothing runs: a call that is refused leaves them as they are
    stats = mapper.last_stats()
    assert stats['anchors'] == sum(w['n_anchor'] for w in refs('emit', c, {})) and stats['minimizers'] == sum(len(mz) for mz, _ in c.reads)
    x = c.index
    off = np.zeros(len(c.reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(mz) for mz, _ in c.reads])
    mz = np.concatenate([mz for mz, _ in c.reads])
    qlen = np.array([q for _, q in c.reads], dtype=np.int32)
    base = dict(k=x.k, lens=x.lens, keys=x.keys, key_off=x.key_off, pos=x.pos, mz_off=off, mz=mz, seq_len=qlen)

    def refused(words, opt=None, knobs=None, **change):
        args = dict(base, **change)
        with pytest.raises(_ffi.MpnError, match='mpn_seed_anchors_batch: ' + words):   # (the validation's words, not a device error's)
            mapper.seed_anchors_batch(args['k'], args['lens'], args['keys'], args['key_off'], args['pos'], mapper.default_opt(**dict(c.opt, **(opt or {}))),
                                      args['mz_off'], args['mz'], args['seq_len'], **(knobs or {}))
        assert mapper.last_stats() == stats, words

    def edit(v, i, val):
        v = v.copy()
        v[i] = val
        return v
    refused('read 1: offsets out of order', mz_off=edit(off, 2, off[1] - 1))
    refused('offsets do not start at 0', mz_off=edit(off, 0, 1))
    refused('offsets do not start at 0', key_off=edit(x.key_off, 0, 1))
    refused('read 3: offsets out of order', key_off=edit(x.key_off, 4, x.key_off[3] - 1))
    refused('index: key 5: not ascending', keys=edit(x.keys, 5, x.keys[4]))
    refused('index: key %d: not ascending, or outside 2k bits' % (len(x.keys) - 1), keys=edit(x.keys, -1, 1 << 30))
    refused('index: position 2: outside its target', pos=edit(x.pos, 2, len(x.lens) << 32))
    refused('index: position 0: outside its target', pos=edit(x.pos, 0, int(x.pos[0]) >> 32 << 32 | 30000 << 1))
    refused('index: k outside 1 .. 28', k=0)
    refused('index: k outside 1 .. 28', k=29)
    refused('index: target 1: negative length', lens=edit(x.lens, 1, -1))
    m1 = int(off[1])                                       # the first minimizer of read 1
    refused('read 1: minimizer 0: hash outside 2k bits', mz=edit(mz, (m1, 0), (1 << 30) << 8 | 15))
    refused('read 1: minimizer 0: span outside', mz=edit(mz, (m1, 0), int(mz[m1, 0]) >> 8 << 8))
    refused('read 0: minimizer 0: span outside', mz=edit(mz, (0, 0), int(mz[0, 0]) >> 8 << 8 | 16))          # last_pos 14: 15 at most
    refused('read 0: minimizer 3: last_pos outside the read', seq_len=edit(qlen, 0, 999))
    refused('read 1: minimizer 3: last_pos decreases', mz=edit(mz, (m1 + 3, 1), int(mz[m1 + 2, 1]) - 2))
    refused('read 2: negative length', seq_len=edit(qlen, 2, -1))
    for bad in (0, -1, (1 << 25) + 1):
        refused('mid_occ %d outside 1 .. 2\\^25' % bad, opt=dict(mid_occ=bad))
    refused('a negative option', opt=dict(min_cnt=-1))
    refused('a negative option', opt=dict(max_gap=-1))
    refused('max_gap 66076419 is beyond 66076418', opt=dict(max_gap=66076419))
    for knob in ('flt_round2', 'flt_wgs', 'grid_cap', 'cap'):
        refused('flt_round2, flt_wgs, grid_cap or the capacity negative', knobs={knob: -1})
    got, counts = mapper.seed_anchors_batch(x.k, x.lens, x.keys, x.key_off, x.pos, mapper.default_opt(**dict(c.opt, mid_occ=1 << 25, max_gap=66076418)), off, mz, qlen)
    check(('the largest cut-off and gap',), c, reference(c._replace(opt=dict(c.opt, mid_occ=1 << 25, max_gap=66076418))), got, counts)
