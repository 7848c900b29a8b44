"""GPU tests (-m gpu) of the chaining stage (csrc/map_kernels.h: anchor_compact_kernel, chain_segments_kernel, chain_dp_kernel,
chain_ends_kernel, chain_sort_ends_kernel, chain_backtrack_kernel) through its stage entry point mpn_chain_batch, which runs the
function the mapper runs (chain_enqueue).  Per read the chain counts, the (score, count) words, the chained anchors and all six
fields of every chain record are compared with the sequential restatement of chain_ref.py: integers, no tolerances.
test_chain_ref.py pins that restatement to the oracle's mmo_chain on the same cases and asserts that the families of chain_cases.py
reach what they are here for.  Every family runs with the mapper's launch values, with the backtrack forced to either path, with
the smallest and the largest work items, with one block and with three per launch; batches that share their options also run as
one batch."""
import numpy as np
import pytest

from chain_cases import FAMILIES, Case, families, read, run
from chain_ref import OPT_KEYS, chain_ref, options

pytestmark = pytest.mark.gpu

NEVER = 1 << 30          # more chain ends than a read can have: the backtrack of every read is the sequential one
# (chain_item, bt_par_min, grid_cap): every value of each knob, and one block with a lane per chain end
CONFIGS = [(0, 0, 0), (0, 1, 0), (0, NEVER, 0), (16, 0, 0), (4096, 0, 0), (0, 0, 1), (0, 0, 3), (0, 1, 1)]


@pytest.fixture(scope='module')
def lib(libmpn):
    return libmpn


@pytest.fixture(scope='module')
def fams():
    return families()


@pytest.fixture(scope='module')
def refs(fams):
    """chain_ref of every read of every case, computed once and left unchanged"""
    return {name: [[chain_ref(c.opt, r)[:3] for r in c.reads] for c in cases] for name, cases in fams.items()}


def chain(opt, reads, config=(0, 0, 0)):
    from megapath_nano_amd import mapper
    off, a = Case('', reads).arrays()
    return mapper.chain_batch(mapper.default_opt(**opt), off, a, chain_item=config[0], bt_par_min=config[1], grid_cap=config[2])


def check(where, want, got):
    """want: (u, b, recs) of chain_ref per read; got: what mapper.chain_batch returned"""
    assert len(got) == len(want), where
    for i, ((u, b, recs), g) in enumerate(zip(want, got)):
        at = where + ('read %d' % i,)
        assert g['n_chain'] == len(u) and g['n_chained'] == len(b), at + ('counts', g['n_chain'], len(u), g['n_chained'], len(b))
        assert [int(v) for v in g['u']] == u, at + ('u', [(int(v) >> 32, int(v) & 0xffffffff) for v in g['u'][:8]], [(v >> 32, v & 0xffffffff) for v in u[:8]])
        assert np.array_equal(g['b'], b), at + ('b',)
        got_recs = [tuple(int(v) for v in r[:4].view(np.uint64)) + (int(r[4]), int(r[5])) for r in g['recs']]
        assert got_recs == recs, at + ('records', [k for k, (x, y) in enumerate(zip(got_recs, recs)) if x != y][:8])


@pytest.mark.parametrize('config', CONFIGS, ids=lambda c: 'item%d-par%d-grid%d' % (c[0], min(c[1], 99), c[2]))
@pytest.mark.parametrize('family', FAMILIES)
def test_family_equals_ref(lib, fams, refs, family, config):
    for c, want in zip(fams[family], refs[family]):
        check((family, c.name, config), want, chain(c.opt, c.reads, config))


@pytest.mark.parametrize('config', [(0, 0, 0), (0, 1, 1)], ids=['mapper', 'par1-grid1'])
def test_batches_that_share_options_as_one(lib, fams, refs, config):
    """the reads of all cases with one option set in one batch (cut after 16000 anchors): a read's chains do not depend on its
    neighbours, its place in the batch or the pieces the compaction cuts the batch into"""
    groups = {}
    for name in FAMILIES:
        for c, want in zip(fams[name], refs[name]):
            g = groups.setdefault(tuple(c.opt[k] for k in OPT_KEYS), [])
            g.extend(zip(c.reads, want))
    assert max(len(g) for g in groups.values()) > 30
    for key, g in groups.items():
        lo = 0
        while lo < len(g):
            hi, n = lo, 0
            while hi < len(g) and (hi == lo or n + len(g[hi][0]) <= 16000):
                n += len(g[hi][0])
                hi += 1
            check((key, lo, hi, config), [w for _, w in g[lo:hi]], chain(dict(zip(OPT_KEYS, key)), [r for r, _ in g[lo:hi]], config))
            lo = hi


def test_empty_batch(lib):
    assert chain(options(), []) == []
    check(('no anchors',), [([], np.zeros((0, 2), np.uint64), [])] * 3, chain(options(), [read([])] * 3))


def test_bad_input_is_refused_before_any_launch(lib):
    from megapath_nano_amd import _ffi, mapper
    reads = [read(run(1000, 100, 12)), read(run(5000, 100, 9))]
    off, a = Case('', reads).arrays()
    want = [chain_ref(options(), r)[:3] for r in reads]
    check(('sound',), want, mapper.chain_batch(mapper.default_opt(), off, a))

    # the counters of the sound call (anchors kept for chaining, batches run) stand for as long as nothing runs: a call that is
    # refused leaves them as they are, one that reaches its first launch has cleared them
    stats = mapper.last_stats()
    assert stats['anchors_kept'] == 21 and stats['sub_batches'] == 1

    def refused(words, opt=None, off=off, a=a, **knobs):
        with pytest.raises(_ffi.MpnError, match='mpn_chain_batch: ' + words):       # (the validation's words, not a device error's)
            mapper.chain_batch(mapper.default_opt(**(opt or {})), off, a, **knobs)
        assert mapper.last_stats() == stats, words

    swapped = a.copy()
    swapped[[14, 15]] = swapped[[15, 14]]
    refused('read 1: anchor 3: x decreases', a=swapped)
    refused('read 1: offsets out of order', off=np.array([0, 14, 12], dtype=np.int64))
    refused('offsets do not start at 0', off=np.array([1, 12, 21], dtype=np.int64))
    for q in (1 << 31, (1 << 32) - 1):
        bad = a.copy()
        bad[5, 1] = int(bad[5, 1]) >> 32 << 32 | q
        refused('read 0: anchor 5: query position', a=bad)
    for key in OPT_KEYS:
        refused('a negative option', opt={key: -1})
    refused('max_chain_iter below 1', opt=dict(max_chain_iter=0))
    # the 32-bit running coordinate of the chain DP's ring: 65 max_gap + 64 must stay below 2^32
    refused('max_gap 66076419 is beyond 66076418', opt=dict(max_gap=66076419))
    refused('max_gap 2147483647 is beyond', opt=dict(max_gap=(1 << 31) - 1))
    for knob in ('chain_item', 'bt_par_min', 'grid_cap'):
        refused('chain_item, bt_par_min, grid_cap', **{knob: -1})
    far = [read(run(1000, 100, 5) + run(1000 + 66076418 + 80, 100 + 200, 5))]
    check(('the largest max_gap',), [chain_ref(options(max_gap=66076418), far[0])[:3]], chain(options(max_gap=66076418), far))
    assert mapper.last_stats()['anchors_kept'] == 10          # (what the family widest-gap measures inside the ring is accepted)


def test_equals_the_mappers_own_path(lib, oracle_built):
    """the anchors the oracle collects for the reads of a small world, chained through the stage entry, against what
    seed_chain_batch makes of the same reads: the entry runs what the mapper runs"""
    from map_cases import small_world
    from megapath_nano_amd import _ffi, mapper
    from oracle import mm2_bindings as mb
    gen, reads = small_world()
    gidx, oidx = mapper.Index(gen), mb.Index(gen)
    try:
        anchors = [mb.collect_anchors(oidx, oidx.mid_occ(), mb.sketch(r['seq'], 10, 15, 0), len(r['seq']))[0] for r in reads]
        for kw in ({}, dict(min_cnt=2, max_gap=300, max_chain_skip=3, bw=100)):
            got = mapper.seed_chain_batch(gidx, mapper.default_opt(**kw), [r['seq'] for r in reads])
            mine = chain(options(**kw), anchors)
            assert sum(g['n_chain'] for g in mine) > len(reads) // 2
            for r, g, m, a in zip(reads, got, mine, anchors):
                assert g['n_anchor'] == len(a), r['name']
                assert np.array_equal(g['u'], m['u']) and np.array_equal(g['b'], m['b']), (r['name'], kw)
        with pytest.raises(_ffi.MpnError, match='max_gap 66076419 is beyond 66076418'):
            mapper.seed_chain_batch(gidx, mapper.default_opt(max_gap=66076419), [reads[0]['seq']])
        stats = mapper.last_stats()                            # (cleared on entry: nothing was sketched, nothing chained)
        assert stats['bases'] == len(reads[0]['seq']) and stats['minimizers'] == 0 and stats['anchors_kept'] == 0 and stats['sub_batches'] == 0
    finally:
        gidx.close()
        oidx.close()
