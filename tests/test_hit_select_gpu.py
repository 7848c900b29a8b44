"""GPU tests (-m gpu) of the hit stage (csrc/hit_kernels.h: mm_gen_regs, mm_set_parent, mm_select_sub, mm_squeeze_a, mm_join_long,
one wave per read; gen_regs .. join_long of csrc/hit_host.cpp for the reads left to the host; anchor_squeeze_kernel) through its stage
entry point mpn_hit_select_batch, which runs the function the mapper runs.  Every per-read and per-hit output and every squeezed
anchor is compared with the sequential restatement of hit_ref.py, exact integers; test_hit_ref.py pins that restatement to the
oracle's own functions on the same cases and asserts that the families of hit_cases.py reach the mechanisms these tests are here
for.  Each batch runs through the mapper's dispatch (path 0), the large instantiation alone (1) and the host functions (2), and
through the kernels again with a single block, which then takes every read in turn on the same LDS arrays."""
import numpy as np
import pytest

from hit_cases import Batch, Chain, Read, families
from hit_ref import KEYS, hit_ref

pytestmark = pytest.mark.gpu
PATHS = (0, 1, 2)


@pytest.fixture(scope='module')
def lib(libmpn):
    return libmpn


@pytest.fixture(scope='module')
def fams():
    return families()


@pytest.fixture(scope='module')
def refs(fams):
    """hit_ref of every read of every batch, computed once and left unchanged"""
    return {name: [ref_of(b) for b in batches] for name, batches in fams.items()}


def ref_of(b):
    return [hit_ref(b.k, r.name, r.qlen, *r.u_a(), **b.opt) for r in b.reads]


def run(b, arrays, path, max_chains=0, grid_cap=0, with_cigar=1):
    from megapath_nano_amd import mapper
    opt = mapper.default_opt(with_cigar=with_cigar, **b.opt)
    return mapper.hit_select_batch(opt, b.k, arrays['q_len'], arrays['names'], arrays['chain_off'], arrays['u'], arrays['recs'], arrays['anchor_off'],
                                   arrays['anchors'], path=path, max_chains=max_chains, grid_cap=grid_cap)


def check(b, want, arrays, path, max_chains=0, grid_cap=0, with_cigar=1):
    what = (b.name, 'path %d' % path, 'max_chains %d' % max_chains, 'grid_cap %d' % grid_cap, 'with_cigar %d' % with_cigar)
    n_regs, n_a, hits, sq = run(b, arrays, path, max_chains, grid_cap, with_cigar)
    assert len(n_regs) == len(b.reads) == len(want)
    assert [int(v) for v in n_regs] == [len(h) for h, _, _ in want], what
    assert [int(v) for v in n_a] == [len(s) for _, s, _ in want], what
    hits_u = hits.view(np.uint64)
    pos = 0
    for r, (whits, _, _) in zip(b.reads, want):
        for i, w in enumerate(whits):
            for j, key in enumerate(KEYS):
                got = int(hits_u[pos, j]) if key in ('fx', 'fy', 'lx', 'ly', 'hash') else int(hits[pos, j])
                assert got == w[key], what + (r.name, len(r.sorted), 'hit %d' % i, key, got, w[key])
            pos += 1
    if not with_cigar:
        assert sq is None
        return
    wsq = np.array([p for _, s, _ in want for p in s], dtype=np.uint64).reshape(-1, 2)
    if not np.array_equal(sq, wsq):
        off = np.concatenate([[0], np.cumsum(n_a)])
        bad = int(np.nonzero((sq != wsq).any(axis=1))[0][0])
        ri = int(np.searchsorted(off, bad, side='right')) - 1
        assert False, what + (b.reads[ri].name, 'squeezed anchor %d' % (bad - off[ri]), [hex(int(v)) for v in sq[bad]], [hex(int(v)) for v in wsq[bad]])


def check_batch(b, want):
    arrays = b.arrays()
    for mc in b.max_chains:
        for path in PATHS:
            check(b, want, arrays, path, mc)
    for path in (0, 1):          # one block: every read on the LDS arrays the read before it has left
        check(b, want, arrays, path, b.max_chains[-1], grid_cap=1)
    check(b, want, arrays, 1, 0, grid_cap=2)
    for path in PATHS:           # hits only
        check(b, want, arrays, path, b.max_chains[-1], with_cigar=0)


@pytest.mark.parametrize('family', ['counts', 'ties', 'mask', 'select', 'join', 'hand'])
def test_family_equals_ref(lib, fams, refs, family):
    for b, want in zip(fams[family], refs[family]):
        check_batch(b, want)


def test_real_chains_equal_ref(lib):
    """the chains of a small world as the chain stage leaves them: the record layout of the synthetic families is the product's"""
    from map_cases import small_world
    from megapath_nano_amd import mapper
    gen, reads = small_world()
    idx = mapper.Index(gen)
    try:
        opt = mapper.default_opt()
        got = mapper.seed_chain_batch(idx, opt, [r['seq'] for r in reads])
    finally:
        idx.close()
    rng = np.random.default_rng(5)
    rs = []
    for r, g in zip(reads, got):
        chains, pos = [], 0
        for u in g['u']:
            cnt = int(u) & 0xffffffff
            chains.append(Chain(g['b'][pos:pos + cnt], int(u) >> 32))
            pos += cnt
        assert pos == len(g['b'])
        if len({c.a[0][0] for c in chains}) == len(chains):
            rs.append(Read(r['name'], len(r['seq']), chains, rng))
    assert len(rs) >= len(reads) - 2 and sum(len(r.sorted) for r in rs) > len(rs) and max(len(r.sorted) for r in rs) >= 3
    for opts in ({}, dict(best_n=50, pri_ratio=0.1)):
        b = Batch('real', rs, max_chains=(0, 2), k=15, **opts)
        want = ref_of(b)
        assert sum(len(h) for h, _, _ in want) >= len(rs) // 2
        check_batch(b, want)


def test_bad_input_is_refused_before_any_launch(lib, fams):
    from megapath_nano_amd import _ffi
    b = fams['hand'][0]

    def broken(change):
        arrays = b.arrays()
        arrays['u'], arrays['anchors'] = arrays['u'].copy(), arrays['anchors'].copy()
        arrays['recs'] = tuple(a.copy() for a in arrays['recs'])
        change(arrays)
        with pytest.raises(_ffi.MpnError):
            run(b, arrays, 0)

    def zero_cnt(a):
        a['u'][0] &= np.uint64(0xffffffff00000000)

    def one_more(a):
        a['u'][0] += np.uint64(1)

    def wrong_first(a):
        a['recs'][0][1] += np.uint64(1)

    def wrong_last(a):
        a['recs'][3][2] += np.uint64(1)

    def same_first(a):
        c0 = int(a['u'][0]) & 0xffffffff      # the first anchor of the second chain of the pool
        a['anchors'][c0, 0] = a['anchors'][0, 0]
        a['recs'][0][1] = a['recs'][0][0]

    def no_length(a):
        a['q_len'] = np.zeros_like(a['q_len'])

    for change in (zero_cnt, one_more, wrong_first, wrong_last, same_first, no_length):
        broken(change)
