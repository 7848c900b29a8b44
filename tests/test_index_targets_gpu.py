"""GPU parity (-m gpu) of the TARGET side of the mapper on the worlds of target_cases.py, bit for bit: the 2-bit packing and its
list of ambiguous-base runs (idx_pack2_kernel), the readers of packed targets (ref_code / RefCursor behind every DP, finish and tag
kernel and idx_decode_kernel), the index sort / emit kernels and the three paths of mpn_index_mid_occ, on N runs on and around
the 16-base words, IUPAC codes, lower case, zero-length and sub-k targets, heavy repeats and thousands of tiny targets.

The oracle (oracle/mm2_oracle.c) keeps targets as one code per base and sketches each target on the CPU, so every comparison is
an equality.  What the worlds contain is asserted on the oracle alone in test_target_cases.py."""
import ctypes as ct
from types import SimpleNamespace

import numpy as np
import pytest

import target_cases as tc
from diff_tags_ref import CS, EQX, MD, codes
from test_dispatch_paths_gpu import World as ChildWorld, assert_paf_matches, run_child
from test_map_tags_gpu import check_paf, check_sam, strip_tags

pytestmark = pytest.mark.gpu

FRACS = (2e-4, 0.01, 0.03, 0.05, 0.1, 0.5)
KW = ((15, 10), (19, 5), (15, 15))
NP = dict(best_n=50, pri_ratio=1.0)


class W:
    def __init__(self, gen, reads, facts):
        from megapath_nano_amd import mapper
        from oracle import mm2_bindings as mb
        self.gen, self.reads, self.facts = gen, reads, facts
        self.names, self.seqs = [r['name'] for r in reads], [r['seq'] for r in reads]
        self.gidx, self.oidx = mapper.Index(gen), mb.Index(gen)
        self._paf = {}

    def oracle_paf(self, **kw):
        from oracle import mm2_bindings as mb
        key = tuple(sorted(kw.items()))
        if key not in self._paf:
            opt = mb.default_opt(**kw)
            self._paf[key] = [mb.map_read(self.oidx, opt, n, s)[2] for n, s in zip(self.names, self.seqs)]
        return self._paf[key]

    def close(self):
        self.gidx.close()
        self.oidx.close()


@pytest.fixture(scope='module')
def worlds(libmpn, oracle_built):
    out = {'dirty': W(*tc.dirty_world('mult16')), 'dirty_plus1': W(*tc.dirty_world('plus1')), 'repeat': W(*tc.repeat_world()),
           'many': W(*tc.many_targets_world())}
    yield out
    for w in out.values():
        w.close()


def expected_index(gen, k, w):
    """keys, key_off, pos from the oracle's per-target sketches, ordered by (hash, position word)"""
    from oracle import mm2_bindings as mb
    mz = np.concatenate([mb.sketch(s, w, k, rid) for rid, (_, s) in enumerate(gen)] + [np.zeros((0, 2), dtype=np.uint64)])
    key, y = mz[:, 0] >> np.uint64(8), mz[:, 1]
    order = np.lexsort((y, key))
    key, y = key[order], y[order]
    first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if len(key) else np.zeros(0, dtype=np.int64)
    return key[first], np.concatenate([first, [len(key)]]).astype(np.int64), y


def idx_get(oidx, key):
    from oracle import mm2_bindings as mb
    L = mb.lib()
    L.mmo_idx_get.argtypes = [ct.c_void_p, ct.c_uint64, ct.POINTER(ct.POINTER(ct.c_uint64))]
    L.mmo_idx_get.restype = ct.c_int64
    p = ct.POINTER(ct.c_uint64)()
    n = L.mmo_idx_get(oidx.h, int(key), ct.byref(p))
    return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, dtype=np.uint64)


def assert_index_equals(gidx, gen, k, w, oidx=None, sample=None):
    keys, key_off, pos = gidx.export()
    wk, wo, wp = expected_index(gen, k, w)
    assert (gidx.n_minimizers, gidx.n_keys) == (len(wp), len(wk))
    for name, a, b in (('keys', keys, wk), ('key_off', key_off, wo), ('pos', pos, wp)):
        if not np.array_equal(a, b):
            i = int(np.flatnonzero(a != b)[0]) if a.shape == b.shape else -1
            raise AssertionError((name, 'first difference at', i, a[i:i + 3], b[i:i + 3], a.shape, b.shape))
    if oidx is not None:
        which = range(len(keys)) if sample is None else np.random.default_rng(0).integers(0, len(keys), size=sample)
        for i in which:
            assert np.array_equal(idx_get(oidx, keys[i]), pos[key_off[i]:key_off[i + 1]]), (i, int(keys[i]))
    return keys, key_off, pos


# ---------------------------------------------------------------------------------------------------------------- the index

@pytest.mark.parametrize('k,w', KW)
@pytest.mark.parametrize('name', ['dirty', 'dirty_plus1', 'repeat', 'many'])
def test_whole_index_equals_oracle_sketches(worlds, name, k, w):
    from megapath_nano_amd import mapper
    from oracle import mm2_bindings as mb
    wd = worlds[name]
    own = (k, w) != (tc.K, tc.W)
    gidx, oidx = (mapper.Index(wd.gen, k=k, w=w), mb.Index(wd.gen, k=k, w=w)) if own else (wd.gidx, wd.oidx)
    try:
        keys, key_off, pos = assert_index_equals(gidx, wd.gen, k, w, oidx, sample=400 if name == 'many' else None)
        occ = np.diff(key_off)
        if name == 'repeat':   # one key whose positions fill a sort bucket and span many 2048-record emit blocks
            assert occ.max() > 60000 and np.sort(occ)[-2] > 30000
            if not own:
                assert (len(pos), len(keys)) == (wd.facts['n_minimizers'], wd.facts['n_keys'])
        if name == 'many':     # the target id takes 13 bits of the position word
            assert int(pos.max() >> np.uint64(32)) > 4900
    finally:
        if own:
            gidx.close()
            oidx.close()


@pytest.mark.parametrize('name', ['dirty', 'dirty_plus1', 'repeat', 'many'])
def test_mid_occ_equals_oracle(worlds, name):
    wd = worlds[name]
    got = [wd.gidx.mid_occ(f) for f in FRACS]
    assert got == [wd.oidx.mid_occ(f) for f in FRACS]
    if name == 'repeat':   # the three paths: LDS bins, global-atomic bins, the open bin with the selection on the host
        assert got[0] > 65535 and 1024 < got[3] <= 65535 and got[4] <= 1024, got
        assert {f: wd.gidx.mid_occ(f) for f in wd.facts['mid_occ']} == wd.facts['mid_occ']


def test_mid_occ_at_the_bin_edges(libmpn, oracle_built):
    """every key of a set with occurrence counts 1023, 1024, 1025, 65 534, 65 535 and 65 536 is selected by some fraction"""
    from megapath_nano_amd import mapper
    from oracle import mm2_bindings as mb
    gen, _, facts = tc.occ_edge_world()
    gidx, oidx = mapper.Index(gen), mb.Index(gen)
    try:
        _, key_off, _ = assert_index_equals(gidx, gen, tc.K, tc.W)
        occ = np.sort(np.diff(key_off))
        assert set(facts['counts']) <= set(occ.tolist())
        n = len(occ)
        fracs = [1.0 - (i + 0.5) / n for i in range(n)]
        got = [gidx.mid_occ(f) for f in fracs]
        assert got == [oidx.mid_occ(f) for f in fracs]
        assert got == [int(x) + 1 for x in occ], (got, occ)   # (the fractions do select every key)
    finally:
        gidx.close()
        oidx.close()


# ------------------------------------------------------------------------------------------------- targets as they went in

def boundaries(gen, facts, targets):
    """(target, position) of every run start, run end and target end of `targets`"""
    out = []
    for t in targets:
        out += [(t, p) for run in facts['runs'][t] for p in run] + [(t, len(gen[t][1]))]
    return sorted(set(out))


@pytest.mark.parametrize('name', ['dirty', 'dirty_plus1'])
def test_fetch_seq_round_trips_dirty_targets(worlds, name):
    from megapath_nano_amd import _ffi
    wd = worlds[name]
    want = [tc.decoded(s) for _, s in wd.gen]
    assert any(b'N' * 1500 in x for x in want) and any(x and x == b'N' * len(x) for x in want) and want[0] == b''
    for t, x in enumerate(want):
        assert wd.gidx.fetch_seq(t, 0, len(x)) == x, wd.gen[t][0]
    n = 0
    for t, p in boundaries(wd.gen, wd.facts, range(len(want))):
        x = want[t]
        for s in range(max(0, p - 16), min(p, len(x)) + 1):
            for e in range(max(p, s), min(len(x), p + 16) + 1):
                assert wd.gidx.fetch_seq(t, s, e - s) == x[s:e], (wd.gen[t][0], p, s, e)
                n += 1
    assert n > 5000   # (17 x 17 ranges around a boundary that is not near an end of its target)
    big = wd.facts['big']
    for args in ((big, len(want[big]) - 1, 2), (big, -1, 2), (big, 0, -1), (len(want), 0, 1), (-1, 0, 1), (0, 0, 1), (0, 1, 0)):
        with pytest.raises(_ffi.MpnError):
            wd.gidx.fetch_seq(*args)
    assert wd.gidx.fetch_seq(0, 0, 0) == b'' and wd.gidx.fetch_seq(big, len(want[big]), 0) == b''


def test_fetch_seq_round_trips_many_targets(worlds):
    wd = worlds['many']
    for t, (_, s) in enumerate(wd.gen):
        assert wd.gidx.fetch_seq(t, 0, len(s)) == tc.decoded(s), t
    for t in wd.facts['tiny'] + wd.facts['family'][:5]:   # every sub-range of the 1..14-base targets, the ends of some others
        x = tc.decoded(wd.gen[t][1])
        for s in range(max(0, len(x) - 16), len(x) + 1):
            for e in range(s, len(x) + 1):
                assert wd.gidx.fetch_seq(t, s, e - s) == x[s:e], (t, s, e)


def test_more_runs_than_the_first_list_capacity(libmpn, oracle_built):
    from megapath_nano_amd import mapper
    from oracle import mm2_bindings as mb
    gen, reads, facts = tc.striped_world()
    assert len(tc.n_runs_of(gen[0][1])) == facts['n_runs'] > facts['first_cap']
    gidx, oidx = mapper.Index(gen), mb.Index(gen)
    try:
        for t, (_, s) in enumerate(gen):
            assert gidx.fetch_seq(t, 0, len(s)) == tc.decoded(s), t
        x = tc.decoded(gen[0][1])
        for s, e in ((0, 4), (3, 1), (2, 3), (299996, 4), (299999, 1), (131071, 40), (262140, 9)):
            assert gidx.fetch_seq(0, s, e) == x[s:s + e]
        _, _, pos = assert_index_equals(gidx, gen, tc.K, tc.W, oidx)
        assert len(pos) > 1000 and np.all(pos >> np.uint64(32) == 1)   # the striped target has no k-mer without an N
        names, seqs = [r['name'] for r in reads], [r['seq'] for r in reads]
        got = mapper.map_batch(gidx, mapper.default_opt(**NP), names, seqs)
        want = [mb.map_read(oidx, mb.default_opt(**NP), n, s)[2] for n, s in zip(names, seqs)]
        assert all(want)
        assert_paf_matches(got, want, reads, 'striped')
    finally:
        gidx.close()
        oidx.close()


# --------------------------------------------------------------------------------------------------------------- PAF parity

def assert_runs_inside_hits(paf, facts, gen):
    """the GPU's own lines: hits that contain the runs of 17, 60 and 300, and a hit that stops at the head or tail run"""
    lines = [l.split('\t') for l in paf.splitlines()]
    for key in ('17', '60', '300'):
        t, s, e = facts['named_runs'][key]
        assert any(f[5] == gen[t][0] and int(f[7]) < s and e < int(f[8]) for f in lines), key
    (th, _, he), (tt, ts, _) = facts['head_run'], facts['tail_run']
    assert any((f[5] == gen[th][0] and int(f[7]) == he) or (f[5] == gen[tt][0] and int(f[8]) == ts) for f in lines)
    return lines


@pytest.mark.parametrize('name,kw', [('dirty', dict(best_n=5, pri_ratio=0.8)), ('dirty', NP), ('dirty', dict(best_n=5, pri_ratio=0.8, with_cigar=0)),
                                     ('dirty_plus1', NP), ('many', NP)])
def test_paf_matches_oracle(worlds, name, kw):
    from megapath_nano_amd import mapper
    wd = worlds[name]
    got = mapper.map_batch(wd.gidx, mapper.default_opt(**kw), wd.names, wd.seqs)
    want = wd.oracle_paf(**kw)
    assert_paf_matches(got, want, wd.reads, (name, kw))
    if name == 'many':
        assert sum(1 for x in want if x) >= 55
    elif kw.get('with_cigar', 1):   # (without the extension a hit ends on its outermost seeds)
        lines = assert_runs_inside_hits(got, wd.facts, wd.gen)
        nn = [int(x[5:]) for f in lines for x in f[12:] if x.startswith('nn:i:')]
        assert max(nn) >= 300 and {1, 21, 63, 301} <= set(nn), sorted(nn)
    else:
        assert got.count('\n') >= len(wd.reads)


def test_tags_and_sam_over_dirty_targets(worlds):
    from megapath_nano_amd import mapper
    from oracle import mm2_bindings as mb
    wd = worlds['dirty']
    packed = mapper.PackedReads(wd.names, wd.seqs)
    ref = SimpleNamespace(rcodes={n: codes(s) for n, s in zip(wd.names, wd.seqs)}, tcodes={n: codes(s) for n, s in wd.gen})
    want_paf = ''.join(wd.oracle_paf(**NP))
    want_sam = ''.join(mb.map_read_sam(wd.oidx, mb.default_opt(**NP), n, s) for n, s in zip(wd.names, wd.seqs))
    assert mapper.map_batch(wd.gidx, mapper.default_opt(out_sam=1, **NP), wd.names, wd.seqs) == want_sam
    paf, sam, _ = mapper.map_batch_full(wd.gidx, mapper.default_opt(out_sam=2, out_tags=CS | MD, **NP), packed, want_paf=True, want_cols=False)
    recs = check_paf(ref, paf)
    check_sam(ref, sam)
    assert strip_tags(paf) == want_paf and strip_tags(sam) == want_sam
    assert any(r['name'] == 'run_300' and '*' in r['cs'] and r['cs'].count('n') >= 300 for r in recs)   # target N against a read base
    paf, sam, _ = mapper.map_batch_full(wd.gidx, mapper.default_opt(out_sam=2, out_tags=CS | MD | EQX, **NP), packed, want_paf=True, want_cols=False)
    assert len(check_paf(ref, paf, eqx=True)) == len(recs) > 15
    check_sam(ref, sam, eqx=True)


# ------------------------------------------------------------------------------------------------------ one index, four routes

def test_same_index_by_every_route(worlds, tmp_path):
    import torch
    from megapath_nano_amd import mapper
    wd = worlds['dirty']
    names, lens = [n for n, _ in wd.gen], [len(s) for _, s in wd.gen]
    flat = np.concatenate([s for _, s in wd.gen])
    dev = torch.device('cuda', 0)
    aligned = torch.zeros(len(flat) + 64, dtype=torch.uint8, device=dev)
    aligned[:len(flat)] = torch.from_numpy(flat).to(dev)
    shifted = torch.zeros(len(flat) + 64, dtype=torch.uint8, device=dev)
    shifted[1:1 + len(flat)] = torch.from_numpy(flat).to(dev)
    torch.cuda.synchronize(dev)
    assert aligned.data_ptr() % 16 == 0 and (shifted.data_ptr() + 1) % 16 == 1
    path = str(tmp_path / 'dirty.mpi')
    wd.gidx.save(path)
    routes = {'from_device aligned': mapper.Index.from_device(names, aligned.data_ptr(), lens),
              'from_device at an odd offset': mapper.Index.from_device(names, shifted.data_ptr() + 1, lens),
              'save + load': mapper.Index.load(path)}
    try:
        want_exp = wd.gidx.export()
        want_seq = [tc.decoded(s) for _, s in wd.gen]
        want_paf = mapper.map_batch(wd.gidx, mapper.default_opt(**NP), wd.names, wd.seqs)
        assert_paf_matches(want_paf, wd.oracle_paf(**NP), wd.reads, 'built from host sequences')
        for what, idx in routes.items():
            assert idx.names == names and list(idx.lens) == lens, what
            for a, b in zip(idx.export(), want_exp):
                assert np.array_equal(a, b), what
            assert [idx.fetch_seq(t, 0, n) for t, n in enumerate(lens)] == want_seq, what
            assert [idx.mid_occ(f) for f in FRACS] == [wd.gidx.mid_occ(f) for f in FRACS], what
            assert mapper.map_batch(idx, mapper.default_opt(**NP), wd.names, wd.seqs) == want_paf, what
    finally:
        for idx in routes.values():
            idx.close()


def test_split_parts_cut_inside_an_n_run(worlds):
    """three parts; the first ends with the N-tailed target, the second begins with the N-headed one"""
    from megapath_nano_amd import mapper
    from oracle import mm2_bindings as mb
    wd = worlds['dirty']
    a, b = wd.facts['split_cut']
    assert a == wd.facts['n_tail'] + 1 == wd.facts['n_head']
    parts = [wd.gen[:a], wd.gen[a:b], wd.gen[b:]]
    gparts, oparts = [mapper.Index(p) for p in parts], [mb.Index(p) for p in parts]
    sp = mb.SplitIndex(oparts)
    try:
        packed = mapper.PackedReads(wd.names, wd.seqs)
        gopt, oopt = mapper.default_opt(out_sam=2, **NP), mb.default_opt(**NP)
        want = [sp.map_read(oopt, n, s) for n, s in zip(wd.names, wd.seqs)]
        want_sam = ''.join(sp.map_read(oopt, n, s, sam=True) for n, s in zip(wd.names, wd.seqs))
        h = mapper.Hits(packed)
        for gp in gparts:
            h.add_part(gp, gopt)
        paf, sam, _ = h.finish(gopt, want_paf=True, want_cols=False)
        h.close()
        h = mapper.Hits(packed)
        h.add_parts(gparts, gopt)
        paf2, sam2, _ = h.finish(gopt, want_paf=True, want_cols=False)
        tnames, tlens = h.targets()
        h.close()
        assert tnames == [n for n, _ in wd.gen] and list(tlens) == [len(s) for _, s in wd.gen]
        assert_paf_matches(paf, want, wd.reads, 'parts one by one')
        assert paf2 == paf and sam2 == sam == want_sam
        assert_runs_inside_hits(paf, wd.facts, wd.gen)
    finally:
        sp.close()
        for x in gparts + oparts:
            x.close()


# -------------------------------------------------------------------------------------------------- sets without a minimizer

@pytest.mark.parametrize('which', [0, 1], ids=['one 10-base target', 'empty and all-N targets'])
def test_target_set_without_a_minimizer(libmpn, oracle_built, which, tmp_path):
    from megapath_nano_amd import mapper, synth
    from oracle import mm2_bindings as mb
    gen = tc.no_minimizer_sets()[which]
    rng = np.random.default_rng(8)
    reads = [('r3000', synth.ALPHA[rng.integers(0, 4, size=3000)]), ('n500', np.full(500, ord('N'), dtype=np.uint8)),
             ('r9', synth.ALPHA[rng.integers(0, 4, size=9)]), ('copy', gen[0][1].copy() if len(gen[0][1]) else synth.ALPHA[rng.integers(0, 4, size=40)])]
    names, seqs = [n for n, _ in reads], [s for _, s in reads]
    gidx, oidx = mapper.Index(gen), mb.Index(gen)
    try:
        assert (gidx.n_keys, gidx.n_minimizers) == (0, 0)
        assert all(len(a) == n for a, n in zip(gidx.export(), (0, 1, 0)))
        assert [gidx.mid_occ(f) for f in FRACS] == [oidx.mid_occ(f) for f in FRACS]
        assert [gidx.fetch_seq(t, 0, len(s)) for t, (_, s) in enumerate(gen)] == [tc.decoded(s) for _, s in gen]
        path = str(tmp_path / 'none.mpi')
        gidx.save(path)
        loaded = mapper.Index.load(path)
        for idx in (gidx, loaded):
            assert mapper.map_batch(idx, mapper.default_opt(**NP), names, seqs) == ''
            assert ''.join(mb.map_read(oidx, mb.default_opt(**NP), n, s)[2] for n, s in reads) == ''
            sam = mapper.map_batch(idx, mapper.default_opt(out_sam=1, **NP), names, seqs)
            assert sam == ''.join(mb.map_read_sam(oidx, mb.default_opt(**NP), n, s) for n, s in reads)
            assert [l.split('\t')[1] for l in sam.splitlines()] == ['4'] * len(reads)
        loaded.close()
    finally:
        gidx.close()
        oidx.close()


# -------------------------------------------------------------------------------------- alternate dispatch paths, one child each

@pytest.fixture(scope='module')
def child_world(libmpn, oracle_built, tmp_path_factory):
    gen, reads, _ = tc.dirty_world('mult16')
    w = ChildWorld('dirty', gen, reads, dict(NP), str(tmp_path_factory.mktemp('target_children') / 'dirty.npz'))
    yield w
    w.close()


@pytest.mark.parametrize('knob,value', [('MPN_TILED', '0'), ('MPN_HOST_HITS', '1')])
def test_dirty_paf_on_the_alternate_paths(child_world, tmp_path, knob, value):
    r = run_child(tmp_path, {knob: value}, [(child_world, 'paf')], timeout=300)[0]
    assert_paf_matches(r['paf'], child_world.paf(), child_world.reads, f'{knob}={value}')
    assert any('nn:i:301' in l for l in r['paf'].splitlines())
    if knob == 'MPN_TILED':
        assert r['stats']['tile_windows'] == 0
    else:
        assert r['stats']['reads_hits_on_host'] == sum(1 for c in child_world.n_chains() if c > 0) >= 15
