"""GPU tests (-m gpu) of index parts sharded over ranks: the hits of a range of reads exported from the
accumulators of contiguous part blocks and imported in part order give, bit for bit, what one accumulator over every part gives;
a bad block is refused and leaves the process usable; and align_and_assign over a ShardedIndex in W = 2 and W = 4 gloo ranks on
one GPU returns the counters of the single-process run.

The world is the strain-rich set of test_dispatch_paths_gpu.py (several hits per read), cut into four index parts: targets
0-29 (the three community genomes and the unrelated genome 3), 30-69, 70-99, 100-129 (40 assemblies per community genome
follow the 10 random genomes, so genome 1's and genome 2's strains span the two halves)."""
import json
import os
import random
import socket
import subprocess
import sys

import numpy as np
import pytest

from test_dispatch_paths_gpu import _strain_rich_world

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUT = [0, 30, 70, 100, 130]
OPTS = {'N5_p0.8': dict(best_n=5, pri_ratio=0.8), 'N50_p1': dict(best_n=50, pri_ratio=1.0)}
TB_SEED = 77


def _taxonomy(n):
    """names: the 10 random genomes each, the strain assemblies 4 to a name; species: 3 names to a species"""
    from megapath_nano_amd.pipeline import Taxonomy
    name = np.array([i if i < 10 else 10 + (i - 10) // 4 for i in range(n)], dtype=np.int32)
    n_names = int(name.max()) + 1
    return Taxonomy(name, n_names, name // 3, n_names // 3 + 1)


@pytest.fixture(scope='module')
def world(libmpn, tmp_path_factory):
    from megapath_nano_amd import mapper
    gen, reads, _ = _strain_rich_world()
    assert len(gen) == CUT[-1]
    parts = [mapper.Index(gen[a:b]) for a, b in zip(CUT, CUT[1:])]
    packed = mapper.PackedReads([r['name'] for r in reads], [r['seq'] for r in reads])
    d = tmp_path_factory.mktemp('index_shards')
    path = str(d / 'world.npz')
    cat = lambda seqs: np.concatenate([np.asarray(s, dtype=np.uint8) for s in seqs])  # noqa: E731
    np.savez(path, gbuf=cat([s for _, s in gen]), glen=np.array([len(s) for _, s in gen], dtype=np.int64),
             gnames=np.array([n for n, _ in gen]), rbuf=cat([r['seq'] for r in reads]),
             rlen=np.array([len(r['seq']) for r in reads], dtype=np.int64), rnames=np.array([r['name'] for r in reads]))
    yield dict(gen=gen, reads=reads, parts=parts, packed=packed, path=path)
    for p in parts:
        p.close()


def _hits(packed, parts, opt, want_text):
    from megapath_nano_amd import mapper
    h = mapper.Hits(packed, want_text=want_text)
    h.add_parts(parts, opt)
    return h


def _finish(h, opt, want_text):
    if want_text:
        paf, sam, cols = h.finish(opt, want_paf=True, want_cols=True)
        return paf, sam, cols
    return None, None, h.finish(opt, want_paf=False, want_cols=True)[2]


def _lines_of(text, names):
    names = set(names)
    return ''.join(l for l in text.splitlines(keepends=True) if l.split('\t', 1)[0] in names)


def _rows_of(cols, lo, hi):
    m = (cols['read_idx'] >= lo) & (cols['read_idx'] < hi)
    out = {k: v[m].copy() for k, v in cols.items()}
    out['read_idx'] -= lo
    return out


def _ranges(n, ref_cols, shard_a_targets):
    """[0, n), [0, n/3), [n/3, n), an empty range, and the longest run of reads with hits, none of them in shard B"""
    rid_by_read = [ref_cols['rid'][ref_cols['read_idx'] == i] for i in range(n)]
    only_a = [len(r) > 0 and bool((r < shard_a_targets).all()) for r in rid_by_read]
    best, run_lo = (0, 0), None
    for i, ok in enumerate(only_a + [False]):
        if ok and run_lo is None:
            run_lo = i
        elif not ok and run_lo is not None:
            if i - run_lo > best[1] - best[0]:
                best = (run_lo, i)
            run_lo = None
    assert best[1] > best[0], 'the world should have reads whose hits all lie in shard A'
    return [(0, n), (0, n // 3), (n // 3, n), (n // 2, n // 2), best]


@pytest.mark.parametrize('want_text', [True, False], ids=['text', 'columns'])
@pytest.mark.parametrize('optname', list(OPTS))
def test_export_import_bit_exact(world, optname, want_text):
    from megapath_nano_amd import mapper
    opt = mapper.default_opt(**OPTS[optname], out_sam=2 if want_text else 0)
    parts, packed = world['parts'], world['packed']
    n = packed.n
    ref = _hits(packed, parts, opt, want_text)
    ref_names, ref_lens = ref.targets()
    ref_paf, ref_sam, ref_cols = _finish(ref, opt, want_text)
    ref.close()
    assert len(ref_cols['read_idx']) > 4 * n, 'the world should bring several hits per read'
    ranges = _ranges(n, ref_cols, CUT[2])
    for split in ((2,), (1,)):   # shards {0, 1} + {2, 3}, then {0} + {1, 2, 3}
        k = split[0]
        shards = [_hits(packed, parts[:k], opt, want_text), _hits(packed, parts[k:], opt, want_text)]
        try:
            for lo, hi in ranges:
                acc = mapper.Hits(packed.sub(lo, hi), want_text=want_text)
                for s, sh in enumerate(shards):           # in shard order: part order, rid shift, rep_len max
                    acc.import_block(sh.export(lo, hi), [k, len(parts) - k][s], *sh.targets())
                names, lens = acc.targets()
                assert names == ref_names and np.array_equal(lens, ref_lens), 'target order'
                paf, sam, cols = _finish(acc, opt, want_text)
                acc.close()
                what = (optname, f'{k}+{len(parts) - k}', (lo, hi))
                if want_text:
                    sel = packed.names[lo:hi]
                    assert paf == _lines_of(ref_paf, sel), what
                    assert sam == _lines_of(ref_sam, sel), what
                want = _rows_of(ref_cols, lo, hi)
                for c in mapper.COL_NAMES:
                    assert np.array_equal(cols[c], want[c]), (what, c)
                assert hi > lo or len(cols['read_idx']) == 0
        finally:
            for sh in shards:
                sh.close()


def test_bad_blocks_are_refused(world):
    from megapath_nano_amd import mapper
    from megapath_nano_amd._ffi import MpnError
    opt = mapper.default_opt(**OPTS['N50_p1'])
    parts, packed, gen = world['parts'], world['packed'], world['gen']
    n = packed.n
    ref = _hits(packed, parts, opt, False)
    want = _finish(ref, opt, False)[2]
    ref.close()
    a, b = _hits(packed, parts[:2], opt, False), _hits(packed, parts[2:], opt, False)
    a_t, b_t = a.targets(), b.targets()
    blk_a, blk_b = a.export(0, n), b.export(0, n)
    k13 = mapper.Index(gen[:10], k=13)
    other_k = _hits(packed, [k13], mapper.default_opt(**OPTS['N50_p1'], k=13), False)
    text = _hits(packed, parts[2:], opt, True)
    acc = mapper.Hits(packed, want_text=False)
    try:
        assert len(blk_a) > 64 and len(blk_b) > 64
        acc.import_block(blk_a, 2, *a_t)
        with pytest.raises(MpnError, match='k = 13'):
            acc.import_block(other_k.export(0, n), 1, *other_k.targets())
        with pytest.raises(MpnError, match='CIGAR'):
            acc.import_block(text.export(0, n), 2, *text.targets())
        with pytest.raises(MpnError, match='reads'):
            acc.import_block(b.export(0, n - 1), 2, *b_t)
        for cut in list(range(0, 65)) + [len(blk_b) - 1]:
            with pytest.raises(MpnError):
                acc.import_block(blk_b[:cut], 2, *b_t)
        bad = blk_b.copy()
        bad[1] ^= 0x40
        with pytest.raises(MpnError, match='magic'):
            acc.import_block(bad, 2, *b_t)
        bad = blk_b.copy()
        bad[len(bad) // 2] ^= 0x10
        with pytest.raises(MpnError, match='corrupt'):
            acc.import_block(bad, 2, *b_t)
        with pytest.raises(MpnError):
            acc.import_block(blk_b, 2, b_t[0][:-1], b_t[1][:-1])   # a target list other than the exporter's
        acc.import_block(blk_b, 2, *b_t)                            # the accumulator is as it was before the refusals
        got = _finish(acc, opt, False)[2]
        for c in mapper.COL_NAMES:
            assert np.array_equal(got[c], want[c]), c
    finally:
        for h in (acc, a, b, other_k, text):
            h.close()
        k13.close()


# ------------------------------------------------------------------------------------------------------------------ ranks

_CHILD = r'''
import datetime, json, os, random, sys
import numpy as np
root, spec = sys.argv[1], json.loads(sys.argv[2])
sys.path.insert(0, root)
import torch
torch.cuda.init()
import torch.distributed as dist
rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
dist.init_process_group('gloo', rank=rank, world_size=world, timeout=datetime.timedelta(seconds=spec['pg_timeout']))
from megapath_nano_amd import dist as mdist, mapper
from megapath_nano_amd.pipeline import ShardedIndex, Taxonomy, align_and_assign
z = np.load(spec['world'])
split = lambda buf, lens: np.split(buf, np.cumsum(lens)[:-1])
gen = list(zip([str(x) for x in z['gnames']], split(z['gbuf'], z['glen'])))
rnames, rseqs = [str(x) for x in z['rnames']], split(z['rbuf'], z['rlen'])
S, cut = spec['shards'], spec['cut']
part_bases = [int(z['glen'][a:b].sum()) for a, b in zip(cut, cut[1:])]
g, s = mdist.index_shard_layout(rank, world, S)
pa, pb = mdist.assign_parts(part_bases, S)[s]
groups = mdist.shard_groups(world, S)
sidx = ShardedIndex([mapper.Index(gen[cut[p]:cut[p + 1]]) for p in range(pa, pb)], rank, world, S, groups)
glo, ghi = mdist.owner_bounds(z['rlen'], world // S, S)[0][g]
packed = mapper.PackedReads(rnames[glo:ghi], rseqs[glo:ghi])
t = spec['tax']
tax = Taxonomy(np.array(t[0], dtype=np.int32), t[1], np.array(t[2], dtype=np.int32), t[3])
opt = mapper.default_opt(**spec['opt'])
out = align_and_assign(sidx, opt, packed, tax, allreduce=mdist.make_allreduce(None), rng=random.Random(spec['seed']),
                       shard=(rank, world))
names, lens = sidx.all_targets()
res = dict(rank=rank, read_count=out['read_count'].tolist(), aligned_bp=out['aligned_bp'].tolist(), n_rows=out['n_rows'],
           n_relations=out['n_relations'], parts=[pa, pb], owned=[glo + x for x in sidx.times['owned']], targets=names == [n for n, _ in gen])
sidx.close()
dist.destroy_process_group()
with open(spec['out'] % rank, 'w') as f:
    json.dump(res, f)
print('CHILD_OK')
'''

_faulted = []   # once a child has failed or timed out, no more children are started


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def run_ranks(tmp_path, world_path, world_size, shards, tax, opt_kw, timeout=600):
    if _faulted:
        pytest.fail('not started: an earlier child failed (' + _faulted[0] + ')')
    spec = dict(world=world_path, shards=shards, cut=CUT, opt=opt_kw, seed=TB_SEED, pg_timeout=300, out=str(tmp_path / 'rank%d.json'),
                tax=[tax.name_code.tolist(), tax.n_names, tax.species_code.tolist(), tax.n_species])
    port = _free_port()
    procs = []
    for r in range(world_size):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world_size), LOCAL_RANK=str(r), LOCAL_WORLD_SIZE=str(world_size),
                   MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), MPN_SINGLE_DEVICE='1', MPN_DIST_BACKEND='gloo',
                   MPN_PIPE_WORKERS='2', MPN_RANKS_ON_NODE=str(world_size))
        procs.append(subprocess.Popen([sys.executable, '-c', _CHILD, ROOT, json.dumps(spec)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = [None] * world_size
    try:
        for r, p in enumerate(procs):
            outs[r] = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        _faulted.append(f'W={world_size} S={shards}: time limit')
        pytest.fail(f'ranks W={world_size} S={shards} exceeded {timeout} s')
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    bad = [(r, p.returncode) for r, p in enumerate(procs) if p.returncode != 0 or 'CHILD_OK' not in (outs[r] or ('', ''))[0]]
    if bad:
        _faulted.append(f'W={world_size} S={shards}: ranks {bad}')
        pytest.fail(f'ranks failed {bad}; stderr tails:\n' + '\n'.join((o or ('', ''))[1][-2000:] for o in outs))
    return [json.load(open(tmp_path / f'rank{r}.json')) for r in range(world_size)]


@pytest.mark.parametrize('world_size,shards', [(2, 2), (4, 2)], ids=['W2_S2', 'W4_S2_R2'])
def test_sharded_ranks_equal_single_process(world, tmp_path, world_size, shards):
    from megapath_nano_amd import mapper
    from megapath_nano_amd.pipeline import align_and_assign
    opt_kw = OPTS['N50_p1']
    tax = _taxonomy(CUT[-1])
    want = align_and_assign(world['parts'], mapper.default_opt(**opt_kw), world['packed'], tax, rng=random.Random(TB_SEED))
    got = run_ranks(tmp_path, world['path'], world_size, shards, tax, opt_kw)
    assert [g['parts'] for g in got] == [[0, 2], [2, 4]] * (world_size // shards)
    from megapath_nano_amd.dist import owner_bounds
    assert [tuple(g['owned']) for g in got] == owner_bounds(world['packed'].lens, world_size // shards, shards)[1]
    for g in got:
        assert g['targets'], 'the gathered target lists, in shard order, are the single-process list'
        assert g['read_count'] == want['read_count'].tolist(), g['rank']
        assert g['aligned_bp'] == want['aligned_bp'].tolist(), g['rank']
        if g['n_rows']:
            assert g['n_relations'] == want['n_relations'], g['rank']
    assert sum(g['n_rows'] for g in got) == want['n_rows']
    assert want['n_relations'] > 0 and want['n_rows'] > 4 * world['packed'].n


def test_ranks_load_only_their_parts(world, tmp_path):
    """A saved four-part index is placed from the part headers alone; each shard loads its block, and a target stream cut into
    parts feeds the same layout."""
    from megapath_nano_amd import mapper
    from megapath_nano_amd.dist import assign_parts
    from megapath_nano_amd.pipeline import own_saved_parts, own_target_parts
    path = str(tmp_path / 'four.mpi')
    for i, p in enumerate(world['parts']):
        p.save(path, append=i > 0)
    info = mapper.Index.part_info(path)
    gen = world['gen']
    assert [(n, b) for _, n, b in info] == [(b - a, sum(len(s) for _, s in gen[a:b])) for a, b in zip(CUT, CUT[1:])]
    assert info[0][0] == 0 and all(info[i][0] < info[i + 1][0] for i in range(3))
    blocks = assign_parts([b for _, _, b in info], 2)
    for rank in range(4):
        got = own_saved_parts(path, rank, 4, 2)
        a, b = blocks[rank % 2]
        assert [p.names for p in got] == [world['parts'][i].names for i in range(a, b)]
        for p in got:
            p.close()
    streamed = lambda: iter([gen[a:b] for a, b in zip(CUT, CUT[1:])])  # noqa: E731
    got = own_target_parts(streamed, 1, 2, 2)
    assert [p.names for p in got] == [world['parts'][i].names for i in range(*blocks[1])]
    for p in got:
        p.close()
