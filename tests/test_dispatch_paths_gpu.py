"""GPU parity (-m gpu) of the mapper's ALTERNATE dispatch paths against oracle/mm2_oracle.c, bit for bit.

The mapper chooses at run time between kernel variants and host fallbacks; the rest of the suite sees the default choice for
its data.  Here every choice is forced (or, for the >384-chain host fallback, reached by the data) and its PAF text or chains
are compared with the oracle:

  * hit selection on the host for every read (MPN_HOST_HITS=1), GPU and host mixed in one batch (MPN_HIT_MAX_CHAINS), the
    natural host fallback of reads with more than HIT_MAX_CHAINS (384) chains, both hit_select_kernel instantiations (48 / 49);
  * the parallel chain backtrack (a lane per chain end, ownership by atomicMin) and the sequential walk (MPN_BT_PAR_MIN);
  * chain-DP work items of 16 and 4096 anchors (MPN_CHAIN_ITEM);
  * the seed filter with a second counting round (MPN_FLT_ROUND2) and with one workgroup (MPN_FLT_WGS);
  * long gap fills on the band kernel instead of the tiled strips (MPN_TILED=0).

The knobs are read once per process, so every setting runs in a child process of its own that only maps and reports; the
oracle side is computed here, once per world.  Children run one at a time; once a child has faulted, timed out or died on a
signal, no later child is started.
"""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from map_cases import hard_reads, small_world

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIT_MAX_CHAINS, HIT_SMALL_CHAINS = 384, 48     # csrc/hit_kernels.h
NO_CUTOFF = 100000                             # mid_occ high enough that every copy of a repeated sequence is seeded
STRAIN_CUT = (40, 90)                          # the strain-rich set as three index parts (minimap2 -I)


# ---------------------------------------------------------------------------------------------------------------- worlds

def _strain_rich_world():
    """3 community genomes x 40 assemblies at 97-99.9 % identity beside 10 random genomes (130 x 100 kb), `-N 50 -p 1`:
    dozens of chains per read (a read in a genome's internal repeat: hundreds)."""
    import torch
    from megapath_nano_amd import synth
    glen, n_fam, copies, n_rand = 100_000, 3, 40, 10
    n = n_rand + n_fam * copies
    names, flat, lens = synth.make_genomes_device(4711, n, glen, 0, torch.device('cuda', 0), families=(n_fam, copies, 0.97, 0.999))
    host = flat.view(n, glen).cpu().numpy()
    del flat
    gen = [(names[i], host[i]) for i in range(n)]
    w = np.zeros(n)
    w[:n_fam + 1] = [3, 2, 1, 1]   # (genome 3 is unrelated: reads with one chain)
    reads = synth.make_reads(99, gen, 40, mean_len=5000, weights=w, random_frac=0.05) + \
        synth.make_reads(98, gen, 4, mean_len=20000, min_len=15000, weights=w)
    for i, r in enumerate(reads):
        r['name'] = f'sr{i:03d}'
    return gen, reads, dict(best_n=50, pri_ratio=1.0)


def _many_copy_world():
    """420 diverged copies (1 % substitutions each) of one 20 kb sequence and an unrelated genome, no occurrence cut-off: a read of
    the sequence has a chain on every copy (> HIT_MAX_CHAINS), a read of the other genome has one."""
    from megapath_nano_amd import synth
    rng = np.random.default_rng(21)
    base = synth.ALPHA[rng.integers(0, 4, size=20000)]
    gen = []
    for c in range(420):
        s = base.copy()
        pos = rng.integers(0, len(s), size=200)
        s[pos] = synth.ALPHA[rng.integers(0, 4, size=200)]
        gen.append((f'copy{c:03d}', s))
    other = synth.ALPHA[rng.integers(0, 4, size=40000)]
    gen.append(('other', other))
    reads = []
    for k in range(12):
        L = int(rng.integers(3000, 8000))
        st = int(rng.integers(0, len(base) - L))
        q = synth.ont_errors(rng, base[st:st + L], 0.02, 0.01, 0.01)
        reads.append(dict(name=f'mc{k:02d}', seq=q if k % 2 == 0 else synth.COMP[q[::-1]]))
    for k in range(4):
        st = int(rng.integers(0, len(other) - 5000))
        reads.append(dict(name=f'oth{k}', seq=other[st:st + 5000].copy()))
    return gen, reads, dict(mid_occ=NO_CUTOFF)


def _tandem_world():
    """the target set of test_map_stages_gpu.py::test_seed_chain_through_a_tandem_repeat (a 37-bp unit x 220 in one target)"""
    from megapath_nano_amd import synth
    rng = np.random.default_rng(11)
    unit = synth.ALPHA[rng.integers(0, 4, size=37)]
    left, right = synth.ALPHA[rng.integers(0, 4, size=6000)], synth.ALPHA[rng.integers(0, 4, size=6000)]
    rep = np.tile(unit, 220)
    pos = rng.integers(0, len(rep), size=120)
    rep[pos] = synth.ALPHA[rng.integers(0, 4, size=120)]
    gen = [('flank_only', np.concatenate([left, right])), ('with_repeat', np.concatenate([left, rep, right])),
           ('other', synth.ALPHA[rng.integers(0, 4, size=9000)])]
    target = gen[1][1]
    reads = []
    for k in range(8):
        st = int(rng.integers(3000, 5500))
        q = target[st:st + int(rng.integers(6000, 11000))].copy()
        p = rng.integers(0, len(q), size=len(q) // 25)
        q[p] = synth.ALPHA[rng.integers(0, 4, size=len(p))]
        reads.append(dict(name=f'tr{k}', seq=q if k % 2 == 0 else synth.COMP[q[::-1]]))
    return gen, reads, dict(mid_occ=NO_CUTOFF)


def _small_world():
    gen, reads = small_world()
    return gen, reads + hard_reads(gen), {}


def _save(path, gen, reads, opt):
    cat = lambda seqs: np.concatenate([np.asarray(s, dtype=np.uint8) for s in seqs])  # noqa: E731
    np.savez(path, meta=np.frombuffer(json.dumps(dict(targets=[n for n, _ in gen], reads=[r['name'] for r in reads],
                                                      opt=opt)).encode(), dtype=np.uint8),
             gbuf=cat([s for _, s in gen]), glen=np.array([len(s) for _, s in gen], dtype=np.int64),
             rbuf=cat([r['seq'] for r in reads]), rlen=np.array([len(r['seq']) for r in reads], dtype=np.int64))


class World:
    """A target set + reads, saved for the children, with the oracle's chains and PAF computed on first use."""

    def __init__(self, name, gen, reads, opt, path):
        from oracle import mm2_bindings as mb
        self.name, self.gen, self.reads, self.opt, self.path = name, gen, reads, opt, path
        _save(path, gen, reads, opt)
        self.oidx = mb.Index(gen)
        self.mid_occ = opt.get('mid_occ') or self.oidx.mid_occ()
        self._chains, self._paf, self._split, self._gidx = None, {}, None, None

    def gidx(self):
        from megapath_nano_amd import mapper
        if self._gidx is None:
            self._gidx = mapper.Index(self.gen)
        return self._gidx

    def chains(self):
        """-> per read (n_anchor, rep_len, u, b), as test_map_stages_gpu.py computes them"""
        from oracle import mm2_bindings as mb
        if self._chains is None:
            oopt = mb.default_opt(**self.opt)

            def one(r):
                a, rep = mb.collect_anchors(self.oidx, self.mid_occ, mb.sketch(r['seq'], 10, 15, 0), len(r['seq']))
                u, b = mb.chain(oopt, a)
                return len(a), rep, u, b
            with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
                self._chains = list(ex.map(one, self.reads))
        return self._chains

    def n_chains(self):
        return [len(c[2]) for c in self.chains()]

    def paf(self, with_cigar=1):
        from oracle import mm2_bindings as mb
        if with_cigar not in self._paf:
            oopt = mb.default_opt(with_cigar=with_cigar, **self.opt)
            with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
                self._paf[with_cigar] = list(ex.map(lambda r: mb.map_read(self.oidx, oopt, r['name'], r['seq'])[2], self.reads))
        return self._paf[with_cigar]

    def split_paf(self):
        """the oracle's --split-prefix merge over the parts of STRAIN_CUT"""
        from oracle import mm2_bindings as mb
        if self._split is None:
            cut = [0, *STRAIN_CUT, len(self.gen)]
            oparts = [mb.Index(self.gen[a:b]) for a, b in zip(cut, cut[1:])]
            sp = mb.SplitIndex(oparts)
            try:
                oopt = mb.default_opt(**self.opt)
                self._split = [sp.map_read(oopt, r['name'], r['seq']) for r in self.reads]
            finally:
                sp.close()
                for p in oparts:
                    p.close()
        return self._split

    def close(self):
        self.oidx.close()
        if self._gidx is not None:
            self._gidx.close()


@pytest.fixture(scope='module')
def worlds(libmpn, oracle_built, tmp_path_factory):
    os.environ.setdefault('OMP_NUM_THREADS', str(min(16, os.cpu_count() or 1)))
    d = tmp_path_factory.mktemp('dispatch_worlds')
    out = {}
    for name, make in (('small', _small_world), ('strain', _strain_rich_world), ('many', _many_copy_world), ('tandem', _tandem_world)):
        gen, reads, opt = make()
        out[name] = World(name, gen, reads, opt, str(d / f'{name}.npz'))
    yield out
    for w in out.values():
        w.close()


# -------------------------------------------------------------------------------------------------------------- checkers

def assert_paf_matches(got, want, reads, what):
    by = {}
    for line in got.splitlines(keepends=True):
        by.setdefault(line.split('\t', 1)[0], []).append(line)
    for r, w in zip(reads, want):
        g = ''.join(by.pop(r['name'], []))
        assert g == w, (what, r['name'], len(r['seq']), g[:600], w[:600])
    assert not by, (what, 'lines of unknown reads', sorted(by)[:5])


def assert_chains_match(got, world, what):
    """got: per read (n_anchor, rep_len, u, b) from seed_chain_batch"""
    want = world.chains()
    assert len(got) == len(want), what
    for r, g, w in zip(world.reads, got, want):
        assert (g[0], g[1]) == (w[0], w[1]), (what, r['name'], 'n_anchor / rep_len', g[:2], w[:2])
        assert np.array_equal(g[2], w[2]), (what, r['name'], 'chains (score, count)', len(g[2]), len(w[2]))
        assert np.array_equal(g[3], w[3]), (what, r['name'], 'chained anchors', len(g[3]), len(w[3]))


def gpu_opt(world, **kw):
    from megapath_nano_amd import mapper
    return mapper.default_opt(**{**world.opt, **kw})


# --------------------------------------------------------------------------------------------------------------- children

_CHILD = r'''
import json, os, sys
import numpy as np
root, spec = sys.argv[1], json.load(open(sys.argv[2]))
sys.path.insert(0, root)
from megapath_nano_amd import mapper

def load(path):
    z = np.load(path)
    meta = json.loads(bytes(z['meta']).decode())
    split = lambda buf, lens: np.split(buf, np.cumsum(lens)[:-1]) if len(lens) else []
    return meta, list(zip(meta['targets'], split(z['gbuf'], z['glen']))), meta['reads'], split(z['rbuf'], z['rlen'])

res = []
for job in spec['jobs']:
    meta, gen, names, seqs = load(job['world'])
    opt = mapper.default_opt(**meta['opt'], **job.get('opt', {}))
    out = dict(kind=job['kind'])
    if job['kind'] == 'paf':
        idx = mapper.Index(gen)
        out['paf'] = mapper.map_batch(idx, opt, names, seqs)
        out['stats'] = mapper.last_stats()
        idx.close()
    elif job['kind'] == 'parts':
        cut = [0] + job['cut'] + [len(gen)]
        parts = [mapper.Index(gen[a:b]) for a, b in zip(cut, cut[1:])]
        h = mapper.Hits(mapper.PackedReads(names, seqs))
        h.add_parts(parts, opt)
        out['paf'] = h.finish(opt, want_paf=True, want_cols=False)[0]
        h.close()
        for p in parts:
            p.close()
    else:
        idx = mapper.Index(gen)
        got = mapper.seed_chain_batch(idx, opt, seqs)
        out['stats'] = mapper.last_stats()
        idx.close()
        np.savez(job['out'], n_anchor=np.array([g['n_anchor'] for g in got], dtype=np.int64),
                 rep_len=np.array([g['rep_len'] for g in got], dtype=np.int64),
                 n_u=np.array([len(g['u']) for g in got], dtype=np.int64), n_b=np.array([len(g['b']) for g in got], dtype=np.int64),
                 u=np.concatenate([g['u'] for g in got]), b=np.concatenate([g['b'] for g in got]).reshape(-1, 2))
    res.append(out)
json.dump(res, open(spec['result'], 'w'))
print('CHILD_OK')
'''

_FAULT_RCS = (124, 134, 137, 139)
_faulted = []   # set once a child has died on a signal, a fault status or the time limit: nothing more is started


def run_child(tmp_path, env, jobs, timeout=900):
    """Map in a fresh process with `env` added to the environment.  jobs: list of (world, kind[, opt]) with kind 'paf', 'parts'
    or 'chains'.  -> list of results: dict(paf, stats) for 'paf', dict(paf) for 'parts', dict(chains, stats) for 'chains'."""
    if _faulted:
        pytest.fail('not started: an earlier child faulted (' + _faulted[0] + ')')
    spec = dict(result=str(tmp_path / 'result.json'), jobs=[])
    for k, (world, kind, *opt) in enumerate(jobs):
        spec['jobs'].append(dict(world=world.path, kind=kind, opt=opt[0] if opt else {}, cut=list(STRAIN_CUT),
                                 out=str(tmp_path / f'chains{k}.npz')))
    with open(tmp_path / 'spec.json', 'w') as f:
        json.dump(spec, f)
    what = ' '.join(f'{k}={v}' for k, v in env.items())
    try:
        p = subprocess.run([sys.executable, '-c', _CHILD, ROOT, str(tmp_path / 'spec.json')], env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        _faulted.append(f'{what}: time limit')
        err = e.stderr.decode(errors='replace') if isinstance(e.stderr, bytes) else (e.stderr or '')
        pytest.fail(f'child [{what}] exceeded {timeout} s; stderr tail:\n{err[-3000:]}')
    if p.returncode < 0 or p.returncode in _FAULT_RCS:
        _faulted.append(f'{what}: exit status {p.returncode}')
        pytest.fail(f'child [{what}] ended with status {p.returncode}; stderr tail:\n{p.stderr[-3000:]}')
    assert p.returncode == 0 and 'CHILD_OK' in p.stdout, f'child [{what}] failed ({p.returncode}); stderr tail:\n{p.stderr[-3000:]}'
    with open(spec['result']) as f:
        res = json.load(f)
    for j, r in zip(spec['jobs'], res):
        if r['kind'] == 'chains':
            z = np.load(j['out'])
            ui, bi = np.cumsum(z['n_u'])[:-1], np.cumsum(z['n_b'])[:-1]
            r['chains'] = list(zip(z['n_anchor'].tolist(), z['rep_len'].tolist(), np.split(z['u'], ui), np.split(z['b'], bi)))
    print(f'[{what}]', [{k: r['stats'][k] for k in ('reads_hits_on_host', 'tile_windows', 'anchors_emitted')} if 'stats' in r else r['kind']
                        for r in res])
    return res


def reads_with_chains(world):
    return sum(1 for c in world.n_chains() if c > 0)


# ---------------------------------------------------------------------------------------------- default path, in process

def test_default_chains_and_worlds(worlds):
    """The default path's chains on every world, and what the worlds are for: reads on both sides of the 48-chain instantiation
    and of the 384-chain host fallback, anchors far beyond the chain DP's LDS tile in the tandem repeat."""
    from megapath_nano_amd import mapper
    counts = {}
    for name, w in worlds.items():
        got = mapper.seed_chain_batch(w.gidx(), gpu_opt(w), [r['seq'] for r in w.reads])
        assert_chains_match([(g['n_anchor'], g['rep_len'], g['u'], g['b']) for g in got], w, 'default ' + name)
        counts[name] = [len(g['u']) for g in got]
        print(f'[default {name}] anchors_emitted', mapper.last_stats()['anchors_emitted'])
    sr = counts['strain']
    assert any(0 < c <= HIT_SMALL_CHAINS for c in sr) and any(HIT_SMALL_CHAINS < c <= HIT_MAX_CHAINS for c in sr), sr
    assert any(c > HIT_MAX_CHAINS for c in sr), sr
    assert any(c < 3 for c in sr if c > 0), sr   # (MPN_HIT_MAX_CHAINS=3 keeps some reads on the GPU)
    mc = counts['many']
    assert sum(c > HIT_MAX_CHAINS for c in mc) >= 10 and any(0 < c <= HIT_MAX_CHAINS for c in mc), mc
    assert sum(w_[0] for w_ in worlds['tandem'].chains()) > 8 * 20000


@pytest.mark.parametrize('with_cigar', [0, 1])
def test_many_copies_take_the_host_fallback(worlds, with_cigar):
    """Reads with more than HIT_MAX_CHAINS chains take the host hit path with no knob set, beside GPU-selected reads in the same
    batch: the only test of that fallback exactly as users meet it."""
    from megapath_nano_amd import mapper
    w = worlds['many']
    got = mapper.map_batch(w.gidx(), gpu_opt(w, with_cigar=with_cigar), [r['name'] for r in w.reads], [r['seq'] for r in w.reads])
    st = mapper.last_stats()
    assert_paf_matches(got, w.paf(with_cigar), w.reads, f'many-copy, -c {with_cigar}')
    assert 0 < st['reads_hits_on_host'] < len(w.reads), st['reads_hits_on_host']
    assert st['reads_hits_on_host'] == sum(c > HIT_MAX_CHAINS for c in w.n_chains())


def test_default_paf_reaches_the_tiled_strips(worlds):
    from megapath_nano_amd import mapper
    w = worlds['small']
    got = mapper.map_batch(w.gidx(), gpu_opt(w), [r['name'] for r in w.reads], [r['seq'] for r in w.reads])
    st = mapper.last_stats()
    assert_paf_matches(got, w.paf(), w.reads, 'small, default')
    assert st['tile_windows'] > 0 and st['reads_hits_on_host'] == 0, st


# ------------------------------------------------------------------------------------------ forced paths, one child each

def test_host_hits_for_every_read(worlds, tmp_path):
    small, sr = worlds['small'], worlds['strain']
    res = run_child(tmp_path, {'MPN_HOST_HITS': '1'}, [(small, 'paf'), (sr, 'paf'), (sr, 'parts')])
    for w, r in zip((small, sr), res):
        assert_paf_matches(r['paf'], w.paf(), w.reads, 'MPN_HOST_HITS=1 ' + w.name)
        assert r['stats']['reads_hits_on_host'] == reads_with_chains(w), (w.name, r['stats']['reads_hits_on_host'])
    assert_paf_matches(res[2]['paf'], sr.split_paf(), sr.reads, 'MPN_HOST_HITS=1 three parts')


@pytest.mark.parametrize('k', [3, HIT_SMALL_CHAINS, HIT_SMALL_CHAINS + 1])
def test_gpu_and_host_hits_mixed(worlds, tmp_path, k):
    sr = worlds['strain']
    r = run_child(tmp_path, {'MPN_HIT_MAX_CHAINS': str(k)}, [(sr, 'paf')])[0]
    assert_paf_matches(r['paf'], sr.paf(), sr.reads, f'MPN_HIT_MAX_CHAINS={k}')
    host = r['stats']['reads_hits_on_host']
    assert 0 < host < reads_with_chains(sr), host
    assert host == sum(c > k for c in sr.n_chains()), host


@pytest.mark.parametrize('par_min', [1, 1000000000], ids=['parallel', 'sequential'])
def test_backtrack_paths(worlds, tmp_path, par_min):
    names = ('small', 'strain', 'many', 'tandem')
    res = run_child(tmp_path, {'MPN_BT_PAR_MIN': str(par_min)}, [(worlds[n], 'chains') for n in names])
    for n, r in zip(names, res):
        assert_chains_match(r['chains'], worlds[n], f'MPN_BT_PAR_MIN={par_min} {n}')


@pytest.mark.parametrize('item', [16, 4096])
def test_chain_dp_work_item_sizes(worlds, tmp_path, item):
    names = ('strain', 'tandem')
    res = run_child(tmp_path, {'MPN_CHAIN_ITEM': str(item)}, [(worlds[n], 'chains') for n in names])
    for n, r in zip(names, res):
        assert_chains_match(r['chains'], worlds[n], f'MPN_CHAIN_ITEM={item} {n}')


@pytest.mark.parametrize('knob', ['MPN_FLT_ROUND2', 'MPN_FLT_WGS'])
def test_seed_filter_variants(worlds, tmp_path, knob):
    names = ('many', 'strain')
    res = run_child(tmp_path, {knob: '1'}, [(worlds[n], 'chains') for n in names])
    for n, r in zip(names, res):
        assert_chains_match(r['chains'], worlds[n], f'{knob}=1 {n}')


def test_gap_fills_on_the_band_kernel(worlds, tmp_path):
    w = worlds['small']
    r = run_child(tmp_path, {'MPN_TILED': '0'}, [(w, 'paf')])[0]
    assert_paf_matches(r['paf'], w.paf(), w.reads, 'MPN_TILED=0')
    assert r['stats']['tile_windows'] == 0, r['stats']['tile_windows']


def test_mixed_hits_parallel_backtrack_band_kernel(worlds, tmp_path):
    sr = worlds['strain']
    env = {'MPN_HIT_MAX_CHAINS': str(HIT_SMALL_CHAINS), 'MPN_BT_PAR_MIN': '1', 'MPN_TILED': '0'}
    r = run_child(tmp_path, env, [(sr, 'paf')])[0]
    assert_paf_matches(r['paf'], sr.paf(), sr.reads, 'combined')
    assert 0 < r['stats']['reads_hits_on_host'] < reads_with_chains(sr) and r['stats']['tile_windows'] == 0, r['stats']
