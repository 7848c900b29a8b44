"""GPU tests (-m gpu) of cs / MD / =X output through the product calls: the strings the mapper writes for its own alignments of
map_cases.small_world() + hard_reads() against the plain-Python writer of diff_tags_ref.py (byte for byte, from each line's own
CIGAR, coordinates and strand), through mpn_map_batch_q, the split-index accumulator and the alternate dispatch paths."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from diff_tags_ref import (CS, CS_LONG, EQX, MD, MD_RE, cigar_text, codes, collapse_eqx, letters, parse_cigar, replay_cs, replay_md,
                           revcomp_codes, write_tags)
from map_cases import hard_reads, small_world

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS_RE, MD_TAG_RE = re.compile(r'\tcs:Z:[^\t\n]*'), re.compile(r'\tMD:Z:[^\t\n]*')


def strip_tags(text):
    return MD_TAG_RE.sub('', CS_RE.sub('', text))


class World:
    def __init__(self):
        from megapath_nano_amd import mapper
        gen, reads = small_world()
        reads = reads + hard_reads(gen)
        self.gen, self.reads = gen, reads
        self.names = [r['name'] for r in reads]
        self.seqs = [r['seq'] for r in reads]
        self.tcodes = {n: codes(s) for n, s in gen}
        self.rcodes = {r['name']: codes(r['seq']) for r in reads}
        self.idx = mapper.Index(gen)
        self.packed = mapper.PackedReads(self.names, self.seqs)
        self._runs = {}

    def run(self, out_tags, out_sam=2):
        """-> (PAF text, SAM text, columns, stats) of one call; cached (the text of a call is the reference of several tests)"""
        from megapath_nano_amd import mapper
        key = (out_tags, out_sam)
        if key not in self._runs:
            opt = mapper.default_opt(out_sam=out_sam, out_tags=out_tags)
            paf, sam, cols = mapper.map_batch_full(self.idx, opt, self.packed, want_paf=True, want_cols=True)
            self._runs[key] = (paf, sam, cols, mapper.last_stats())
        return self._runs[key]


@pytest.fixture(scope='module')
def world(libmpn):
    w = World()
    yield w
    w.idx.close()


def tag_names(fields):
    return [f[:2] for f in fields]


def check_paf(world, paf, long_form=False, eqx=False, want_md=True):
    """every PAF line that has cg:Z carries the tags, in order, equal to the writer's for the line's own alignment -> per-line records"""
    recs = []
    for line in paf.splitlines():
        f = line.split('\t')
        tags = f[12:]
        names = tag_names(tags)
        if 'cg' not in names:
            assert 'cs' not in names and 'MD' not in names, line[:300]
            continue
        assert names[-(3 + want_md):] == ['rl', 'cg', 'cs'] + (['MD'] if want_md else []), (names, line[:200])
        by = {t[:2]: t[5:] for t in tags}
        qs, qe, ts, te, rev = int(f[2]), int(f[3]), int(f[7]), int(f[8]), f[4] == '-'
        q = world.rcodes[f[0]][qs:qe]
        q = revcomp_codes(q) if rev else q
        t = world.tcodes[f[5]][ts:te]
        cig = parse_cigar(by['cg'])
        if eqx:
            assert 'M' not in by['cg'], by['cg'][:200]
        want = write_tags(collapse_eqx(cig), q, t)
        what = (f[0], f[4], qs, qe, f[5], ts, te)
        assert by['cs'] == want['cs_long' if long_form else 'cs'], what + (by['cs'][:300], want['cs_long' if long_form else 'cs'][:300])
        if want_md:
            assert by['MD'] == want['md'], what + (by['MD'][:300], want['md'][:300])
            assert MD_RE.match(by['MD'])
            assert replay_md(by['MD'], cig, letters(q)) == letters(t), what
        if eqx:
            assert cig == want['eqx'], what + (by['cg'][:300], cigar_text(want['eqx'])[:300])
        assert replay_cs(by['cs'], letters(t)) == letters(q), what
        recs.append(dict(name=f[0], rev=rev, qs=qs, qe=qe, cs=by['cs'], md=by.get('MD'), tp=by['tp'], zd='zd' in by, cg=by['cg']))
    return recs


def check_sam(world, sam, long_form=False, eqx=False, want_md=True):
    recs = []
    for line in sam.splitlines():
        f = line.split('\t')
        names = tag_names(f[11:])
        if f[5] == '*':
            assert 'cs' not in names and 'MD' not in names, line[:300]
            continue
        k = names.index('cs')
        assert names[k:] == ['cs'] + (['MD'] if want_md else []) + ['rl'] and names[k - 1] in ('SA', 'zd', 'de'), names
        by = {t[:2]: t[5:] for t in f[11:]}
        flag, pos = int(f[1]), int(f[3]) - 1
        ops = parse_cigar(f[5])
        clip0 = ops[0] >> 4 if ops[0] & 15 in (4, 5) else 0
        clip1 = ops[-1] >> 4 if ops[-1] & 15 in (4, 5) else 0
        cig = [c for c in ops if c & 15 not in (4, 5)]
        full = world.rcodes[f[0]]
        full = revcomp_codes(full) if flag & 16 else full
        q = full[clip0:len(full) - clip1]
        tspan = sum(c >> 4 for c in cig if c & 15 in (0, 2, 7, 8))
        t = world.tcodes[f[2]][pos:pos + tspan]
        if eqx:
            assert 'M' not in f[5]
        want = write_tags(collapse_eqx(cig), q, t)
        what = (f[0], flag, f[2], pos)
        assert by['cs'] == want['cs_long' if long_form else 'cs'], what
        if want_md:
            assert by['MD'] == want['md'], what
            assert replay_md(by['MD'], cig, letters(q)) == letters(t), what
        if eqx:
            assert cig == want['eqx'], what
        recs.append(dict(name=f[0], flag=flag))
    return recs


def assert_inputs_cover(paf_recs, sam_recs):
    """the reads really contain what the tests are for"""
    assert any(r['rev'] and '*' in r['cs'] and '+' in r['cs'] and '-' in r['cs'] for r in paf_recs), 'no - strand hit with all three events'
    assert any(r['name'] in ('with_n', 'n_run') and re.search(r'\*[acgt]n', r['cs']) for r in paf_recs), 'no hit over an N run'
    assert any(r['name'] in ('with_n', 'n_run') and re.search(r'\*[acgt]n\*[acgt]n\*[acgt]n', r['cs']) for r in paf_recs), 'no N run inside an alignment'
    assert any(r['name'] == 'lower' for r in paf_recs), 'the lower-case read has no alignment'
    assert any(r['flag'] & 0x800 for r in sam_recs), 'no supplementary record with a CIGAR'
    assert any(r['flag'] & 0x100 for r in sam_recs), 'no secondary record with a CIGAR'
    assert any(r['zd'] for r in paf_recs), 'no z-drop-cut hit'
    assert any(r['tp'] in 'Ii' for r in paf_recs), 'no inversion hit'
    assert any(r['name'] == 'long_60k' and r['qe'] - r['qs'] > 50000 for r in paf_recs), 'the 60-kb read is not aligned end to end'


def test_cs_and_md_present_and_correct(world):
    paf, sam, cols, st = world.run(CS | MD)
    paf_recs, sam_recs = check_paf(world, paf), check_sam(world, sam)
    assert len(paf_recs) == len(sam_recs) > 40
    assert_inputs_cover(paf_recs, sam_recs)
    assert st['k_tags_ns'] > 0, st['k_tags_ns']
    lower = [r for r in paf_recs if r['name'] == 'lower'][0]
    assert lower['cs'] == ':2000' and lower['md'] == '2000', (lower['cs'], lower['md'])


def test_nothing_else_changes(world):
    paf, sam, cols, _ = world.run(CS | MD)
    paf0, sam0, cols0, st0 = world.run(0)
    assert 'cs:Z:' not in paf0 + sam0 and 'MD:Z:' not in paf0 + sam0
    assert strip_tags(paf) == paf0
    assert strip_tags(sam) == sam0
    assert paf != paf0 and sam != sam0
    for k in cols0:
        assert np.array_equal(cols[k], cols0[k]), k
    assert st0['k_tags_ns'] == 0


def test_cs_long_and_eqx(world):
    paf, sam, cols, _ = world.run(CS_LONG | EQX)
    paf0, sam0, cols0, _ = world.run(0)
    check_paf(world, paf, long_form=True, eqx=True, want_md=False)
    check_sam(world, sam, long_form=True, eqx=True, want_md=False)
    assert 'MD:Z:' not in paf + sam

    def collapse_text(m):
        return m.group(1) + cigar_text(collapse_eqx(parse_cigar(m.group(2))))
    back = re.sub(r'(\tcg:Z:)([0-9MIDX=]+)', collapse_text, strip_tags(paf))
    assert back == paf0                           # every other field of every line, and the collapsed CIGARs
    sam_back = []
    for line in strip_tags(sam).splitlines(keepends=True):
        f = line.split('\t')
        if f[5] != '*':
            assert 'M' not in f[5]
            lead, trail = re.match(r'^(\d+[SH])?', f[5]).group(0), re.search(r'(\d+[SH])?$', f[5]).group(0)
            body = cigar_text(collapse_eqx([c for c in parse_cigar(f[5]) if c & 15 not in (4, 5)]))
            f[5] = lead + body + trail
        sam_back.append('\t'.join(f))
    assert ''.join(sam_back) == sam0
    for k in cols0:
        assert np.array_equal(cols[k], cols0[k]), k


def test_columns_only_call_ignores_the_tags(world):
    from megapath_nano_amd import mapper
    _, _, cols0, _ = world.run(0)
    opt = mapper.default_opt(out_sam=0, out_tags=CS | MD | EQX)
    text, cols = mapper.map_batch_ex(world.idx, opt, world.packed, want_paf=False, want_cols=True)
    st = mapper.last_stats()
    assert text is None
    for k in cols0:
        assert np.array_equal(cols[k], cols0[k]), k
    assert st['k_tags_ns'] == 0 and st['k_finish_ns'] > 0, (st['k_tags_ns'], st['k_finish_ns'])


def test_mapping_only_call_ignores_the_tags(world):
    from megapath_nano_amd import mapper
    a = mapper.map_batch_full(world.idx, mapper.default_opt(with_cigar=0, out_sam=2, out_tags=CS | MD | EQX), world.packed, want_paf=True)
    b = mapper.map_batch_full(world.idx, mapper.default_opt(with_cigar=0, out_sam=2), world.packed, want_paf=True)
    assert a[0] == b[0] and a[1] == b[1] and 'cs:Z' not in a[0] + a[1]


def test_split_parts_closed_before_finish(world):
    from megapath_nano_amd import _ffi, mapper
    cut = [0, 2, 4, len(world.gen)]
    opt = mapper.default_opt(out_sam=2, out_tags=CS | MD)
    # three parts held resident, one call
    parts = [mapper.Index(world.gen[a:b]) for a, b in zip(cut, cut[1:])]
    h = mapper.Hits(world.packed)
    h.add_parts(parts, opt)
    want_paf, want_sam, _ = h.finish(opt, want_paf=True, want_cols=False)
    h.close()
    for p in parts:
        p.close()
    # streamed: each part is destroyed before the next is built and long before the text is written
    h = mapper.Hits(world.packed)
    for a, b in zip(cut, cut[1:]):
        part = mapper.Index(world.gen[a:b])
        h.add_part(part, opt)
        part.close()
    with pytest.raises(_ffi.MpnError, match='mpn_hits_export'):
        h.export(0, world.packed.n)
    for bad in (CS | MD | EQX, CS_LONG | MD, EQX):
        with pytest.raises(_ffi.MpnError, match='do not carry'):
            h.finish(mapper.default_opt(out_sam=2, out_tags=bad), want_paf=True, want_cols=False)
    with pytest.raises(_ffi.MpnError, match='out_tags differs'):
        extra = mapper.Index(world.gen[:1])
        try:
            h.add_part(extra, mapper.default_opt(out_sam=2, out_tags=CS))
        finally:
            extra.close()
    got_paf, got_sam, _ = h.finish(opt, want_paf=True, want_cols=False)
    h.close()
    assert got_paf == want_paf and got_sam == want_sam
    recs = check_paf(world, got_paf)
    check_sam(world, got_sam)
    assert len(recs) > 40
    # an accumulator that was told there would be no text computes nothing
    h = mapper.Hits(world.packed, want_text=False)
    part = mapper.Index(world.gen[:2])
    h.add_part(part, opt)
    assert mapper.last_stats()['k_tags_ns'] == 0
    part.close()
    h.close()


_CHILD = r'''
import json, sys
import numpy as np
root, tests, out = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path.insert(0, root); sys.path.insert(0, tests)
from map_cases import hard_reads, small_world
from megapath_nano_amd import mapper
gen, reads = small_world()
reads = reads + hard_reads(gen)
idx = mapper.Index(gen)
packed = mapper.PackedReads([r['name'] for r in reads], [r['seq'] for r in reads])
paf, sam, _ = mapper.map_batch_full(idx, mapper.default_opt(out_sam=2, out_tags=5), packed, want_paf=True, want_cols=False)
json.dump(dict(paf=paf, sam=sam, stats=mapper.last_stats()), open(out, 'w'))
idx.close()
print('CHILD_OK')
'''


_FAULT_RCS = (124, 134, 137, 139)
_faulted = []   # set once a child has died on a signal, a fault status or the time limit: no later child is started


def run_child(tmp_path, env, timeout=600):
    """Map in a fresh process with `env` added to the environment, under the guard of tests/test_dispatch_paths_gpu.py's
    run_child: after a child that faulted, timed out or died on a signal, nothing more is started on the GPU."""
    if _faulted:
        pytest.fail('not started: an earlier child faulted (' + _faulted[0] + ')')
    out = str(tmp_path / 'res.json')
    what = ' '.join(f'{k}={v}' for k, v in env.items())
    try:
        p = subprocess.run([sys.executable, '-c', _CHILD, ROOT, os.path.join(ROOT, 'tests'), out], env=dict(os.environ, **env), capture_output=True,
                           text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        _faulted.append(f'{what}: time limit')
        err = e.stderr.decode(errors='replace') if isinstance(e.stderr, bytes) else (e.stderr or '')
        pytest.fail(f'child [{what}] exceeded {timeout} s; stderr tail:\n{err[-3000:]}')
    if p.returncode < 0 or p.returncode in _FAULT_RCS:
        _faulted.append(f'{what}: exit status {p.returncode}')
        pytest.fail(f'child [{what}] ended with status {p.returncode}; stderr tail:\n{p.stderr[-3000:]}')
    assert p.returncode == 0 and 'CHILD_OK' in p.stdout, f'child [{what}] failed ({p.returncode}); stderr tail:\n{p.stderr[-3000:]}'
    return out


@pytest.mark.parametrize('env', [{'MPN_HOST_HITS': '1'}, {'MPN_TILED': '0'}], ids=['host_hits', 'band_kernel'])
def test_dispatch_variants(world, tmp_path, env):
    """the knobs are read once per process (tests/test_dispatch_paths_gpu.py): each setting maps in a child of its own"""
    out = run_child(tmp_path, env)
    res = json.load(open(out))
    if 'MPN_HOST_HITS' in env:
        assert res['stats']['reads_hits_on_host'] > 0
    else:
        assert res['stats']['tile_windows'] == 0
    recs = check_paf(world, res['paf'])
    srecs = check_sam(world, res['sam'])
    assert_inputs_cover(recs, srecs)
    paf, sam, _, _ = world.run(CS | MD)
    assert res['paf'] == paf and res['sam'] == sam
