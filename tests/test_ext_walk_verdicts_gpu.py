"""GPU parity test (-m gpu) of the z-drop verdicts of the wave-per-window walk kernels through the whole mapper: the PAF text and
the 13 hit columns under MPN_EXT_WALK = lane, wave and auto must be equal to each other, and the PAF equal to the oracle's
(oracle/mm2_bindings.py), on a world made for long gap fills of which some fail the test:

* the targets are mosaic copies of the genomes the reads come from: conserved blocks (anchors) alternate with blocks of 1.2-2.8 kb
  that diverged by ~22 % substitutions (no anchors), so a read's hit is a chain of sparse anchors with fills of 1-3 kb between
  them -- windows with more than 1024 target rows, which the dispatcher sends to the long lists (tiled strips) and MPN_EXT_WALK=auto
  to the wave kernels;
* some reads have several hundred bases inside such a block replaced by unrelated sequence (plain z-drop: the hit is split);
* some carry a reverse-complemented segment inside such a block (the inversion probe);
* map_cases.hard_reads (inverted 1.2 kb segment, long deletions, N runs) are mapped against an undiverged genome beside them.

The switch is read once per process: every setting runs in a subprocess of its own, one at a time.  The test is not vacuous:
second_pass_jobs > 0 under every setting, walk_wave_windows > 0 and walk_wave_failed > 0 (fills that the wave z-drop test failed) under auto and wave (0 under lane), and a read
comes out split."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mosaic_world(seed=77):
    """-> (targets [(name, ASCII array)], reads [dict(name, seq)])"""
    from map_cases import hard_reads
    from megapath_nano_amd import synth
    rng = np.random.default_rng(seed)
    comp = synth.COMP
    sources = [synth.random_genome(rng, 90000, gc=0.5) for _ in range(2)]
    targets, blocks = [], []
    for gi, g in enumerate(sources):
        t = g.copy()
        pos, div = 400, []
        while pos + 3400 < len(g):
            n = int(rng.integers(1200, 2800))
            sub = np.flatnonzero(rng.random(n) < 0.22) + pos
            t[sub] = synth.ALPHA[(np.searchsorted(synth.ALPHA, t[sub]) + rng.integers(1, 4, size=len(sub))) % 4]
            div.append((pos, pos + n))
            pos += n + int(rng.integers(350, 600))
        targets.append((f'NZ_MOS{gi:05d}.1', t))
        blocks.append(div)
    plain = synth.make_genomes(seed + 1, 4, 100000, strain_pairs=1)   # hard_reads need three genomes
    targets += plain
    reads = []

    def add(name, parts):
        seq = synth.ont_errors(rng, np.concatenate(parts), 0.02, 0.01, 0.02)
        reads.append(dict(name=name, seq=seq, genome=-1, start=0, end=0, strand='+'))

    junk = lambda n: synth.ALPHA[rng.integers(0, 4, size=n)]  # noqa: E731
    for gi, g in enumerate(sources):
        div = blocks[gi]
        for k in range(7):    # plain reads over several diverged blocks: long fills that pass the test
            s = int(rng.integers(0, len(g) - 16000))
            add(f'mos{gi}_{k}', [g[s:s + int(rng.integers(8000, 15000))]])
        for k in range(5):    # unrelated sequence in place of the middle of a diverged block
            b0, b1 = div[int(rng.integers(2, len(div) - 3))]
            n = int(rng.integers(400, 900))
            mid = (b0 + b1 - n) // 2
            add(f'junk{gi}_{k}', [g[b0 - 5000:mid], junk(n), g[mid + n:b1 + 5000]])
        for k in range(5):    # a reverse-complemented segment inside a diverged block
            b0, b1 = div[int(rng.integers(2, len(div) - 3))]
            a, b = b0 + (b1 - b0) // 4, b1 - (b1 - b0) // 4
            add(f'inv{gi}_{k}', [g[b0 - 5000:a], comp[g[a:b][::-1]], g[b:b1 + 5000]])
    reads += hard_reads(plain, seed=seed + 2)
    return targets, reads


def oracle_paf(targets, reads, best_n=5, pri_ratio=0.8):
    from oracle import mm2_bindings as mb
    oidx = mb.Index(targets)
    oopt = mb.default_opt(best_n=best_n, pri_ratio=pri_ratio)
    out = ''.join(mb.map_read(oidx, oopt, r['name'], r['seq'])[2] for r in reads)
    oidx.close()
    return out


def _map_all():
    """runs in the subprocess -> PAF text, a digest of the hit columns, the counters"""
    from megapath_nano_amd import mapper
    targets, reads = mosaic_world()
    gidx = mapper.Index(targets)
    gopt = mapper.default_opt(best_n=5, pri_ratio=0.8)
    packed = mapper.PackedReads([r['name'] for r in reads], [r['seq'] for r in reads])
    before = mapper.last_stats()
    paf, cols = mapper.map_batch_ex(gidx, gopt, packed, want_paf=True, want_cols=True)
    after = mapper.last_stats()
    h = hashlib.sha256()
    for k in sorted(cols):
        h.update(k.encode())
        h.update(np.ascontiguousarray(cols[k]).tobytes())
    gidx.close()
    return {'paf': paf, 'cols': h.hexdigest(), 'n_cols': len(cols), 'n_rows': int(len(next(iter(cols.values())))),
            'stats': {k: int(after[k] - before[k]) for k in ('second_pass_jobs', 'walk_wave_windows', 'walk_wave_failed', 'tile_windows', 'dp_jobs')}}


def _run(walk):
    code = f'''
import json, sys
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
import test_ext_walk_verdicts_gpu as T
print(json.dumps(T._map_all()))
'''
    env = dict(os.environ, MPN_EXT_WALK=walk)
    p = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, (walk, p.returncode, p.stderr[-3000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_verdicts_equal_between_walks_and_oracle(libmpn, oracle_built):
    targets, reads = mosaic_world()
    want = oracle_paf(targets, reads)
    split = {l.split('\t')[0] for l in want.splitlines() if 'zd:i:' in l}
    assert split, 'no read comes out split'
    assert any('tp:A:I' in l for l in want.splitlines()), 'no inversion line'
    runs = {walk: _run(walk) for walk in ('lane', 'wave', 'auto')}
    for walk, r in runs.items():
        print(walk, r['stats'], 'rows', r['n_rows'])
        assert r['paf'] == want, walk
        assert r['n_cols'] >= 13 and r['cols'] == runs['lane']['cols'], walk
        assert r['stats']['second_pass_jobs'] > 0, (walk, r['stats'])
    assert runs['lane']['stats']['walk_wave_windows'] == 0
    assert runs['auto']['stats']['walk_wave_windows'] > 0 and runs['wave']['stats']['walk_wave_windows'] > 0
    assert runs['wave']['stats']['walk_wave_windows'] > runs['auto']['stats']['walk_wave_windows']
    # under auto failing fills reach the wave z-drop test (they are long-list windows), under wave every failing fill does
    assert runs['lane']['stats']['walk_wave_failed'] == 0
    assert runs['auto']['stats']['walk_wave_failed'] > 0, runs['auto']['stats']
    assert runs['wave']['stats']['walk_wave_failed'] >= runs['auto']['stats']['walk_wave_failed']
