"""GPU parity tests (-m gpu) of the pipelined tiled extension DP (ext_dp_tile_kernel<S, NW>: a window's tiles on the waves of one
workgroup, the first row of a tile handed over through an LDS ring) against the oracle's mmo_extd2, bit for bit on scores, end
points and CIGARs.  Every tiled class runs in a subprocess of its own (MPN_TILE_CLASS is read once per process), with
force_kernel 6 (tiled where eligible), 0 (automatic) and 5 (band kernel) on the same pairs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APPROX, RIGHT, EXTZ, REV = 0x02, 0x08, 0x40, 0x80
CLASSES = {1: 4, 2: 8, 3: 4}   # pipelined tiled class -> rows per lane S (plan_kernels.h tile_class_s)


def _pairs(seed, shapes, tail=False, ambig=False):
    from test_ext_dp_gpu import mutate
    rng = np.random.default_rng(seed)
    qs, ts = [], []
    for tlen, qextra in shapes:
        t = rng.integers(0, 4, size=tlen).astype(np.uint8)
        q = mutate(rng, t, 0.1)
        if qextra is not None:   # pin the query length (padding with unrelated bases, or cutting)
            n = max(1, tlen + qextra)
            q = q[:n] if len(q) >= n else np.concatenate([q, rng.integers(0, 4, size=n - len(q)).astype(np.uint8)])
        if tail:
            q = np.concatenate([q, rng.integers(0, 4, size=int(rng.integers(300, 900))).astype(np.uint8)])
            t = np.concatenate([t, rng.integers(0, 4, size=int(rng.integers(300, 900))).astype(np.uint8)])
        if ambig:
            q[rng.integers(0, len(q), size=max(1, len(q) // 50))] = 4
            t[rng.integers(0, len(t), size=max(1, len(t) // 60))] = 4
        qs.append(q)
        ts.append(t)
    return qs, ts


def _cases(S):
    """(name, qs, ts, w, zdrop, end_bonus, flag, kernels) for the rows-per-lane S."""
    R = 64 * S
    out = []
    # 1 to 64 tiles; tlen at R - 1, R, R + 1 and at tile multiples (up to 8191 anti-diagonal-bounded for the exact variants)
    edges = sorted({n for k in (1, 2, 3, 5, 8) for n in (k * R - 1, k * R, k * R + 1) if 0 < n <= 8191})
    qs, ts = _pairs(100 + S, [(n, 0) for n in edges])
    out.append(('edges_approx', qs, ts, 751, 400, -1, APPROX, [6, 0]))
    qs2, ts2 = _pairs(200 + S, [(n, None) for n in edges if n <= 6900])
    out.append(('edges_extz', qs2, ts2, 751, 400, -1, EXTZ, [6, 0]))
    out.append(('edges_rev', qs2, ts2, 751, 200, 30, EXTZ | RIGHT | REV, [6, 0]))
    out.append(('edges_global', qs2, ts2, 300, 400, -1, 0, [6]))
    qs, ts = _pairs(300 + S, [(min(64 * R, 8191), 0), (min(40 * R, 8191), 3)])
    out.append(('many_tiles', qs, ts, 200, 400, -1, APPROX, [6]))
    # n_r up to the cap of the exact variants (qlen + tlen - 1 <= 14000), z-drop inside a late tile (tail), reach_end + end bonus
    qs, ts = _pairs(400 + S, [(6900, 0), (7000, 1)])
    out.append(('cap_extz', qs, ts, 751, 400, 10, EXTZ, [6]))
    qs, ts = _pairs(500 + S, [(3 * R + 40, None), (6 * R + 3, None)], tail=True)
    out.append(('late_zdrop', qs, ts, 751, 400, -1, EXTZ, [6, 0]))
    out.append(('late_zdrop_rev', qs, ts, 500, 150, 5, EXTZ | RIGHT | REV, [6, 0]))
    # the band leaving the matrix (lopsided windows), ambiguous bases, low-complexity ties
    rng = np.random.default_rng(600 + S)
    lq, lt = [], []
    for qlen, tlen in ((5000, 1300), (1300, 5000), (600, 1500)):
        t = rng.integers(0, 4, size=tlen).astype(np.uint8)
        q = rng.integers(0, 4, size=qlen).astype(np.uint8)
        n = min(qlen, tlen)
        q[:n] = np.where(rng.random(n) < 0.9, t[:n], q[:n])
        lq.append(q)
        lt.append(t)
    out.append(('band_leaves', lq, lt, 751, 400, -1, EXTZ, [6]))
    qs, ts = _pairs(700 + S, [(1800, None), (2600, None)], ambig=True)
    out.append(('ambig_extz', qs, ts, 751, 100, 5, EXTZ | RIGHT | REV, [6]))
    out.append(('ambig_approx', qs, ts, 900, 400, -1, APPROX, [6]))
    lq = [np.array(([0, 1] * 1300)[:n], dtype=np.uint8) for n in (1300, 2200)] + [np.zeros(1500, dtype=np.uint8)]
    lt = [np.array(([0, 1] * 1400)[:n + 37], dtype=np.uint8) for n in (1300, 2200)] + [np.zeros(1530, dtype=np.uint8)]
    for flag in (EXTZ, EXTZ | RIGHT | REV, 0, APPROX):
        out.append((f'ties_{flag}', lq, lt, 500, 400, -1, flag, [6]))
    # the ~5000 x 5000, w = 751 end extensions that the band kernel took before
    qs, ts = _pairs(800 + S, [(4850, None), (5000, None), (5000, None)], tail=True)
    out.append(('band82_extz', qs, ts, 751, 400, -1, EXTZ, [6, 0, 5]))
    out.append(('band82_rev', qs, ts, 751, 400, -1, EXTZ | RIGHT | REV, [6, 0, 5]))
    # one batch that mixes sizes and bands: several tiled lists (and the one-wave list for the wide band) in one call
    qs, ts = _pairs(900 + S, [(300, 0), (1600, 0), (3000, 2), (5000, 1), (1100, 0)])
    out.append(('mixed', qs, ts, [751, 751, 750, 751, 3000], 400, -1, APPROX, [6, 0]))
    return out


def _run_class(cls):
    code = f'''
import json, sys
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
import test_ext_tile_pipeline_gpu as T
print(json.dumps(T._check_all({CLASSES[cls]})))
'''
    env = dict(os.environ, MPN_TILE_CLASS=str(cls))
    p = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def _check_all(S):
    from megapath_nano_amd import mapper
    from oracle import mm2_bindings as mb
    opt = mapper.default_opt()
    bad, tiled = [], 0
    for name, qs, ts, w, zdrop, eb, flag, kernels in _cases(S):
        ws = np.broadcast_to(np.asarray(w), (len(qs),))
        want = [mb.extd2(q, t, w=int(wi), zdrop=zdrop, end_bonus=eb, flag=flag) for q, t, wi in zip(qs, ts, ws)]
        keys = ['zdropped', 'n_cigar', 'cigar', 'score'] if flag & APPROX else \
            ['max', 'zdropped', 'max_q', 'max_t', 'mqe', 'mqe_t', 'score', 'reach_end', 'n_cigar', 'cigar']
        for k in kernels:
            names = ('tile_windows_s4_nw8', 'tile_windows_s8_nw4', 'tile_windows_s4_nw16')
            before = mapper.last_stats()
            got = mapper.ext_dp_batch(opt, qs, ts, w, zdrop, eb, flag, force_kernel=k)
            after = mapper.last_stats()
            tiled += sum(after[n] - before[n] for n in names)
            assert after['tile_wait_giveups'] == before['tile_wait_giveups']
            for i, (g, e) in enumerate(zip(got, want)):
                for key in keys:
                    if key == 'score' and e['zdropped']:
                        continue
                    if key in ('mqe', 'score') and g[key] < -10**8 and e[key] < -10**8:
                        continue
                    if g[key] != e[key]:
                        bad.append([name, k, i, len(qs[i]), len(ts[i]), key])
                        break
    return {'bad': bad[:20], 'n_bad': len(bad), 'pipelined_windows': tiled}


@pytest.mark.parametrize('cls', sorted(CLASSES))
def test_pipelined_tiles_match_oracle(libmpn, oracle_built, cls):
    r = _run_class(cls)
    assert r['n_bad'] == 0, r
    assert r['pipelined_windows'] > 0, r   # the class was really taken
