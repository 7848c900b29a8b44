"""GPU parity tests (-m gpu) of the wave-per-window traceback (ext_bt_wave_kernel) and z-drop test (ext_ztest_wave_kernel) at the
DP stage entry: on seeded pairs `MPN_EXT_WALK=wave` (every window through the wave kernels) must give, bit for bit, what
`MPN_EXT_WALK=lane` (a lane per window) gives and what the oracle's mmo_extd2 gives, on every layout of the direction matrix:
layout 3 (tiled strips, force_kernel 6, tile classes <4, 8> and <16, 1>), layout 2 (band kernel, 5), layout 0 (workgroup
kernel, 1 and 3) and layout 1 (strip kernel, 4).  The switch is read once per process: every (setting, tile class) runs in a
subprocess of its own, one at a time, and reports the walk_wave_windows counter so that a run that silently took the lane
kernel fails."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APPROX, RIGHT, EXTZ, REV = 0x02, 0x08, 0x40, 0x80
TILE_CLASSES = {1: 4, 0: 16}   # MPN_TILE_CLASS -> rows per lane S: <4, 8> and <16, 1>


def _long_gap_pairs(seed):
    """gaps longer than a 64-cell patch, in both directions, alone and several per window"""
    from test_ext_dp_gpu import mutate
    rng = np.random.default_rng(seed)
    qs, ts = [], []
    for L, dels, inss in ((1500, (150,), ()), (1500, (), (200,)), (2600, (70, 300), (130,)), (5000, (500,), (90, 260))):
        t = rng.integers(0, 4, size=L).astype(np.uint8)
        q = list(mutate(rng, t, 0.08))
        cuts = sorted(int(x) for x in rng.integers(200, len(q) - 700, size=len(dels) + len(inss)))
        for k, n in enumerate(dels):
            del q[cuts[k] + 400 * k: cuts[k] + 400 * k + n]
        for k, n in enumerate(inss):
            at = min(cuts[len(dels) + k], len(q) - 50)
            q[at:at] = rng.integers(0, 4, size=n).tolist()
        qs.append(np.array(q, dtype=np.uint8))
        ts.append(t)
    return qs, ts


def _thin_pairs(seed):
    """the smallest windows (one row, one column) and paths that are one long insertion or one long deletion"""
    rng = np.random.default_rng(seed)
    shapes = ((1, 1), (1, 2), (2, 1), (300, 1), (1, 300), (700, 2), (2, 700), (90, 3), (3, 90), (1, 65), (65, 1))
    qs = [rng.integers(0, 4, size=ql).astype(np.uint8) for ql, _ in shapes]
    ts = [rng.integers(0, 4, size=tl).astype(np.uint8) for _, tl in shapes]
    return qs, ts


def _cases(S):
    """(name, qs, ts, w, zdrop, end_bonus, flag, kernels)"""
    import test_ext_tile_pipeline_gpu as T
    from test_ext_dp_gpu import make_pairs
    # layout 3: the tile pipeline's shapes (1 to 64 tiles, tlen at k R - 1, k R, k R + 1, lopsided windows whose path runs along the
    # band edge, ambiguous bases, low-complexity ties, right-aligned + reversed CIGARs, the ~5000 x 5000 w = 751 extensions with
    # unrelated tails), every one on the tiled kernel only
    out = [(n, qs, ts, w, zd, eb, fl, [6]) for n, qs, ts, w, zd, eb, fl, _ in T._cases(S)]
    by = {c[0]: c for c in out}
    # layouts 2 and 0 on the long shapes: band kernel and workgroup kernels
    n, qs, ts, w, zd, eb, fl, _ = by['band82_extz']
    out.append(('band82_extz_l2_l0', qs, ts, w, zd, eb, fl, [5, 3]))
    n, qs, ts, w, zd, eb, fl, _ = by['band82_rev']
    out.append(('band82_rev_l2_l0', qs, ts, w, zd, eb, fl, [5, 1]))
    n, qs, ts, w, zd, eb, fl, _ = by['band_leaves']
    out.append(('band_leaves_l2_l0', qs, ts, w, zd, eb, fl, [5, 1, 3]))
    out.append(('band_leaves_approx', qs, ts, 4000, zd, eb, APPROX, [6, 5, 1]))
    for fl in (EXTZ, EXTZ | RIGHT | REV, 0, APPROX):
        n, qs, ts, w, zd, eb, _, _ = by[f'ties_{fl}']
        out.append((f'ties_{fl}_l2_l0', qs, ts, w, zd, eb, fl, [5, 1]))
    n, qs, ts, w, zd, eb, fl, _ = by['ambig_extz']
    out.append(('ambig_extz_l2_l0', qs, ts, w, zd, eb, fl, [5, 1, 3]))
    # gaps longer than a patch, every layout (the strip kernel takes what is eligible for it, the band kernel the rest)
    qs, ts = _long_gap_pairs(31 + S)
    for fl in (APPROX, 0, EXTZ | RIGHT | REV):
        out.append((f'long_gaps_{fl}', qs, ts, 751, 400, -1, fl, [6, 5, 1, 3, 4]))
    # one row, one column, one long insertion / deletion
    qs, ts = _thin_pairs(41 + S)
    for fl in (APPROX, 0, EXTZ, EXTZ | RIGHT | REV):
        out.append((f'thin_{fl}', qs, ts, 751, 400, -1, fl, [6, 5, 1, 3, 4, 0]))
    # layout 1: every strip height, the class edges, right-aligned gaps, ambiguous bases
    qs, ts = make_pairs(51, [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 700, 1000, 1023, 1024])
    for fl in (APPROX, APPROX | RIGHT):
        out.append((f'strip_{fl}', qs, ts, 3000, 400, -1, fl, [4, 1, 5]))
    qs, ts = make_pairs(52, [60, 130, 260, 500, 900], tail=True)
    qs, ts = [q[:1000] for q in qs], [t[:1024] for t in ts]
    for fl in (EXTZ, EXTZ | RIGHT | REV):
        out.append((f'strip_tail_{fl}', qs, ts, 3000, 100, -1, fl, [4, 1, 3]))
    qs, ts = make_pairs(53, [220, 480, 900], ambig=True, big_indel=True)
    out.append(('strip_ambig', qs, ts, 3000, 400, -1, APPROX, [4, 5, 1]))
    # narrow bands: the path runs along the band edge on the band and workgroup layouts
    qs, ts = make_pairs(54, [600, 1500, 2600])
    out.append(('narrow_global', qs, ts, 100, 400, -1, 0, [1, 3, 5, 6]))
    out.append(('narrow_approx', qs, ts, 20, 400, -1, APPROX, [1, 3, 5, 6]))
    return out


def _check_all(S):
    """runs in the subprocess: every case against the oracle; a digest per (case, kernel) for the comparison between settings"""
    from megapath_nano_amd import mapper
    from oracle import mm2_bindings as mb
    opt = mapper.default_opt()
    bad, digests = [], {}
    before = mapper.last_stats()
    for name, qs, ts, w, zdrop, eb, flag, kernels in _cases(S):
        ws = np.broadcast_to(np.asarray(w), (len(qs),))
        want = [mb.extd2(q, t, w=int(wi), zdrop=zdrop, end_bonus=eb, flag=flag) for q, t, wi in zip(qs, ts, ws)]
        keys = ['zdropped', 'n_cigar', 'cigar', 'score'] if flag & APPROX else \
            ['max', 'zdropped', 'max_q', 'max_t', 'mqe', 'mqe_t', 'score', 'reach_end', 'n_cigar', 'cigar']
        for k in kernels:
            got = mapper.ext_dp_batch(opt, qs, ts, w, zdrop, eb, flag, force_kernel=k)
            h = hashlib.sha256()
            for i, (g, e) in enumerate(zip(got, want)):
                h.update(json.dumps([g[key] for key in ('max', 'zdropped', 'max_q', 'max_t', 'mqe', 'mqe_t', 'score', 'reach_end', 'n_cigar', 'cigar')]).encode())
                for key in keys:
                    if key == 'score' and e['zdropped']:
                        continue
                    if key in ('mqe', 'score') and g[key] < -10**8 and e[key] < -10**8:
                        continue
                    if g[key] != e[key]:
                        bad.append([name, k, i, len(qs[i]), len(ts[i]), key])
                        break
            digests[f'{name}/{k}'] = h.hexdigest()
    after = mapper.last_stats()
    return {'bad': bad[:20], 'n_bad': len(bad), 'digests': digests, 'n_windows': int(after['dp_jobs'] - before['dp_jobs']),
            'walk_wave_windows': int(after['walk_wave_windows'] - before['walk_wave_windows'])}


def _run(cls, walk):
    code = f'''
import json, sys
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
import test_ext_walk_wave_gpu as T
print(json.dumps(T._check_all({TILE_CLASSES[cls]})))
'''
    env = dict(os.environ, MPN_TILE_CLASS=str(cls), MPN_EXT_WALK=walk)
    p = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert p.returncode == 0, (walk, p.returncode, p.stderr[-3000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize('cls', sorted(TILE_CLASSES, reverse=True))
def test_wave_walk_matches_lane_walk_and_oracle(libmpn, oracle_built, cls):
    lane = _run(cls, 'lane')
    wave = _run(cls, 'wave')
    print('windows', wave['n_windows'], 'through the wave kernel', wave['walk_wave_windows'], 'under lane', lane['walk_wave_windows'])
    assert lane['n_bad'] == 0, lane['bad']
    assert wave['n_bad'] == 0, wave['bad']
    assert lane['walk_wave_windows'] == 0, lane['walk_wave_windows']
    # every window of every case took the wave kernel
    assert wave['walk_wave_windows'] == wave['n_windows'] > 0, (wave['walk_wave_windows'], wave['n_windows'])
    assert lane['digests'].keys() == wave['digests'].keys()
    differ = [k for k in lane['digests'] if lane['digests'][k] != wave['digests'][k]]
    assert not differ, differ
