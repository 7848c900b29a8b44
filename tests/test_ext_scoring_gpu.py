"""GPU parity tests (-m gpu) of the extension-DP kernels under scoring sets other than the map-ont default: mapper.ext_dp_batch
against the oracle's mmo_extd2 (int32 states, no width limits), bit-exact on scores, end points and CIGAR, with the comparison
rule of test_ext_dp_gpu.check.

The kernels are written around the scoring values: the strip, pair and tile cells fold 8 * score + rank + 128 into a byte and the gap
costs into biased 16-bit halves, and the exact variants keep H of a cell in a 16-bit field of an LDS word.  The sets below sit at the
ends of those ranges (ext_strip_scores_ok), on both sides of ext_strip_exact_ok's boundary and on both sides of the tiled exact
variant's H range (ext_tile_exact_ok).  Every set is one ksw2's own int8 states are defined on: a + max(q + e, q2 + e2) <= 127.
'no-mismatch' is deliberately outside -sc_mis <= 2 (q + e): ksw2 returns the empty result there, and so must every kernel."""
import numpy as np
import pytest

from test_ext_dp_gpu import APPROX, EXTZ, REV, RIGHT, make_pairs, mutate

pytestmark = pytest.mark.gpu

SETS = {
    'sr': dict(a=2, b=8, q=12, e=2, q2=32, e2=1),            # strip cell, wide gap costs
    'asm20': dict(a=1, b=4, q=6, e=2, q2=26, e2=1),          # a = 1
    'asm10': dict(a=1, b=9, q=16, e=2, q2=41, e2=1),
    'asm5': dict(a=1, b=19, q=39, e=3, q2=81, e2=1),         # b > 16: outside ext_strip_scores_ok, the band / workgroup kernels carry everything
    'A5': dict(a=5, b=4, q=8, e=2, q2=24, e2=1),             # H range
    'A15': dict(a=15, b=16, q=20, e=6, q2=60, e2=3),         # byte table at both ends: 8 * 15 + 4 + 128 = 252, 8 * (-16) + 128 = 0
    'single': dict(a=2, b=4, q=4, e=2, q2=4, e2=2),          # e == e2, long_thres = 0
    'swapped': dict(a=2, b=4, q=24, e=1, q2=4, e2=2),        # the q2 + e2 < q + e swap
    'big-e': dict(a=2, b=4, q=10, e=5, q2=10, e2=5),         # low side of H
    'no-mismatch': dict(a=2, b=40, q=4, e=2, q2=24, e2=1),   # every kernel returns the empty result, like ksw2
    # H range only
    'A4': dict(a=4, b=4, q=4, e=2, q2=24, e2=1),
    'A5d': dict(a=5, b=4, q=4, e=2, q2=24, e2=1),
    'A8': dict(a=8, b=4, q=4, e=2, q2=24, e2=1),
}
TABLE = ['sr', 'asm20', 'asm10', 'asm5', 'A5', 'A15', 'single', 'swapped', 'big-e', 'no-mismatch']
WIDE = ('sr', 'A5', 'A15', 'swapped', 'single')   # the sets that run the longer tiled lists


def test_sets_are_in_ksw2_domain():
    for name, s in SETS.items():
        assert all(-128 <= v <= 127 for v in s.values()), name
        assert s['a'] + max(s['q'] + s['e'], s['q2'] + s['e2']) <= 127, name
        assert (s['b'] <= 2 * (s['q'] + s['e'])) == (name != 'no-mismatch'), name


def oracle(name, qs, ts, w, zdrop, end_bonus, flag, sc_ambi=1):
    from oracle import mm2_bindings as mb
    s = SETS[name]
    return [mb.extd2(q, t, sc_mch=s['a'], sc_mis=-s['b'], sc_n=-sc_ambi, q=s['q'], e=s['e'], q2=s['q2'], e2=s['e2'], w=w, zdrop=zdrop,
                     end_bonus=end_bonus, flag=flag) for q, t in zip(qs, ts)]


def check(name, qs, ts, w, zdrop, end_bonus, flag, kernels, sc_ambi=1):
    """ext_dp_batch under the set `name` on every kernel of `kernels` == the oracle (keys and exemptions of test_ext_dp_gpu.check)."""
    from megapath_nano_amd import mapper
    opt = mapper.default_opt(sc_ambi=sc_ambi, **SETS[name])
    want = oracle(name, qs, ts, w, zdrop, end_bonus, flag, sc_ambi)
    for k in kernels:
        got = mapper.ext_dp_batch(opt, qs, ts, w, zdrop, end_bonus, flag, force_kernel=k)
        for i, (g, e) in enumerate(zip(got, want)):
            keys = ['zdropped', 'n_cigar', 'cigar', 'score'] if flag & APPROX else \
                ['max', 'zdropped', 'max_q', 'max_t', 'mqe', 'mqe_t', 'score', 'reach_end', 'n_cigar', 'cigar']
            for key in keys:
                if key == 'score' and e['zdropped']:
                    continue
                if key in ('mqe', 'score') and g[key] < -10**8 and e[key] < -10**8:
                    continue  # both 'never set' (the two sides use different -inf constants)
                assert g[key] == e[key], (name, k, flag, w, zdrop, i, len(qs[i]), len(ts[i]), key,
                                          g[key] if key != 'cigar' else g[key][:6], e[key] if key != 'cigar' else e[key][:6])
    return want


@pytest.fixture(scope='module')
def built(libmpn, oracle_built):
    return True


def low_complexity(ns, tail):
    qs = [np.array(([0, 1] * (n // 2 + 1))[:n], dtype=np.uint8) for n in ns] + [np.zeros(ns[0] + 70, dtype=np.uint8)]
    ts = [np.array(([0, 1] * n)[:n * 3 // 2 if tail is None else n + tail], dtype=np.uint8) for n in ns] + \
        [np.zeros(ns[0] + (150 if tail is None else 100), dtype=np.uint8)]
    return qs, ts


def lopsided(seed, shapes, ident):
    rng = np.random.default_rng(seed)
    qs, ts = [], []
    for qlen, tlen in shapes:
        t = rng.integers(0, 4, size=tlen).astype(np.uint8)
        q = rng.integers(0, 4, size=qlen).astype(np.uint8)
        n = min(qlen, tlen)
        q[:n] = np.where(rng.random(n) < ident, t[:n], q[:n])   # a homologous prefix, the rest unrelated
        qs.append(q)
        ts.append(t)
    return qs, ts


@pytest.mark.parametrize('name', TABLE)
def test_gap_fills(built, name):
    """Approximate-maximum gap fills, left- and right-aligned, at sizes that cross the lane-group and strip-height classes; the pairs of
    one list are neighbours, so the paired strip (two windows per register) sees two different halves.  Ambiguous bases scored 0, 1
    and 3; a big indel.  Kernel 4 takes the strip where the band does not clip (w >= the window), kernel 6 the tiles."""
    qs, ts = make_pairs(1, [30, 64, 65, 200, 256, 257, 400, 511, 512, 513, 700, 1024, 1025])
    check(name, qs, ts, 751, 400, -1, APPROX, [0, 1, 3, 4, 5, 6])
    check(name, qs, ts, 751, 400, -1, APPROX | RIGHT, [1, 4, 5])
    check(name, qs, ts, 2000, 400, -1, APPROX, [4, 0])            # nothing clips: strips up to 1024 rows, tiles beyond
    qs, ts = make_pairs(11, [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 512, 513, 600, 700])
    check(name, qs, ts, 751, 400, -1, APPROX, [1, 4, 5])
    check(name, qs, ts, 751, 400, -1, APPROX | RIGHT, [1, 4, 5])
    qs, ts = make_pairs(2, [220, 260, 310, 1100], ambig=True)
    for amb in (0, 1, 3):
        check(name, qs, ts, 751, 400, -1, APPROX, [1, 3, 4, 5, 6], sc_ambi=amb)
    qs, ts = make_pairs(3, [450, 500], big_indel=True)
    check(name, qs, ts, 751, 400, -1, APPROX, [1, 3, 4, 5, 6])


def strip_exact_limit(s):
    """The largest L = max(qlen, tlen) + 1 that ext_strip_exact_ok admits: 8 mch L < 32000 and 16 min(q + e L, q2 + e2 L) < 32000."""
    l_mch = 31999 // (8 * s['a'])
    l_gap = max((1999 - s['q']) // s['e'], (1999 - s['q2']) // s['e2'])
    return min(l_mch, l_gap)


def test_strip_exact_limit_is_the_guard_boundary():
    """(the closed form above against the two inequalities as the guard states them)"""
    for name, s in SETS.items():
        ok = lambda L: 8 * s['a'] * L < 32000 and 16 * min(s['q'] + s['e'] * L, s['q2'] + s['e2'] * L) < 32000   # noqa: E731
        L = strip_exact_limit(s)
        assert ok(L) and not ok(L + 1), (name, L)
    assert strip_exact_limit(dict(a=2, b=4, q=4, e=2, q2=24, e2=1)) == 1975 and strip_exact_limit(SETS['A15']) == 266


@pytest.mark.parametrize('name', TABLE)
def test_exact_strips(built, name):
    """The exact strip variants (kernel 4: the band never clips, up to 1024 target rows): end extensions to the right and to the left,
    exact global fills, z-drop at the default and at a small threshold, without and with an end bonus, unrelated tails, ambiguous
    bases, ties on every anti-diagonal -- and one window on each side of ext_strip_exact_ok's boundary, which both must equal the
    oracle (the guard as well as the cell): a long query on a short target (the first row reaches the gap-cost bound) and, where the
    limit is below 1024 rows, a near-identical square window (H reaches the match bound)."""
    rng = np.random.default_rng(41)
    qs, ts = make_pairs(41, [1, 3, 17, 47, 64, 150, 256, 257, 420, 512, 800, 1000])
    ts = [np.concatenate([t, rng.integers(0, 4, size=len(t) // 2 + 3).astype(np.uint8)])[:1024] for t in ts]   # target window ~1.5 x query
    for flag in (EXTZ, EXTZ | RIGHT | REV, 0, RIGHT):
        check(name, qs, ts, 3000, 400, -1, flag, [4, 0, 1])
        check(name, qs, ts, 3000, 45, 20, flag, [4])
    qs, ts = make_pairs(42, [60, 130, 260, 500], tail=True)          # unrelated tails: the extension z-drops
    qs, ts = [q[:1000] for q in qs], [t[:1024] for t in ts]
    for flag in (EXTZ, EXTZ | RIGHT | REV):
        check(name, qs, ts, 3000, 400, -1, flag, [4, 1])
        check(name, qs, ts, 3000, 30, 5, flag, [4, 0])
    qs, ts = make_pairs(43, [80, 240, 480], ambig=True)
    for amb in (0, 3):
        check(name, qs, ts, 3000, 400, 10, EXTZ, [4], sc_ambi=amb)
        check(name, qs, ts, 3000, 60, -1, EXTZ | RIGHT | REV, [4, 1], sc_ambi=amb)
    qs, ts = low_complexity((50, 150, 333), None)
    for flag in (EXTZ, EXTZ | RIGHT | REV, 0):
        check(name, qs, ts, 3000, 400, -1, flag, [4, 1])
        check(name, qs, ts, 3000, 20, 3, flag, [4])
    # both sides of the guard
    L = strip_exact_limit(SETS[name])
    rng = np.random.default_rng(44)
    qs, ts = [], []
    for qlen in (L - 5, L + 5):
        t = rng.integers(0, 4, size=min(1000, L // 2)).astype(np.uint8)
        q = np.concatenate([mutate(rng, t, 0.05), rng.integers(0, 4, size=qlen).astype(np.uint8)])[:qlen]
        qs.append(q)
        ts.append(t)
        if L + 5 <= 1024:
            t = rng.integers(0, 4, size=qlen).astype(np.uint8)
            q = t.copy()
            q[rng.integers(0, qlen, size=3)] ^= 1
            qs.append(q)
            ts.append(t)
    assert all(len(q) == n for q, n in zip(qs[::2] if L + 5 <= 1024 else qs, (L - 5, L + 5)))
    for flag in (EXTZ, EXTZ | RIGHT | REV, 0):
        check(name, qs, ts, 3000, 400, -1, flag, [4, 0])


@pytest.mark.parametrize('name', TABLE)
def test_tiled_windows(built, name):
    """Kernel 6 (and the dispatcher's choice) beyond the strips' reach, on the flags of test_tiled_exact_extensions: tails that z-drop,
    reach_end / mqe without tails, exact global fills, lopsided windows whose band leaves the matrix, low complexity, and the
    tiled gap fills.  The sets outside WIDE run the shorter half of the list."""
    qs, ts = make_pairs(9, [3000, 5200], tail=True)
    check(name, qs, ts, 751, 400, -1, EXTZ, [6, 0])
    check(name, qs, ts, 751, 400, -1, EXTZ | RIGHT | REV, [6, 0])
    qs, ts = make_pairs(17, [1100, 1500, 2600, 4800])           # no tail: the extension runs to the end (reach_end / mqe)
    check(name, qs, ts, 751, 400, 10, EXTZ, [6, 0])
    check(name, qs, ts, 751, 400, -1, EXTZ | RIGHT | REV, [6])
    check(name, qs, ts, 751, 400, -1, 0, [6, 0])                # exact global fill
    check(name, qs, ts, 300, 100, -1, 0, [6])
    qs, ts = make_pairs(15, [1000, 1025, 2049, 3000])
    check(name, qs, ts, 751, 400, -1, APPROX, [6, 0])
    check(name, qs, ts, 9000, 400, -1, APPROX, [6])             # no clipping, only tiles
    if name not in WIDE:
        return
    qs, ts = make_pairs(13, [700, 2000, 3500], tail=True)
    for w in (100, 500, 1000):
        check(name, qs, ts, w, 400, -1, EXTZ, [6])
        check(name, qs, ts, w, 200, 30, EXTZ | RIGHT | REV, [6])
    qs, ts = make_pairs(18, [1200, 2500], ambig=True, big_indel=True)
    check(name, qs, ts, 751, 400, -1, EXTZ, [6], sc_ambi=3)
    check(name, qs, ts, 751, 100, 5, EXTZ | RIGHT | REV, [6], sc_ambi=0)
    qs, ts = lopsided(3, ((5000, 1300), (1300, 5000), (4000, 1100), (600, 1500)), 0.9)   # the band leaves the matrix long before the query ends
    check(name, qs, ts, 751, 400, -1, EXTZ, [6, 0])
    check(name, qs, ts, 200, 400, -1, EXTZ | RIGHT | REV, [6])
    qs, ts = low_complexity((1300, 2200), 37)
    for flag in (EXTZ, EXTZ | RIGHT | REV, 0):
        check(name, qs, ts, 500, 400, -1, flag, [6])
        check(name, qs, ts, 500, 20, 3, flag, [6])


def h_pair(length, rate):
    rng = np.random.default_rng(1)
    t = rng.integers(0, 4, size=length).astype(np.uint8)
    return (mutate(rng, t, rate) if rate > 0 else t.copy()), t


@pytest.mark.parametrize('name,length,rate,above', [('A5', 6900, 0.02, True), ('A8', 6900, 0.12, True), ('A15', 2400, 0.0, True),
                                                    ('A5d', 6500, 0.0, False), ('A4', 6900, 0.0, False), ('A4', 7000, 0.0, False)])
def test_h_range_high_side(built, name, length, rate, above):
    """H above the 16-bit field of the tiled exact variant's anti-diagonal word (32767): windows inside its geometry limits whose
    maximum lies beyond (the test asserts that it does), and controls just inside the field.  A value that lost its top bit would
    make a high-scoring anti-diagonal look low: the maximum would land early and the z-drop rule could fire.
    ext_tile_exact_ok refuses match * min(qlen, tlen) >= 32000, so under force_kernel = 6 the windows above the field and the A5d
    control (32500: inside the field, outside the guard) take the workgroup kernel; the A4 controls (27600 and 28000, the largest a
    14000-anti-diagonal window reaches at match 4) are the ones that run the tiled exact cell near the top of its range."""
    q, t = h_pair(length, rate)
    q = q[:7000]   # (inside the tiled exact variant's geometry limits, whatever the insertions added)
    assert len(q) + len(t) - 1 <= 14000 and len(t) <= 8191
    for flag in (EXTZ, EXTZ | RIGHT | REV, 0):
        want = check(name, [q], [t], 751, 400, -1, flag, [6, 0, 5])[0]
        if flag == EXTZ:
            assert (want['max'] > 32767) == above and (above or want['max'] > 27000), (name, want['max'])


def test_h_range_low_side(built):
    """H below -32768 in an in-band cell: the big-e set on 7000 target rows with a band that covers the matrix; the first-column cell
    (6999, 0) holds -(10 + 5 * 7000).  The window is inside the tiled variant's geometry limits, but its band is too wide for the
    pipelined classes (ext_tile_pipe_ok) and the automatic choice gives the one-wave class short windows only: force_kernel = 6
    alone brings it to the tiled kernel; 0 checks whatever the dispatcher picks instead."""
    rng = np.random.default_rng(5)
    t = rng.integers(0, 4, size=7000).astype(np.uint8)
    q = mutate(rng, t, 0.12)[:6900]
    assert len(q) == 6900 and 10 + 5 * 7000 > 32768
    for flag in (EXTZ, 0):
        check('big-e', [q], [t], 9000, 400, -1, flag, [6, 0])


@pytest.mark.parametrize('name', ['sr', 'A5'])
def test_zdrop_scaling(built, name):
    """z-drop thresholds well below and above the default on windows with unrelated tails, every kernel family."""
    small = make_pairs(6, [40, 150, 400, 900], tail=True)
    large = make_pairs(9, [3000, 5200], tail=True)
    for zdrop in (50, 100, 1000):
        for flag in (EXTZ, EXTZ | RIGHT | REV):
            check(name, small[0], small[1], 751, zdrop, -1, flag, [6, 4, 5, 1])
            check(name, [q[:1000] for q in small[0]], [t[:1024] for t in small[1]], 3000, zdrop, -1, flag, [4])   # (the exact strips)
            check(name, large[0], large[1], 751, zdrop, -1, flag, [6, 5])
