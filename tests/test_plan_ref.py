"""CPU tests of the plain restatement the extension planning stage is checked against (plan_ref.py): it equals the planning half of
the oracle's own align1 (exported as mmo_plan_hit, which calls the function align1 calls) hit by hit, field by field, window by
window and anchor by anchor on every read of every family of plan_cases.py, and the families reach the mechanisms
test_ext_plan_gpu.py relies on them to reach.  What is reached is counted from plan_ref's events only, never from the kernel, so
that a change to the generators cannot quietly empty a family.

Three things the stage's description names cannot happen on input that passes the stage entry's validation, and are covered by
their nearest reachable edge instead: a trim by mm_fix_bad_ends leaves at least two anchors (each scan does), so cnt1 = 2 stands
for "a trim that leaves one anchor"; diff = 2 * min(n_ins, n_del) is even, so 40 and 42 are the two sides of the threshold; and
y < qlen, x < tlen put the last k-mer's centre inside read and target, so every hit has a right window (the shortest one, of
k / 2 + 1 bases, is in the `ends` family)."""
import time

import numpy as np
import pytest

from plan_cases import families, validate
from plan_ref import EZ_REFUSED, SEED_IGNORE, SEED_LONG_JOIN, SEED_TANDEM

LDS_ANCHORS, MASK_BITS = 1024, 8192        # what the kernel stages in LDS / covers with its bit mask (csrc/plan_kernels.h)


@pytest.fixture(scope='module')
def fams():
    return families()


@pytest.fixture(scope='module')
def refs(fams):
    """plan_ref of every read of every batch, computed once and left unchanged: {family: [[(hits, anchors, evs)]]}"""
    t0 = time.time()
    out = {name: [b.ref() for b in batches] for name, batches in fams.items()}
    assert time.time() - t0 < 30, 'the restatement is meant to take seconds'
    return out


def each(fams, refs, family):
    """(batch, read, hit tuple, hit, ev) of every hit of a family"""
    for b, rs in zip(fams[family], refs[family]):
        for r, (hits, _, evs) in zip(b.reads, rs):
            for spec, h, ev in zip(r.hits, hits, evs):
                yield b, r, spec, h, ev


def by_name(fams, refs, family, batch=0):
    """{read name: (read, hits, anchors, evs)} of one batch"""
    return {r.name: (r, *x) for r, x in zip(fams[family][batch].reads, refs[family][batch])}


def test_every_input_passes_the_entry_validation(fams):
    for batches in fams.values():
        for b in batches:
            validate(b)


def test_every_window_lies_inside_read_and_target(fams, refs):
    for name in fams:
        for b, r, spec, h, ev in each(fams, refs, name):
            for w in h['windows']:
                assert 0 <= w['qs'] and w['qs'] + w['raw']['qlen'] <= r.qlen and 0 <= w['ts'] and w['ts'] + w['raw']['tlen'] <= b.tlens[h['rid']], (b.name, r.name, w)
                assert w['raw']['qlen'] > 0 and w['raw']['tlen'] > 0, (b.name, r.name, w)


def test_ref_equals_oracle_export(oracle_built, fams, refs):
    from oracle import mm2_bindings as mb
    n_hits = n_win = 0
    for name, batches in fams.items():
        for b, rs in zip(batches, refs[name]):
            opt = mb.default_opt(**b.opt)
            for r, (hits, left, _) in zip(b.reads, rs):
                a = np.array(r.anchors, dtype=np.uint64).reshape(-1, 2)
                for (as_, cnt, mlen, inv), h in zip(r.hits, hits):
                    what = (b.name, r.name, 'hit at %d' % as_)
                    rid = h['rid']
                    oh, ow = mb.plan_hit(opt, b.k, b.tlens[rid], r.qlen, as_, cnt, mlen, inv, a)
                    for key in mb.PLAN_HIT_KEYS:
                        assert h[key] == oh[key], what + (key, h[key], oh[key])
                    assert h['n_jobs'] == len(ow) == len(h['windows']), what + ('n_jobs', h['n_jobs'], len(ow))
                    for j, (w, o) in enumerate(zip(h['windows'], ow)):
                        assert w['raw'] == o, what + ('window %d' % j, w['raw'], o)
                        # the placeholder rule: position, flags and anchor stay, the rest is zero
                        if o['refused']:
                            want = dict(o, qlen=0, tlen=0, w=0, zdrop=0, end_bonus=0, flag=o['flag'] | EZ_REFUSED)
                        else:
                            want = o
                        for key in ('qs', 'qlen', 'ts', 'tlen', 'reversed', 'w', 'zdrop', 'end_bonus', 'flag', 'anchor'):
                            assert w[key] == want[key], what + ('window %d' % j, key, w[key], want[key])
                        assert (w['rid'], w['rev']) == (oh['rid'], oh['rev'])
                    n_hits += 1
                    n_win += len(ow)
                # the anchors as the oracle left them, SEED_IGNORE marks included
                assert [tuple(int(v) for v in p) for p in a] == left, (b.name, r.name, 'anchors')
    assert n_hits > 800 and n_win > 10000


def test_ends_family(fams, refs):
    seen = set()
    for b, r, (as_, cnt, _, _), h, ev in each(fams, refs, 'ends'):
        kinds = [w['kind'] for w in h['windows']]
        assert kinds.count('right') == 1                       # (see the module's docstring)
        assert kinds == ['left'] * (h['qs'] > 0 and h['rs'] > 0) + ['fill'] * (len(kinds) - 1 - kinds.count('left')) + ['right']
        name = r.name.split('-t')[0]
        seen.add((b.k, name, h['rid'], h['rev']))
        if name in ('qs0', 'rs0', 'qs0-rs0'):
            assert 'left' not in kinds and (h['qs'] == 0) == ('qs0' in name) and (h['rs'] == 0) == ('rs0' in name), (b.name, r.name)
        if name == 'qs1-rs1':
            assert kinds[0] == 'left' and (h['qs'], h['rs']) == (1, 1) and h['windows'][0]['qlen'] == 1
        if name == 'rs0-clamp':
            assert ev['rs0_clamped'] and h['windows'][0]['ts'] == 0 and h['windows'][0]['tlen'] == 3
        if name.startswith('cnt'):
            assert cnt == int(name[3:]) and kinds.count('fill') == min(cnt - 1, 1)
        if name in ('last-base', 'both-last'):
            assert h['windows'][-1]['qlen'] == (b.k >> 1) + 1
        if name in ('t-last-base', 'both-last'):
            assert h['windows'][-1]['tlen'] == (b.k >> 1) + 1
    assert {k for k, *_ in seen} == {15, 20} and {(rid, rev) for _, _, rid, rev in seen} >= {(0, 0), (2, 1), (1, 0), (1, 1)}
    assert {fams['ends'][1].tlens[1], fams['ends'][1].tlens[2]} != {fams['ends'][1].tlens[0]}


def test_fix_bad_ends_family(fams, refs):
    stops = {'front': set(), 'back': set()}
    for b, r, (as_, cnt, _, _), h, ev in each(fams, refs, 'fix_bad_ends'):
        stops['front'].add(ev['front_stop'])
        stops['back'].add(ev['back_stop'])
    for side in ('front', 'back'):
        assert stops[side] >= {'l', 'm', 'mlen', 'long_join', 'end'}, (side, stops[side])
    d = by_name(fams, refs, 'fix_bad_ends')
    trim = {n: (x[1][0]['as1'] - x[0].hits[0][0], x[0].hits[0][0] + x[0].hits[0][1] - x[1][0]['as1'] - x[1][0]['cnt1']) for n, x in d.items()}
    assert trim['front'] == (1, 0) and trim['front-2'] == (2, 0) and trim['back'] == (0, 1) and trim['back-2'] == (0, 2) and trim['both'] == (1, 2)
    # a trimmed front and a filter range behind it: in-hit positions (the mask's) and positions after the trim differ
    r, hits, left, evs = d['both-filter']
    assert trim['both-filter'] == (2, 3) and evs[0]['ranges'] == [(18, 22)]
    assert [i for i, (x, y) in enumerate(left) if y & SEED_IGNORE] == [20, 21, 22, 23]
    # two anchors are the least a trim leaves
    assert hits[0]['cnt1'] >= 2 and all(h['cnt1'] >= 2 for *_, (_, cnt, _, _), h, _ in each(fams, refs, 'fix_bad_ends') if cnt >= 3)
    for n in ('cnt3-front', 'to-two-front', 'to-two-both'):
        assert d[n][1][0]['cnt1'] == 2 and d[n][1][0]['as1'] > 0, (n, d[n][1][0]['cnt1'])
    assert trim['to-two-both'][0] > 0 and trim['to-two-both'][1] > 0 and d['to-three'][1][0]['cnt1'] == 3
    # what stops a scan decides what it trims: a bad step into the last anchor the scan looks at, and one anchor further
    for name, n, front_in, back_in in (('l', 12, 4, 8), ('m', 90, 33, 57), ('mlen', 30, 4, 26)):
        for v in ('-in', '-out', '-back-in', '-back-out'):
            ev = d['stop-%s%s' % (name, v)][3][0]
            assert (ev['front_stop'], ev['back_stop']) == (name, name), (name, v, ev['front_stop'], ev['back_stop'])
        assert trim['stop-%s-in' % name] == (front_in, 0) and trim['stop-%s-back-in' % name] == (0, n - back_in), name
        assert trim['stop-%s-out' % name] == (0, 0) == trim['stop-%s-back-out' % name], name
    want = {'stop-never': ('end', 'end'), 'lj-front': ('long_join', None), 'lj-front-1': ('long_join', None), 'lj-back': (None, 'long_join'),
            'lj-back-last': (None, 'long_join')}
    for n, (f, bk) in want.items():
        ev = d[n][3][0]
        assert (f is None or ev['front_stop'] == f) and (bk is None or ev['back_stop'] == bk), (n, ev['front_stop'], ev['back_stop'])
    assert trim['lj-front'] == (0, 0) and trim['lj-front-1'] == (0, 0) and trim['lj-back'] == (0, 0) and trim['lj-back-last'] == (0, 0)
    assert trim['lj-none'] == (3, 4)           # the same steps without the joins
    # other thresholds move the stops
    d2 = by_name(fams, refs, 'fix_bad_ends', 1)
    assert any(d[n][1][0]['as1'] != d2[n][1][0]['as1'] or d[n][1][0]['cnt1'] != d2[n][1][0]['cnt1'] for n in d)


def test_filter_bad_seeds_family(fams, refs):
    d = by_name(fams, refs, 'filter_bad_seeds')
    ev = {n: x[3][0] for n, x in d.items()}
    marked = {n: [i for i, (_, y) in enumerate(x[2]) if y & SEED_IGNORE] for n, x in d.items()}
    assert [len(ev[n]['K']) for n in ('k0', 'k1', 'k2', 'k2-same-sign', 'k2-11')] == [0, 1, 2, 2, 2]
    assert marked['k0'] == marked['k1'] == marked['k2-same-sign'] == marked['k2-11'] == [] and marked['k2'] == [30, 31, 32, 33, 34]
    assert max(ev['diff40']['max_diffs']) == 40 and marked['diff40'] == [] and max(ev['diff42']['max_diffs']) == 42 and marked['diff42'] == [30, 31, 32, 33, 34]
    assert max(ev['diff40-3']['max_diffs']) == 40 and marked['diff40-3'] == [] and max(ev['diff42-3']['max_diffs']) == 42 and len(marked['diff42-3']) == 6
    for n in ('run12', 'run25'):
        assert ev[n]['ext_cnt_breaks'] >= 1 and len(ev[n]['K']) > 11 and marked[n], n
    assert ev['run11']['ext_cnt_breaks'] == 0 and len(ev['run11']['K']) == 11 and ev['run11']['ranges'] == [(30, 60)]      # max_ext_cnt + 1 entries: a run takes them all
    assert len(ev['run25']['ranges']) >= 2
    assert ev['far']['ext_len_breaks'] >= 1 and marked['far'] == []
    assert ev['far-edge-in']['ext_len_breaks'] == 0 and len(marked['far-edge-in']) == 122 and ev['far-edge-out']['ext_len_breaks'] == 1 and not marked['far-edge-out']
    for n in ('delayed', 'delayed-2'):
        assert ev[n]['range_replaced'] >= 1 and ev[n]['ranges'][0] == (32, 152), (n, ev[n]['ranges'])
    assert len(ev['delayed-2']['ranges']) == 3
    # mask word boundaries: an entry at each position, as a range's start, end and inside; as the first entry of all
    for p in (63, 64, 65, 127, 128):
        assert ev['bit%d' % p]['K'] == [p - 9, p, p + 7] and ev['bit%d' % p]['ranges'] == [(p - 9, p)]
        assert ev['bit%d-first' % p]['K'] == [p, p + 1] and marked['bit%d-first' % p] == [p]
    assert ev['bits-all']['K'] == [63, 64, 65, 127, 128] and marked['bits-all']
    for n in ('zero-word', 'zero-words-3', 'word-edges'):
        K = ev[n]['K']
        assert any(q // 64 - p // 64 >= 2 for p, q in zip(K, K[1:])) or n == 'word-edges', n       # an all-zero word between two entries
        assert ev[n]['ranges'] and ev[n]['ranges'][0][1] - ev[n]['ranges'][0][0] >= 64, n
    assert ev['word-edges']['K'] == [64, 128, 192, 256]
    # flagged anchors are skipped by the fills, except the last one
    assert ev['tandem']['skipped'] == 3 and ev['tandem']['flagged_last'] == 0
    assert ev['tandem-last']['skipped'] == 1 and ev['tandem-last']['flagged_last'] == 1
    assert ev['marked-last']['skipped'] == 2 and ev['marked-last']['flagged_last'] == 1 and ev['marked-last-2']['flagged_last'] == 1
    for n in ('tandem-last', 'marked-last', 'marked-last-2'):
        h = d[n][1][0]
        assert h['windows'][-2]['kind'] == 'fill' and h['windows'][-2]['anchor'] == h['cnt1'] - 1
    for n, cnt in (('k-at-last-lj', 60), ('k-at-last-span', 60), ('k-at-last-130', 130)):
        assert ev[n]['K'][-1] == cnt - 1 and d[n][1][0]['cnt1'] == cnt and marked[n] and marked[n][-1] == cnt - 2, n
    # half the reach under max_gap = 2000
    ev2 = {n: x[3][0] for n, x in by_name(fams, refs, 'filter_bad_seeds', 1).items()}
    assert ev2['zero-word']['ranges'] == [] and ev2['zero-word']['ext_len_breaks'] >= 1


def straddles(ev, as_, h, edge):
    """ranges of the hit that hold in-hit positions edge - 1 and edge (positions count from the hit's first anchor, as the mask's bits do)"""
    off = h['as1'] - as_
    return [(s + off, e + off) for s, e in ev['ranges'] if s + off < edge < e + off]


@pytest.mark.parametrize('family,edge,about', [('lds_edge', LDS_ANCHORS, 1100), ('mask_edge', MASK_BITS, 8300)])
def test_edge_families(fams, refs, family, edge, about):
    d = by_name(fams, refs, family)
    assert {x[0].hits[0][1] for x in d.values()} >= {edge - 1, edge, edge + 1, about}
    ev = {n: x[3][0] for n, x in d.items()}
    off = {n: x[1][0]['as1'] - x[0].hits[0][0] for n, x in d.items()}
    for n in ('cnt%d' % about, 'around-edge', 'offset'):
        assert straddles(ev[n], d[n][0].hits[0][0], d[n][1][0], edge), (n, ev[n]['ranges'])
    K = [p + off['cnt%d' % about] for p in ev['cnt%d' % about]['K']]
    assert any(p < edge for p in K) and sum(1 for p in K if p >= edge) >= 4                       # entries on both sides
    assert any(s + off['cnt%d' % about] > edge for s, e in ev['cnt%d' % about]['ranges'])          # a range entirely beyond
    assert [(s + off[n], e + off[n]) for n in ('ends-on-edge', 'starts-on-edge') for s, e in ev[n]['ranges']] == [(edge - 6, edge), (edge, edge + 6)]
    assert off['offset'] == 2 and d['offset'][0].hits[0][0] == 37 and ev['offset']['left']['end'] == 'other' and ev['offset']['right']['end'] == 'found'
    for n in ('cnt%d' % (edge - 1), 'cnt%d' % edge, 'cnt%d' % (edge + 1)):
        assert len(ev[n]['ranges']) == 2 and d[n][1][0]['cnt1'] == d[n][0].hits[0][1], n
    # the marks are in the anchors handed back, on both sides of the edge
    left = d['around-edge'][2]
    assert [i for i, (_, y) in enumerate(left) if y & SEED_IGNORE] == [edge - 1, edge]
    if family == 'lds_edge':
        assert ev['before-edge']['ranges'] == [(edge - 7, edge - 1)] and ev['tandem-edge']['skipped'] == 6


def test_neighbours_family(fams, refs):
    d = by_name(fams, refs, 'neighbours')
    for side, end in (('left', 'index0'), ('right', 'last')):
        ev = {n[len(side) + 1:]: x[3][0][side] for n, x in d.items() if n.startswith(side + '-')}
        lim = {n[len(side) + 1:]: (x[1][0]['qs0'], x[1][0]['rs0']) if side == 'left' else (x[1][0]['qe0'], x[1][0]['re0']) for n, x in d.items()
               if n.startswith(side + '-')}
        # min_cnt qualifying anchors change nothing, min_cnt + 1 do
        assert [ev['n%d' % n]['qualified'] for n in (0, 1, 3, 4, 5, 9)] == [0, 1, 3, 4, 4, 4]
        assert lim['n0'] == lim['n1'] == lim['n3'] != lim['n4'] == lim['n5'] == lim['n9']
        assert [ev['n%d' % n]['end'] for n in (0, 1, 3, 4)] == [end, end, end, 'found']              # the walk reaches the list's end
        assert [ev['n%d-then-other' % n]['end'] for n in (0, 3, 4)] == ['other', 'other', 'found']
        for which in ('x', 'y', 'xy'):
            e = ev['fail-' + which]
            assert e['qualified'] == 3 and e['failed_x'] == (2 if 'x' in which else 0) and e['failed_y'] == (2 if which == 'y' else 0), (side, which, e)
            assert lim['fail-' + which] == lim['n3'] and ev['fail-%s-then-4th' % which]['end'] == 'found' and lim['fail-%s-then-4th' % which] != lim['n3']
        assert [ev['edge%+d' % k]['end'] for k in (-1, 0, 1)] == (['found', end, end] if side == 'left' else [end, end, 'found'])
        for n in ('cut-by-target', 'cut-by-strand'):
            assert ev[n]['end'] == 'other' and ev[n]['qualified'] == 2 and lim[n] == lim['n0'], (side, n)
        assert ev['rev']['end'] == 'found' and ev['far-neighbours']['end'] == 'found' and lim['far-neighbours'] == lim['n0']
    assert d['left-rs1-clamp'][3][0]['rs1_clamped'] == 1
    d1 = by_name(fams, refs, 'neighbours', 1)
    assert d1['left-n1'][3][0]['left']['end'] == 'index0' and d1['left-cut-by-target'][3][0]['left']['end'] == 'found'


def test_limits_family(fams, refs):
    seen = {'left': set(), 'right': set()}
    fills = {}
    for b, r, spec, h, ev in each(fams, refs, 'limits'):
        for side in ('left', 'right'):
            g = ev[side + '_gap']
            if g is not None:
                seen[side].add((b.name.split('-ttail')[0], g['capped'], g['grown'], g['target_closer']))
        if r.name == 'lead150':
            fills[b.name] = [w['anchor'] for w in h['windows'] if w['kind'] == 'fill']
    for side in ('left', 'right'):
        for name in ('limits-default', 'limits-gap300', 'limits-a1-q10-e3'):
            got = {t[1:] for t in seen[side] if t[0] == name}
            assert {(c, True, t) for c in (False, True) for t in (False, True)} <= got, (side, name, got)     # max_gap below / above the overhang
        assert any(not t[2] for t in seen[side] if t[0] == 'limits-a1-q10-e3'), side                               # l * a <= q
    assert any(not t[2] for t in seen['left'] if t[0] == 'limits-default')
    # min_ksw_len: 0 fills between every two anchors, a value above every gap leaves the one fill that ends at the last anchor
    assert fills['limits-ksw0'] == list(range(1, 30)) and fills['limits-ksw-huge'] == [29]
    assert 1 < len(fills['limits-default']) < len(fills['limits-ksw45']) < 29
    # the overhang on the edge of max_gap: one base more changes nothing
    d = by_name(fams, refs, 'limits')
    w = {n: d[n][1][0]['windows'] for n in d}
    assert w['lead5007'][0]['qlen'] == 5000 == w['lead5008'][0]['qlen'] and w['lead5006'][0]['qlen'] == 4999
    assert w['tail5000'][-1]['qlen'] == 5000 == w['tail5001'][-1]['qlen'] and w['tail4999'][-1]['qlen'] == 4999
    assert w['tlead150'][0]['tlen'] == 143 and w['tlead8'][0]['tlen'] == 1


def test_refused_family(fams, refs):
    kinds = {}
    for b, r, spec, h, ev in each(fams, refs, 'refused'):
        kinds.setdefault(b.opt['max_sw_mat'], []).extend(ev['refused'])
        for w in h['windows']:
            if w['flag'] & EZ_REFUSED:
                assert (w['qlen'], w['tlen'], w['w'], w['zdrop'], w['end_bonus']) == (0, 0, 0, 0, 0) and w['raw']['qlen'] * w['raw']['tlen'] > b.opt['max_sw_mat']
                assert (w['qs'], w['ts'], w['anchor'], w['reversed']) == (w['raw']['qs'], w['raw']['ts'], w['raw']['anchor'], w['raw']['reversed'])
    assert kinds[0] == [] and kinds[100000000] == []
    assert set(kinds[1]) == {'left', 'fill', 'right'} and set(kinds[30000]) == {'left', 'fill', 'right'}
    n_reads = len(fams['refused'][0].reads)
    assert kinds[30000].count('fill') == 4 * n_reads and kinds[35000].count('fill') == 3 * n_reads - 2 + 2     # the last fill is 180 x 180
    # the product on the limit is not refused, one below it is
    assert kinds[40000].count('fill') == 2 and kinds[39999].count('fill') == 3 * n_reads - 2 + 2
    assert set(kinds[100000]) == {'left', 'right', 'fill'} and kinds[100000].count('fill') == 2          # only the two long fills
    assert set(kinds[185000]) == {'left', 'right'} and set(kinds[1000000]) == {'left'}
    d = by_name(fams, refs, 'refused', 2)
    assert {w['kind'] for w in d['short-ends'][1][0]['windows'] if w['flag'] & EZ_REFUSED} == {'fill'}    # short ends pass where fills do not
    # split_inv picks zdrop_inv for the left window alone
    w = by_name(fams, refs, 'refused', 0)['split-inv'][1][0]['windows']
    assert w[0]['zdrop'] == 200 and {x['zdrop'] for x in w[1:]} == {400}


def test_long_join_family(fams, refs):
    d = by_name(fams, refs, 'long_join')
    w = {n: {x['anchor']: x for x in d[n][1][0]['windows'] if x['kind'] == 'fill'} for n in d}
    assert w['lj-q'][20]['w'] == w['lj-q'][20]['qlen'] > w['lj-q'][20]['tlen'] and w['lj-t'][20]['w'] == w['lj-t'][20]['tlen'] > w['lj-t'][20]['qlen']
    assert w['lj-short'][17]['qlen'] < 200 and w['lj-short'][17]['w'] == w['lj-short'][17]['qlen'] == w['lj-short'][17]['tlen'] + 5
    assert w['lj-two'][20]['w'] > 2600 and w['lj-two'][40]['w'] > 1200 and w['lj-two'][40]['w'] == w['lj-two'][40]['tlen']
    assert 20 not in w['lj-marked'] and 20 not in w['lj-tandem'] and d['lj-marked'][3][0]['ranges'] == [(18, 22)]
    assert all(x['w'] == 751 for n in w for a, x in w[n].items() if not d[n][0].anchors[a][1] & SEED_LONG_JOIN)
    refused = [x for x in by_name(fams, refs, 'long_join', 1)['lj-two'][1][0]['windows'] if x['flag'] & EZ_REFUSED]
    assert [x['anchor'] for x in refused if x['kind'] == 'fill'] == [20]


def test_rounds_family(fams, refs):
    b1, b2 = fams['rounds'][0], fams['rounds'][1]
    for r1, r2, (h1, left1, _), (h2, left2, ev2) in zip(b1.reads, b2.reads, refs['rounds'][0], refs['rounds'][1]):
        assert r2.anchors == left1 and any(y & SEED_IGNORE for _, y in r2.anchors)
        as_, cnt, _, inv = r2.hits[0]
        assert as_ > r1.hits[0][0] and as_ + cnt == r1.hits[0][0] + r1.hits[0][1]                     # a suffix of the first pass's hit
        if h2[0]['windows'][0]['kind'] == 'left':
            assert h2[0]['windows'][0]['zdrop'] == (200 if inv else 400)
    assert {r.hits[0][3] for r in b2.reads} == {0, 1}
    # the marks a first pass left are obeyed where the remainder's own filter would not set them (its range is cut in two)
    r, hits, left, evs = by_name(fams, refs, 'rounds', 1)['r0-from12']
    assert evs[0]['skipped'] > sum(e - s for s, e in evs[0]['ranges']) - 1 and SEED_IGNORE & r.anchors[5 + 12][1]
    z = refs['rounds'][2]
    assert {w['zdrop'] for hits, _, _ in z for w in hits[0]['windows'] if w['kind'] != 'left'} == {300}
    assert {w['zdrop'] for hits, _, _ in z for w in hits[0]['windows'] if w['kind'] == 'left'} == {300, 77}


def test_batch_family(fams, refs):
    b = fams['batch'][0]
    assert sum(1 for r in b.reads if len(r.hits) > 1 and [h[0] for h in r.hits] != sorted(h[0] for h in r.hits)) >= 3      # out of order
    assert sum(len(r.hits) for r in b.reads) >= 20 and {len(r.hits) for r in b.reads} >= {2, 3}
    r, hits, left, evs = by_name(fams, refs, 'batch')['big-small-mid']
    assert [h[1] for h in r.hits] == [8300, 3, 70] and straddles(evs[0], 0, hits[0], MASK_BITS) and evs[2]['ranges'] == [(30, 35)]
    assert hits[1]['n_jobs'] == 3 and evs[1]['K'] == []
    r, hits, left, evs = by_name(fams, refs, 'batch')['mid-big-small-same-target']
    assert [h[1] for h in r.hits] == [8200, 3, 70]
    assert any(y & SEED_TANDEM for rd in fams['filter_bad_seeds'][0].reads for _, y in rd.anchors)
    assert any(y & SEED_LONG_JOIN for rd in fams['long_join'][0].reads for _, y in rd.anchors)
