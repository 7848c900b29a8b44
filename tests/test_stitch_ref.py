"""CPU tests of the plain restatement the stitching stage is checked against (stitch_ref.py): it equals the second half of the
oracle's own align1 (exported as mmo_stitch_hit, which runs the function align1 runs, with the caller's window results in place of
the DP) field by field and operation by operation on every hit of every family of stitch_cases.py, and the families reach the
mechanisms test_ext_stitch_gpu.py relies on them to reach.  What is reached is counted from stitch_ref's own record only, never
from the kernel, so that a change to the generators cannot quietly empty a family.

Five things the stage's description names cannot happen on windows that the oracle plans too, or on input that passes the entry's
validation at all, and are covered by their nearest reachable edge:
  - a hit without a right extension is never planned (y < qlen and x < tlen leave room behind the last k-mer's centre): such hits
    are run against the restatement alone (`n*-noright` in `sizes`); a refused right extension is the nearest planned one.
  - a cut outside the hit (split_n = 0 or split_n >= cnt): the search starts below the fill's last anchor, so 1 <= j + 1 <= cnt1 - 1
    and 1 <= split_n <= cnt - 1; split_n = 1 and split_n = cnt - 1 are in `split`.
  - for the same reason cnt1 - (j + 1) >= 1: the bar of min_cnt 0 and 1 always holds; min_cnt - 1 anchors left over exist for
    min_cnt 3 only; for min_cnt 1 exactly one is left over, for min_cnt 0 the margin is 1 at the least.
  - a span of the finishing job clamped from a negative length: a planned fill starts at an anchor of the hit (ts >= rs, qs >= qs of
    the hit) and the left extension ends at the first, so re1 >= rs1 and qe1 >= qs1; a refused fill at the first anchor gives the
    shortest hit there is (`fill-first`, and 0 x 0 in `all`); the clamp itself is taken by two hits whose cut window is moved
    before that point, run against the restatement alone (`fill-first-moved`, `drop-moved` in `refused`).
  - an inversion mark on a placeholder: the oracle's z-drop test of an empty CIGAR finds nothing, the entry refuses the pair."""
import numpy as np
import pytest

from plan_ref import EZ_EXTZ_ONLY, EZ_REFUSED, ax, ay, span
from stitch_cases import FAMILIES, families, many_hits
from stitch_ref import EZ_INV, OUT_KEYS


@pytest.fixture(scope='module')
def fams():
    return families()


@pytest.fixture(scope='module')
def refs(fams):
    """stitch_ref of every hit of every batch, computed once and left unchanged: {family: [[((out, cigar, fin, split), ev)]]}"""
    out = {name: [[c.ref(read=i) for i, c in enumerate(b.cases)] for b in batches] for name, batches in fams.items()}
    return out


def each(fams, refs, family):
    for b, rs in zip(fams[family], refs[family]):
        for c, ((out, cigar, fin, split), ev) in zip(b.cases, rs):
            yield b, c, out, cigar, fin, split, ev


def named(fams, refs, family):
    return {c.name: (c, out, cigar, fin, split, ev) for b, c, out, cigar, fin, split, ev in each(fams, refs, family)}


def test_families_are_the_ones_named():
    assert set(FAMILIES) == {'sizes', 'merge', 'empty', 'cut', 'refused', 'ends', 'split', 'batch'}


def oracle_hit(mb, c):
    opt = mb.default_opt(**c.opt)
    a = np.array(c.read.anchors, dtype=np.uint64).reshape(-1, 2)
    rows, ops = [], []
    for w in c.wins:
        r = w['res']
        kind = (0 if w['reversed'] else 2) if w['flag'] & EZ_EXTZ_ONLY else 1
        rows.append([kind, w['qs'], w['ts'], r['max'], r['zdropped'], r['max_q'], r['max_t'], r['mqe_t'], r['score'], r['reach_end'], len(r['ops']),
                     2 if w['flag'] & EZ_INV else r['zdropped']])
        ops.extend(length << 4 | kind_ for kind_, length in r['ops'])
    got = mb.stitch_hit(opt, c.k, c.tlens[c.hit['rid']], c.read.qlen, c.as_, c.cnt, c.mlen, c.split_inv, a, rows, ops)
    assert [tuple(int(v) for v in p) for p in a] == [tuple(p) for p in c.anchors_planned]     # the marks the oracle's planning left
    return got


def compare(what, c, out, cigar, split, o, ocig):
    for key in OUT_KEYS:
        if key == 'split_inv':
            continue
        assert out[key] == o[key], what + (key, out[key], o[key])
    assert cigar == ocig, what + ('cigar',)
    assert o['consumed'] == (out['drop_fill'] + (1 if c.wins[0]['flag'] & EZ_EXTZ_ONLY and c.wins[0]['reversed'] else 0) + 1 if out['dropped']
                             else len(c.wins)), what + ('windows consumed', o['consumed'])
    if split is None:
        # no second hit; the hit keeps what it came with (split_reg was not called, or returned at once)
        assert o['r2_cnt'] == 0 and o['mlen'] == c.mlen and o['r2_split_inv'] == 0, what + ('no split', o)
        assert out['split_inv'] == 0 or out['split_n'] > 0, what
    else:
        assert (o['r2_as'], o['r2_cnt']) == (split['r2_as'], split['r2_cnt']), what + ('r2', o, split)
        assert (o['mlen'], o['blen'], o['r2_mlen'], o['r2_blen']) == (split['mlen_l'], split['blen_l'], split['mlen_r'], split['blen_r']), what + ('sums', o, split)
        assert o['r2_split_inv'] == out['split_inv'], what + ('split_inv', o['r2_split_inv'], out['split_inv'])
        n = out['split_n']
        h = c.anchors_planned[c.as_:c.as_ + c.cnt]
        assert (split['fx'], split['fy'], split['lx_left'], split['ly_left']) == (*h[n], *h[n - 1]), what


def test_ref_equals_oracle_export(oracle_built, fams, refs):
    from oracle import mm2_bindings as mb
    n_hits = n_alone = 0
    for name in fams:
        if name == 'batch':          # (the same hits again)
            continue
        for b, c, out, cigar, fin, split, ev in each(fams, refs, name):
            what = (name, b.name, c.name)
            if not c.oracle:
                n_alone += 1
                continue
            o, ocig = oracle_hit(mb, c)
            compare(what, c, out, cigar, split, o, ocig)
            # the finishing job is the same coordinates again
            assert (fin['qs1'], fin['rs1'], fin['n_cigar']) == (o['qs1'], o['rs1'], o['n_ops']), what
            assert fin['qspan'] == max(o['qe1'] - o['qs1'], 0) and fin['tspan'] == max(o['re1'] - o['rs1'], 0), what
            n_hits += 1
    assert n_hits >= 150 and n_alone == 9, (n_hits, n_alone)


def test_many_hits_templates_equal_oracle(oracle_built):
    from oracle import mm2_bindings as mb
    b, idx, templates = many_hits()
    assert len(b.cases) == 8300 and sorted(set(idx)) == list(range(len(templates)))
    for c in templates:
        assert len(c.wins) == 2
        (out, cigar, fin, split), ev = c.ref()
        o, ocig = oracle_hit(mb, c)
        compare(('many', c.name), c, out, cigar, split, o, ocig)
    assert sum(templates[i].ref()[0][3] is not None for i in set(idx)) == 2        # two of the templates are cut and split


def test_refused_windows_are_what_the_oracle_refuses(oracle_built, fams, refs):
    """a wrong window list, or a record where align_pair would refuse, is noticed by the replay itself"""
    from oracle import mm2_bindings as mb
    c = named(fams, refs, 'refused')['fill'][0]
    assert [bool(w['flag'] & EZ_REFUSED) for w in c.wins] == [False] * 4 + [True] + [False] * 4
    saved = c.wins[2]['qs']
    c.wins[2]['qs'] += 1
    try:
        with pytest.raises(AssertionError, match='not those align1 reaches'):
            oracle_hit(mb, c)
    finally:
        c.wins[2]['qs'] = saved
    oracle_hit(mb, c)


# ---- what the families reach, counted from the restatement's record ---------------------------------------------------------------
def test_sizes_reach_every_pass_count(fams, refs):
    got = {}
    for b, c, out, cigar, fin, split, ev in each(fams, refs, 'sizes'):
        n = len(c.wins)
        left = bool(c.wins[0]['flag'] & EZ_EXTZ_ONLY and c.wins[0]['reversed'])
        right = bool(c.wins[-1]['flag'] & EZ_EXTZ_ONLY and not c.wins[-1]['reversed'])
        got.setdefault(n, set()).add((left, right))
        assert ev['merges'] == 0 and ev['cut'] is None and out['n_ops'] == 2 * n and out['has_p'] == 1, c.name
        assert out['dp_score'] == sum(w['res']['max'] if w['flag'] & EZ_EXTZ_ONLY else w['res']['score'] for w in c.wins), c.name
    for n in (2, 63, 64, 65, 128, 129, 200):
        assert {(True, True), (False, True)} <= got[n], (n, got[n])
    assert got[1] == {(False, True), (False, False)}
    for n in (2, 64, 65):
        assert {(True, False), (False, False)} <= got[n], (n, got[n])
    assert any(c.as_ > 0 and c.hit['rev'] == 1 and c.hit['rid'] == 1 for b, c, *_ in each(fams, refs, 'sizes'))


def test_merge_family_reaches_the_scan_carry_and_the_shared_word(fams, refs):
    by = named(fams, refs, 'merge')
    for name in ('every-join', 'every-join-noleft'):
        c, out, cigar, fin, split, ev = by[name]
        assert len(c.wins) == 131 and ev['merges'] == 130 and ev['merge_joins'] == [(k, k + 1) for k in range(130)], name
        assert out['n_ops'] == 131 * 3 - 130
    c, out, cigar, fin, split, ev = by['pass-joins']
    assert ev['merge_joins'] == [(63, 64), (127, 128)]
    # runs of single-op windows: r + 1 adds land on one word; at 62 / 61 / 63 / 126 / 58 the word and its adds lie in different passes
    for name, adds, through in (('run2-at10', 3, 2), ('run3-at10', 4, 3), ('run2-at62', 3, 2), ('run3-at61', 4, 3), ('run3-at62', 4, 3), ('run3-at63', 4, 3),
                                ('run70-at5', 71, 70), ('run70-at58', 71, 70), ('run2-at126', 3, 2)):
        c, out, cigar, fin, split, ev = by[name]
        assert ev['max_adds_on_one_op'] == adds and ev['merges'] == adds and ev['merges_through_single'] == through, (name, ev)
        at = int(name.split('at')[1])
        r = adds - 1
        assert ev['merge_joins'] == [(k, k + 1) for k in range(at, at + r + 1)], name
        merged_len = 2 + 3 + sum(1 + k % 4 for k in range(at + 1, at + r + 1))
        assert merged_len << 4 | (1 if at % 2 else 2) in cigar, name
    assert sum(1 for name in by if by[name][5]['max_adds_on_one_op'] >= 3) >= 9
    crossing = [name for name in by if name.startswith('run') and any(a // 64 != b // 64 for a, b in by[name][5]['merge_joins'])]
    assert len(crossing) >= 7, crossing
    c, out, cigar, fin, split, ev = by['run-from-0']
    assert ev['max_adds_on_one_op'] == 8 and cigar[0] == (sum(range(1, 9)) + 6) << 4      # (window 8 starts with 6M of its own)
    c, out, cigar, fin, split, ev = by['alternate']
    assert ev['merge_joins'] == [(k, k + 1) for k in range(0, 130, 2)] and ev['max_adds_on_one_op'] == 1


def test_empty_family_reaches_the_look_back(fams, refs):
    by = named(fams, refs, 'empty')
    c, out, cigar, fin, split, ev = by['around']
    assert ev['merge_joins'] == [(2, 5), (5, 7), (7, 9), (9, 11)] and ev['empty_skipped'] == [2, 1, 1, 1] and ev['merges_through_single'] == 1
    assert ev['ext_max_not_counted'] == 1        # (the left extension: empty with a maximum)
    c, out, cigar, fin, split, ev = by['lane0']
    assert ev['merge_joins'] == [(63, 65), (127, 129), (129, 130)] and ev['empty_skipped'] == [1, 1, 0]
    for name, skipped in (('gap-60-131', 70), ('gap-63-128', 64), ('gap-0-139', 138), ('gap-10-75', 64)):
        c, out, cigar, fin, split, ev = by[name]
        a, b = (int(v) for v in name.split('-')[1:])
        assert ev['merge_joins'] == [(a, b)] and ev['empty_skipped'] == [skipped], (name, ev)
        assert any(all(not w['res']['ops'] for w in c.wins[p:p + 64]) for p in (64,) if a < p and p + 64 <= b) or name == 'gap-10-75'
    assert sum(1 for name in by if max(by[name][5]['empty_skipped'] or [0]) >= 64) == 4
    for n in (1, 2, 65, 130):
        c, out, cigar, fin, split, ev = by['all-empty-%d' % n]
        assert len(c.wins) == n and out['n_ops'] == 0 and out['has_p'] == 0 and cigar == [], n
        assert ev['ext_max_not_counted'] == (1 if n == 1 else 2)
        assert out['dp_score'] == sum(w['res']['score'] for w in c.wins if not w['flag'] & EZ_EXTZ_ONLY)
    c, out, cigar, fin, split, ev = by['ext-max-no-ops']
    assert ev['ext_max_not_counted'] == 2 and out['dp_score'] == sum(w['res']['score'] for w in c.wins[1:-1]) and out['has_p'] == 1
    assert (out['rs1'], out['qs1']) == (c.hit['rs'] - 15, c.hit['qs'] - 13) and (out['re1'], out['qe1']) == (c.hit['re'] + 15, c.hit['qe'] + 13)


def test_cut_family_reaches_every_cut(fams, refs):
    by = named(fams, refs, 'cut')
    assert by['first-fill-noleft'][5]['cut'] == 0 and by['first-fill-noleft'][1]['drop_fill'] == 0
    for at in (1, 2, 62, 63, 64, 65, 127, 128, 138):
        for sfx in ('', '-plain'):
            c, out, cigar, fin, split, ev = by['at-%d%s' % (at, sfx)]
            assert len(c.wins) == 140 and ev['cut'] == at and out['drop_fill'] == at - 1 and out['dropped'] == 1 and ev['drop_uses_max'], at
            assert out['n_ops'] == ((at + 1) * 3 - at if not sfx else (at + 1) * 2), at
            assert ev['merges'] == (at if not sfx else 0)
            # nothing of the right extension: the hit ends in the fill
            w = c.wins[at]
            assert (out['re1'], out['qe1']) == (w['ts'] + 10, w['qs'] + 9)
    for at in (63, 64):
        assert by['at-%d-noleft' % at][5]['cut'] == at and by['at-%d-noleft' % at][1]['drop_fill'] == at
    for name, first in (('one-pass', 10), ('two-passes', 30), ('63-64', 63), ('64-65', 64), ('1-130', 1), ('70-71-third', 70)):
        c, out, cigar, fin, split, ev = by['two-' + name]
        assert ev['cut'] == first and out['drop_max_t'] == 9 and sum(w['res']['zdropped'] for w in c.wins) == 2, name
    assert by['three'][5]['cut'] == 66
    for name, n_ext, cut in (('left-zdropped', 1, None), ('right-zdropped', 1, None), ('both-zdropped-then-fill', 1, 70), ('right-zdropped-short', 1, None),
                             ('right-zdropped-noleft-64', 1, None)):
        c, out, cigar, fin, split, ev = by[name]
        assert ev['ext_zdropped'] == n_ext and ev['cut'] == cut and out['dropped'] == (cut is not None), (name, ev)
    assert len(by['right-zdropped-noleft-64'][0].wins) == 64
    for name in ('max-not-score', 'max-not-score-empty'):
        c, out, cigar, fin, split, ev = by[name]
        assert out['dp_score'] == c.wins[0]['res']['max'] + sum(w['res']['score'] for w in c.wins[1:4]) + 57
    assert by['max-0'][1]['re1'] == by['max-0'][0].wins[4]['ts']


def test_refused_family_reaches_each_position(fams, refs):
    by = named(fams, refs, 'refused')
    pos = lambda name: by[name][5]['refused']  # noqa: E731
    assert pos('left') == [0] and pos('right') == [8] and pos('both') == [0, 8] and pos('fill') == [4] and pos('fill-noleft') == [3]
    assert pos('fill-first') == [1] and pos('fill-last') == [7] and pos('all') == [0, 1] and pos('fill-at-64') == [64]
    c, out, cigar, fin, split, ev = by['left']
    assert (out['rs1'], out['qs1']) == (c.hit['rs'], c.hit['qs']) and out['dropped'] == 0
    c, out, cigar, fin, split, ev = by['left-merge-over']
    assert ev['merges'] == 0 and cigar[0] == 9 << 4
    c, out, cigar, fin, split, ev = by['right']
    assert (out['re1'], out['qe1']) == (c.hit['re'], c.hit['qe'])
    for name, cut in (('fill', 4), ('fill-noleft', 3), ('fill-first', 1), ('fill-last', 7), ('fill-after-drop', 2), ('fill-before-drop', 4), ('two-fills', 4),
                      ('fill-at-64', 64), ('fill-min-cnt-1', 4)):
        c, out, cigar, fin, split, ev = by[name]
        w = c.wins[cut]
        assert ev['cut'] == cut, (name, ev)
        if name != 'fill-after-drop':
            assert w['flag'] & EZ_REFUSED and (out['drop_max_t'], out['drop_max_q'], out['re1'], out['qe1']) == (-1, -1, w['ts'], w['qs']), name
    c, out, cigar, fin, split, ev = by['all']
    assert out['n_ops'] == 0 and out['has_p'] == 1 and out['dropped'] == 1 and fin['qspan'] == 0 and fin['tspan'] == 0 and out['dp_score'] == 0
    # a refused fill right behind the anchor the hit starts at: the hit is what the left extension reached, 15 x 13 bases
    c, out, cigar, fin, split, ev = by['fill-first']
    assert (out['rs1'], out['re1'], out['qs1'], out['qe1']) == (c.hit['rs'] - 15, c.hit['rs'], c.hit['qs'] - 13, c.hit['qs'])
    assert (fin['tspan'], fin['qspan']) == (15, 13)
    # the clamp of the finishing job's spans, on windows moved before the point the left extension reached (the restatement's alone)
    c, out, cigar, fin, split, ev = by['fill-first-moved']
    assert not c.oracle and (out['re1'] - out['rs1'], out['qe1'] - out['qs1']) == (-1, -1) and (fin['tspan'], fin['qspan']) == (0, 0)
    c, out, cigar, fin, split, ev = by['drop-moved']
    assert not c.oracle and (out['re1'] - out['rs1'], out['qe1'] - out['qs1']) == (-11, -14) and (fin['tspan'], fin['qspan']) == (0, 0)


def test_ends_family_takes_both_rules_on_both_sides(fams, refs):
    by = named(fams, refs, 'ends')
    for lr in (0, 1):
        for rr in (0, 1):
            for sfx in ('', '-rev'):
                c, out, cigar, fin, split, ev = by['reach-%d-%d%s' % (lr, rr, sfx)]
                h = c.hit
                assert (out['rs1'], out['qs1']) == ((h['rs'] - 41, h['qs0']) if lr else (h['rs'] - 22, h['qs'] - 20))
                assert (out['re1'], out['qe1']) == ((h['re'] + 46, h['qe0']) if rr else (h['re'] + 24, h['qe'] + 19))
                assert h['qs0'] != h['qs'] - 20 and h['qe0'] != h['qe'] + 19


def test_split_family_reaches_search_bar_and_sums(fams, refs):
    by = named(fams, refs, 'split')
    steps = {name: (by['search-' + name][5]['steps'], by['search-' + name][5]['fell_through']) for name in
             ('at-once', 'one-step', 'three-steps', 'four-steps', 'before-window', 'before-window-1', 'fall-through', 'fall-through-1', 'first-anchor')}
    assert steps == {'at-once': (0, False), 'one-step': (1, False), 'three-steps': (3, False), 'four-steps': (4, False), 'before-window': (5, False),
                     'before-window-1': (5, False), 'fall-through': (5, True), 'fall-through-1': (5, True), 'first-anchor': (4, False)}
    assert by['search-fall-through'][1]['split_n'] == 1 and by['search-first-anchor'][1]['split_n'] == 1
    assert by['search-fall-through-lead'][0].as_ == 9 and by['search-fall-through-lead'][5]['fell_through']
    assert by['search-fall-through-noleft'][5]['fell_through'] and by['search-fall-through-noleft'][5]['cut'] == 0
    fell = [name for name in by if by[name][5]['fell_through']]
    assert len(fell) == 8, fell
    # both sides of the bar
    margins = {}
    for name in by:
        if name.startswith('bar-'):
            c, out, cigar, fin, split, ev = by[name]
            margins.setdefault(c.min_cnt, set()).add(ev['margin'])
            assert (out['split_n'] > 0) == (ev['margin'] >= 0) == (split is not None), name
            assert out['split_inv'] == (1 if ev['margin'] >= 0 else 0), name          # (every bar case is marked as an inversion)
    assert margins == {3: {-1, 0, 1}, 1: {0, 1}, 0: {1}}, margins
    for m in (1, 0):
        c, out, cigar, fin, split, ev = by['last-fill-%d' % m]
        assert out['split_n'] == c.cnt - 1 and split['r2_cnt'] == 1
        assert by['first-fill-%d' % m][1]['split_n'] == 1
        for name in ('two-anchors-%d' % m, 'two-anchors-left-%d' % m):
            c, out, cigar, fin, split, ev = by[name]
            assert c.cnt == 2 and out['split_n'] == 1 and (split['mlen_l'], split['mlen_r']) == (span(c.read.anchors[0]), span(c.read.anchors[1]))
    assert by['two-anchors-left-1'][5]['fell_through']
    assert by['first-fill-3'][1]['split_n'] == 1
    # trimmed hits: as < as1, as1 + cnt1 < as + cnt
    c, out, cigar, fin, split, ev = by['trim-front']
    assert c.hit['as1'] == c.as_ + 1 and out['split_n'] == ev['cut'] + 1
    c, out, cigar, fin, split, ev = by['trim-front-lead']
    assert c.as_ == 5 and c.hit['as1'] == 6 and out['split_n'] == ev['cut'] + 1 - 1
    c, out, cigar, fin, split, ev = by['trim-front-first']
    assert ev['fell_through'] and out['split_n'] == 2
    c, out, cigar, fin, split, ev = by['trim-back']
    assert c.hit['as1'] == c.as_ and c.hit['cnt1'] == c.cnt - 1 and ev['margin'] == 0 and split is not None
    c, out, cigar, fin, split, ev = by['trim-back-bar']
    assert ev['margin'] == -1 and split is None and c.cnt - 37 >= 3            # (the untrimmed hit would have passed)
    c, out, cigar, fin, split, ev = by['trim-both']
    assert c.as_ == 3 and c.hit['as1'] == 4 and c.hit['cnt1'] == c.cnt - 2 and split is not None
    # the inversion mark
    assert [by[n][1]['split_inv'] for n in ('inv', 'inv-no-remainder', 'inv-elsewhere', 'inv-not-dropped')] == [1, 0, 0, 0]
    assert by['inv-no-remainder'][5]['margin'] == -1 and by['inv-not-dropped'][5]['cut'] is None
    assert sum(1 for w in by['inv-not-dropped'][0].wins if w['flag'] & EZ_INV) == 2
    # mm_split_reg's sums: the three branches of the mlen rule on both sides, halves of more than 64 anchors
    for cnt in (2, 64, 65, 200):
        cuts = sorted(int(name.split('-')[3]) for name in by if name.startswith('sums-%d-' % cnt))
        assert cuts == sorted({1, cnt // 2, cnt - 2, cnt - 1} - {0}), (cnt, cuts)
        for cut in cuts:
            c, out, cigar, fin, split, ev = by['sums-%d-cut-%d' % (cnt, cut)]
            assert c.cnt == cnt and c.hit['cnt1'] == cnt and len(c.wins) == cnt + 1 and split is not None and out['split_n'] in (cut, cut - 1), (cnt, cut, out)
    c, out, cigar, fin, split, ev = by['sums-200-cut-100']
    h = c.anchors_planned[c.as_:c.as_ + c.cnt]
    for half in (h[:out['split_n']], h[out['split_n']:]):
        assert len(half) > 64
        took = set()
        for p, q in zip(half, half[1:]):
            tl, ql = ax(q) - ax(p), ay(q) - ay(p)
            took.add('span' if tl > span(q) and ql > span(q) else 'tl' if tl < ql else 'ql')
        assert took == {'span', 'tl', 'ql'}


def test_batch_family_is_every_hit_once(fams):
    n = sum(len(b.cases) for name in fams if name != 'batch' for b in fams[name])
    assert sum(len(b.cases) for b in fams['batch']) == n and [b.min_cnt for b in fams['batch']] == [3, 1, 0]
    # the places in the pool and in the window array are shuffled, and no two windows share a word
    for b in fams['batch']:
        arr = b.arrays()
        first = arr['hits'][:, 13]
        assert (np.diff(first) < 0).any()
        iv = sorted((int(p), int(p) + int(n_)) for p, n_ in zip(arr['cig_pos'], arr['wins'][:, 12]) if n_)
        assert all(a[1] <= b_[0] for a, b_ in zip(iv, iv[1:]))
        assert (np.diff(arr['cig_pos']) < 0).any()
