"""CPU: the plain restatement of the realigner's placement stage (tests/realign_place_ref.py) against the oracle's
fast_align_reads_to_haplotypes -- the text tests/test_realign_oracle.py pins to the compiled reference -- on the seeded windows, the
random windows and every constructed case; the oracle's end results on the constructed cases against the compiled reference's
(golden/realign_place_golden.json, made by golden/make_realign_golden.py); and that every constructed family reaches what it is
named for."""
import json
import os

import pytest

import realign_place_cases as pc
import realign_place_ref as ref
from oracle import realign_oracle as ro
from realign_cases import make_cases, make_window, random_window_kwargs

GOLD_PLACE = os.path.join(os.path.dirname(__file__), 'golden', 'realign_place_golden.json')


def _assert_equals_oracle(w, got):
    want = ro.fast_align_reads_to_haplotypes(w['seqs'], w['reference'], w['haplotypes'], w['ref_prefix'], w['ref_suffix'])
    assert len(want) == len(w['haplotypes'])
    assert got['score'] == [h['score'] for h in want]
    assert got['position'] == [[r['position'] for r in h['reads']] for h in want]
    assert got['read_score'] == [[r['score'] for r in h['reads']] for h in want]
    for hi, h in enumerate(want):       # the read's CIGAR is its length, and a dropped haplotype has no score
        assert all(r['cigar'] == ('%d=' % len(w['seqs'][ri]) if r['score'] else '') for ri, r in enumerate(h['reads']))
        assert not (got['dropped'][hi] and h['score'])


def _structure(w, got):
    """what holds for any window: the list's order, one hit per (haplotype, read, start), start = max(0, t - p), bits under hits"""
    keys = [(h, t, r, p) for h, r, s, mm, t, p in got['hits']]
    assert keys == sorted(keys)
    assert len({(h, r, s) for h, r, s, mm, t, p in got['hits']}) == len(got['hits'])
    for h, r, s, mm, t, p in got['hits']:
        assert s == max(0, t - p) and 0 <= mm <= 2 and got['kmer'][h][t] == 1
        assert s + len(w['seqs'][r]) <= len(w['haplotypes'][h]) and len(w['seqs'][r]) > 32
    assert [len(k) for k in got['kmer']] == [len(h) - 31 for h in w['haplotypes']]


def test_restatement_equals_oracle_on_seeded_and_random_windows():
    wins = make_cases() + [make_window(5000 + k, **kw) for k, kw in enumerate(random_window_kwargs())]
    n_hits = n_dropped = 0
    for w in wins:
        got = ref.place_window(**w)
        _assert_equals_oracle(w, got)
        _structure(w, got)
        n_hits += len(got['hits'])
        n_dropped += sum(got['dropped'])
    assert n_hits > 5000 and n_dropped > 10


@pytest.mark.parametrize('family', pc.FAMILIES)
def test_restatement_equals_oracle_on_constructed_cases(family):
    for f, name, w in pc.make_cases():
        if f == family:
            _assert_equals_oracle(w, pc.placed(w))
            _structure(w, pc.placed(w))


def test_restatement_equals_oracle_on_the_overflow_case():
    w = pc.all_a_window()
    got = pc.placed(w)
    _assert_equals_oracle(w, got)
    _structure(w, got)
    assert len(got['hits']) == pc.ALL_A_HITS == 66720 > 65536
    assert max(16 * len(w['seqs']) * len(w['haplotypes']), 65536) < len(got['hits'])   # above the list's first capacity


def test_oracle_end_results_on_constructed_cases_match_compiled_reference(oracle_built):
    gold = json.load(open(GOLD_PLACE))['expected']
    wins = [(f + '/' + n, w) for f, n, w in pc.make_cases()] + [('overflow/all_a', pc.all_a_window())]
    assert sorted(gold) == sorted(k for k, _ in wins)
    for key, w in wins:
        assert [list(x) for x in ro.realign_reads(**w)] == gold[key], key


# ---- every family reaches what it is named for --------------------------------------------------------------------------------
def _hits(w, hap=0, read=None, start=None):
    return [x for x in pc.placed(w)['hits'] if x[0] == hap and (read is None or x[1] == read) and (start is None or x[2] == start)]


def test_lengths_family():
    seen, diagonals = set(), set()
    for f, name, w in pc.make_cases():
        if f != 'lengths':
            continue
        (hap,), got = w['haplotypes'], pc.placed(w)
        HL = len(hap)
        assert got['dropped'] == [False]
        for r, s in enumerate(w['seqs']):
            L = len(s)
            seen.add((HL, L))
            diagonals.add(HL + L - 63)
            if L <= 32 or L > HL:
                assert not _hits(w, read=r)                                        # not indexed, or no room
            if L > HL:
                assert any(e[2] == r and e[5] is None for e in got['evals'])       # k-mers marked, nothing placed
            if 32 < L <= HL and r % 2 == 0:
                assert (0, r, HL - L, 0) in [x[:4] for x in _hits(w, read=r)]      # the read that ends with the haplotype
            if 32 < L <= HL and r % 2 == 1:
                assert (0, r, 0, 1) in [x[:4] for x in _hits(w, read=r)]           # one mismatch, at start 0
        if any(len(s) > HL for s in w['seqs']):
            assert set(got['kmer'][0]) == {1}
    assert {(HL, L) for HL in pc.LENGTHS_HL for L in pc.LENGTHS_L} <= seen
    assert {1, 63, 64, 65, 127, 128, 129} <= diagonals
    assert {(32, 32), (64, 64), (96, 96), (32, 250), (160, 33)} <= seen       # L == HL, L > HL


def _start0(w):
    """the accepted evaluations of start 0 as (t, p), split into diagonal 0's own and the clamped ones"""
    ev = [(t, p) for h, t, r, p, s, mm in pc.placed(w)['evals'] if s == 0 and mm is not None and mm <= 2]
    return sorted(x for x in ev if x[0] == x[1]), sorted(x for x in ev if x[0] < x[1])


def test_clamp_family():
    def hit0(name):
        h = _hits(pc.case('clamp', name), start=0)
        assert len(h) <= 1
        return h[0] if h else None

    own, clamped = _start0(pc.case('clamp', 'only_clamp'))
    assert not own and clamped and hit0('only_clamp') == (0, 0, 0, 2, 0, 21)       # only through the clamp: t = 0, offset 21
    assert len({t for t, p in clamped}) >= 3
    own, clamped = _start0(pc.case('clamp', 'same_t'))
    assert own[0][0] == clamped[0][0] == 6 and hit0('same_t') == (0, 0, 0, 2, 6, 6)   # same t: the smaller p, diagonal 0's, wins
    own, clamped = _start0(pc.case('clamp', 'own_earlier'))
    assert own[0] == (0, 0) < clamped[0] and clamped[0][0] == 10 and hit0('own_earlier') == (0, 0, 0, 0, 0, 0)
    own, clamped = _start0(pc.case('clamp', 'own_later'))
    assert own[0] == (21, 21) and clamped[0] == (0, 21) and hit0('own_later') == (0, 0, 0, 2, 0, 21)
    w = pc.case('clamp', 'three_mm')
    assert hit0('three_mm') is None and any(s == 0 and mm == 3 for h, t, r, p, s, mm in pc.placed(w)['evals'])
    assert pc.placed(w)['kmer'][0][0] == 1                                           # no hit, the bit still set
    own, clamped = _start0(pc.case('clamp', 'far'))
    assert not own and clamped == [(10, 80)] and hit0('far') == (0, 0, 0, 0, 10, 80)
    assert len(pc.case('clamp', 'far')['seqs'][0]) >= 110 and 80 - 10 > 64
    own, clamped = _start0(pc.case('clamp', 'two_negative'))
    assert not own and {(14, 21), (7, 21), (0, 21), (0, 28)} <= set(clamped) and hit0('two_negative') == (0, 0, 0, 2, 0, 21)


def test_letters_family():
    def one(name, read=0):
        w = pc.case('letters', name)
        return w, [x[2:] for x in _hits(w, read=read)]

    w, h = one('n_both')
    assert h == [(10, 0, 10, 0)] and 'N' in w['seqs'][0][:32] and w['haplotypes'][0][30] == 'N'
    w, h = one('n_read')
    assert h == [(10, 0, 16, 6)] and w['seqs'][0][5] == 'N'                        # the run starts behind the N; no mismatch
    w, h = one('n_hap')
    assert h == [(10, 0, 31, 21)] and w['haplotypes'][0][30] == 'N'
    w, h = one('lower_read')
    assert h == [(10, 1, 10, 0)] and not _hits(w, read=1)                          # lower against upper case is a mismatch
    w, h = one('lower_both')
    assert h == [(20, 0, 20, 0)] and [x[2:4] for x in _hits(w, read=1)] == [(20, 1)]
    w, h = one('mm2')
    assert [x[:2] for x in h] == [(10, 2)]
    w, h = one('mm3')
    assert h == [] and any(mm == 3 for *_, mm in pc.placed(w)['evals']) and 1 in pc.placed(w)['kmer'][0]
    w, h = one('first_last')
    assert h == [(10, 2, 11, 1)]
    w, h = one('n_and_mm')
    assert [x[:2] for x in h] == [(10, 2)]


def test_ties_family():
    w = pc.case('ties', 'tandem')
    got = pc.placed(w)
    starts = [x[2] for x in _hits(w, hap=0, read=0)]
    assert len(starts) >= 6 and len({x[3] for x in _hits(w, hap=0, read=0)}) == 1   # many starts, one score
    assert got['position'][0][0] == _hits(w, hap=0, read=0)[0][2]                   # the first evaluated keeps the read
    ev = [(t, r) for h, t, r, p, s, mm in got['evals'] if h == 0]
    assert max(ev.count(x) for x in set(ev)) >= 2                                   # one read, two offsets, one t
    w = pc.case('ties', 'identical')
    hs = _hits(w, hap=0)
    assert [x[1] for x in hs] == [0, 1, 2] and len({x[2:] for x in hs}) == 1
    w = pc.case('ties', 'meet')
    by_t = {}
    for h, t, r, p, s, mm in pc.placed(w)['evals']:
        by_t.setdefault(t, set()).add(r)
    assert any(rs == {0, 1, 2} for rs in by_t.values())


def test_coverage_family():
    def res(name):
        w = pc.case('coverage', name)
        got = pc.placed(w)
        return w, got, got['dropped'][0], got['score'][0]

    def uncovered_kmer_at(w, got, x):
        """x holds a read's k-mer and no accepted evaluation with t <= x covers it"""
        assert got['kmer'][0][x] == 1
        return not any(t <= x and s <= x < s + len(w['seqs'][r]) for h, r, s, mm, t, p in got['hits'])

    for name, x, dropped in (('below_prefix', 59, False), ('at_prefix', 60, True), ('below_suffix', 119, True), ('at_suffix', 120, False),
                             ('suffix_over_hl', 100, True), ('prefix_zero', 50, True), ('prefix_zero_at_0', 0, True),
                             ('decoy_no_fit', 110, True), ('late', 60, True), ('is_reference', 100, False), ('zero_score', 20, False)):
        w, got, d, score = res(name)
        assert uncovered_kmer_at(w, got, x), name
        assert d == dropped, name
        assert (score > 0) == (not dropped and name != 'zero_score'), name
    w, got, d, score = res('suffix_over_hl')
    assert w['ref_suffix'] > len(w['haplotypes'][0])
    w, got, d, score = res('prefix_zero')
    assert w['ref_prefix'] == 0
    w, got, d, score = res('no_kmer')                 # uncovered positions without a k-mer: the test is skipped there
    assert not d and score > 0 and got['kmer'][0][50] == 0 and w['ref_prefix'] == 0 == w['ref_suffix']
    w, got, d, score = res('decoy_no_fit')
    assert any(mm is None and t == 110 for h, t, r, p, s, mm in got['evals'])
    w, got, d, score = res('at_prefix')
    assert any(mm == 3 and t == 60 for h, t, r, p, s, mm in got['evals'])
    w, got, d, score = res('late')                    # covered in the end, by a placement found behind it
    assert any(s <= 60 < s + len(w['seqs'][r]) and t > 60 for h, r, s, mm, t, p in got['hits'])
    w, got, d, score = res('in_time')
    assert not d and any(s <= 60 < s + len(w['seqs'][r]) and t <= 60 for h, r, s, mm, t, p in got['hits'])
    w, got, d, score = res('is_reference')
    assert w['haplotypes'][0] == w['reference']
    w, got, d, score = res('zero_score')
    assert got['position'] == [[-1, -1]]


def test_shapes_family():
    pairs = set()
    for f, name, w in pc.make_cases():
        if f == 'shapes':
            pairs.add(len(w['seqs']) * len(w['haplotypes']))
    assert {1, 3, 4, 5, 9} <= pairs
    w = pc.case('shapes', 'no_reads')
    assert pc.placed(w)['hits'] == [] and pc.placed(w)['position'] == [[], []] and set(pc.placed(w)['kmer'][0]) == {0}
    w = pc.case('shapes', 'no_haplotypes')
    assert ref.results(pc.placed(w)) == dict(hits=[], kmer=[], dropped=[], score=[], position=[], read_score=[])
    w = pc.case('shapes', 'short_reads')
    assert max(len(s) for s in w['seqs']) == 32 and pc.placed(w)['hits'] == [] and pc.placed(w)['evals'] == []
    for n in (1, 3, 4, 5, 9):
        assert pc.placed(pc.case('shapes', 'pairs%d' % n))['hits']
