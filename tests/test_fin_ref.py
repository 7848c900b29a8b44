"""CPU tests of the plain restatement the finishing kernel is checked against (fin_ref.py): it equals the oracle's own fix_cigar +
update_extra (exported as mmo_fix_update) on every case of every family of fin_cases.py, it gives the literal values of a few
hand-worked cases, and the families reach the mechanisms test_aln_finish_gpu.py relies on them to reach (counted by fin_ref's
events only, so that a change to the generators cannot quietly empty a family)."""
import pytest

from fin_cases import HAND, LDS_CLASSES, N_OPS, PERIODS, families, hand_alns
from fin_ref import KEYS, fin_ref

SCORINGS = (dict(a=2, b=4, sc_ambi=1, q_=4, e=2), dict(a=1, b=19, sc_ambi=3, q_=39, e=3), dict(a=5, b=4, sc_ambi=0, q_=8, e=2))


@pytest.fixture(scope='module')
def fams():
    return families()


@pytest.fixture(scope='module')
def refs(fams):
    return {name: [fin_ref(a.cigar, a.q, a.t) for a in alns] for name, alns in fams.items()}


def test_ref_equals_oracle_export(oracle_built, fams, refs):
    from oracle import mm2_bindings as mb
    n = 0
    for name, alns in fams.items():
        for k, (a, r) in enumerate(zip(alns, refs[name])):
            for sc in SCORINGS[:1] if name == 'sizes' else SCORINGS:
                want = mb.fix_update(a.cigar, a.q, a.t, **sc)
                got = r if sc is SCORINGS[0] else fin_ref(a.cigar, a.q, a.t, **sc)
                for key in KEYS:
                    assert got[key] == want[key], (name, a.name, key, sc)
                n += 1
    assert n > 600


def test_hand_worked_cases(oracle_built):
    from oracle import mm2_bindings as mb
    assert len(HAND) >= 5
    for (name, cigar, _, _, want), a in zip(HAND, hand_alns()):
        got = fin_ref(a.cigar, a.q, a.t)
        orc = mb.fix_update(a.cigar, a.q, a.t)
        for key in KEYS:
            assert got[key] == want[key], (name, key, got[key], want[key])
            assert orc[key] == want[key], (name, key, 'oracle', orc[key], want[key])


def total(rs, key):
    return sum(r['ev'][key] for r in rs)


@pytest.mark.parametrize('period', PERIODS)
def test_repeat_families_reach_the_mechanisms(fams, refs, period):
    alns, rs = fams['period-%d' % period], refs['period-%d' % period]
    assert sorted({len(a.cigar) for a in alns}) == sorted(N_OPS)
    ev = {k: total(rs, k) for k in ('shifted', 'saturated', 'dependent', 'merged', 'shrinks')}
    print(period, ev, max(r['ev']['max_shift'] for r in rs))
    assert ev['saturated'] >= 1 and ev['dependent'] >= 1 and ev['merged'] >= 1 and ev['shrinks'] >= 1, ev
    # a dependent pair (k - 2, k) in the ranges of two different lanes, for the CIGARs of 128 ops and more
    crossing = 0
    for a, r in zip(alns, rs):
        n = len(a.cigar)
        per = (n + 63) // 64
        if n >= 128:
            crossing += sum(1 for k in r['ev']['dependent_at'] if (k - 2) // per != k // per)
    assert crossing >= 1
    if period <= 2:
        assert max(r['ev']['max_shift'] for r in rs) >= 16


def test_constructed_families_reach_the_mechanisms(fams, refs):
    lead = refs['leading']
    assert total(lead, 'lead_i') >= 6 and total(lead, 'lead_d') >= 6
    for a, r in zip(fams['leading'], lead):
        if a.name.startswith('lead-'):
            assert r['qshift'] + r['tshift'] > 0 and (r['qshift'] > 0) == ('I' in a.name), a.name
            assert r['ev']['saturated'] >= 1, a.name
    by = {a.name: r for a, r in zip(fams['leading'], lead)}
    assert by['lead-I-70ops']['n_cigar'] >= 65 and by['lead-D-130ops']['n_cigar'] >= 129     # more than one / two chunks of 64 move down
    assert by['becomes-empty']['n_cigar'] == 0 and by['becomes-single']['n_cigar'] == 1 and by['becomes-single-D']['n_cigar'] == 0
    assert by['first-op-gap-I']['qshift'] == 3 and by['first-op-gap-D']['tshift'] == 4
    mer = {a.name: r for a, r in zip(fams['merge'], refs['merge'])}
    for name in ('5I6D7I-middle', '5I6D7I-end', '6D5I7D-end-after-0M', 'I-D-0M-I', 'I-D-0I', 'adjacent-after-shift', 'adjacent-after-shift-p2'):
        assert mer[name]['ev']['merged'] == 1, name
    for name in ('pair-at-end-k=n-2', '5I6D-alone', '5I6D-between', 'I-0M-D', 'emptied-runs-no-pair', 'I-0M-I', '3M4M', '3M4M-shrink', '2I3I', '2I3I-shrink'):
        assert mer[name]['ev']['merged'] == 0, name
    assert mer['adjacent-after-shift']['ev']['saturated'] >= 1 and mer['adjacent-after-shift']['cigar'] == [4 << 4, (5 << 4) | 1, (1 << 4) | 2, 7 << 4]
    assert mer['emptied-runs-no-pair']['ev']['dependent'] == 2 and mer['I-0M-D']['n_cigar'] == 4
    assert mer['3M4M']['ev']['shrinks'] == 0 and mer['3M4M']['n_cigar'] == 4 and mer['3M4M-shrink']['ev']['shrinks'] == 1
    assert mer['5I6D-alone']['n_cigar'] == 1 and mer['5I6D-between']['n_cigar'] == 4
    assert any(r['n_ambi'] > 0 and r['ev']['shifted'] for a, r in zip(fams['ambiguous'], refs['ambiguous']) if a.name.startswith('N-next'))
    dp = {a.name: r for a, r in zip(fams['dpmax'], refs['dpmax'])}
    assert dp['all-mismatch']['dp_max'] == 0 and dp['all-mismatch-1op']['dp_max'] == 0 and dp['few-ops']['dp_max'] > 0


def test_size_family_sits_on_the_class_bounds(fams, refs):
    needs = [a.need for a in fams['sizes']]
    for lds in LDS_CLASSES:
        assert needs.count(lds) == 2 and needs.count(lds + 4) == 2, lds
    beyond = [(a, r) for a, r in zip(fams['sizes'], refs['sizes']) if a.need > LDS_CLASSES[-1]]
    assert len({a.need for a, _ in beyond}) >= 4 and len(beyond) >= 5
    assert any(a.period in (1, 2) and r['ev']['dependent'] >= 1 for a, r in beyond)
    # job ids differ from list positions: the jobs beyond the classes are neither first, nor adjacent, nor in order of size
    pos = [i for i, a in enumerate(fams['sizes']) if a.need > LDS_CLASSES[-1]]
    assert pos[0] > 0 and any(b - a > 1 for a, b in zip(pos, pos[1:]))
    assert all(k <= 2 for a in fams['sizes'] for k in [c & 15 for c in a.cigar])


def test_offset_family_covers_every_word_offset(fams):
    offs = fams['offsets']
    for rev in (0, 1):
        mine = [p for p in offs if p.rev == rev]
        assert {p.off_qs for p in mine} == set(range(4)) and {p.off_qe for p in mine} == set(range(4)), rev
        assert {p.off_t for p in mine} == set(range(16)), rev
    first, last = offs[0], offs[-1]
    assert first.rev == 1 and first.qs == 0                       # the word below the first read
    assert last.ts + len(last.t) == len(last.target)              # the last word of the packed targets
