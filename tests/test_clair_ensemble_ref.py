"""CPU test: the plain restatement (tests/clair_ensemble_ref.py) prints, byte for byte, what the reference's own ensemble.py and
overlap_variant.py printed (tests/golden/clair_ensemble/, written by tests/golden/make_clair_ensemble_golden.py)."""
import pytest

import clair_ensemble_cases as ec
import clair_ensemble_ref as ref


def test_the_golden_holds_the_cases_the_tests_name():
    g = ec.golden()
    assert [c['name'] for c in g['ensemble']] == ec.ENSEMBLE_NAMES and [c['name'] for c in g['overlap']] == ec.OVERLAP_NAMES


@pytest.mark.parametrize('name', ec.ENSEMBLE_NAMES)
def test_ensemble_restatement_on_the_goldens(name):
    case = ec.ensemble_case(name)
    assert ref.ensemble_text(case['input'], case['minimum_count']) == case['output']


@pytest.mark.parametrize('name', ec.OVERLAP_NAMES)
def test_overlap_restatement_on_the_goldens(name):
    case = ec.overlap_case(name)
    assert ref.overlap_text(case['input']) == case['output']


def test_what_the_goldens_show():
    """first-appearance order with '10' ahead of '9'; a key below the count is dropped; an exact tie goes to the even digit; a
    deletion over a SNP keeps the later row unless the kept one has the strictly higher QUAL"""
    one = ec.ensemble_case('one_line_per_key')['output'].splitlines()
    assert [l.split('\t')[1] for l in one] == ['10', '9', '9', '09', '100000']
    assert len(ec.ensemble_case('interleaved_min3')['output'].splitlines()) == 2
    ties = ec.ensemble_case('ties')['output'].splitlines()[0].split('\t')[3 + ec.CELLS:]
    assert ties[0] == '0.007812' and ties[1] == '0.023438'             # 1/128 = 7812.5e-6 down to even, 3/128 = 23437.5e-6 up to even
    rows = [l.split('\t') for l in ec.overlap_case('deletion_over_snp')['output'].splitlines() if l[0] != '#']
    assert [(r[1], r[5]) for r in rows] == [('102', '60'), ('200', '60'), ('302', '55')]
    assert all(r[2] == r[6] == r[7] == '.' for r in rows)
    quals = [l.split('\t') for l in ec.overlap_case('chromosomes_and_quals')['output'].splitlines() if l[0] != '#']
    assert any(r[5] == '12' and r[9].split(':')[1] == '12' for r in quals)
