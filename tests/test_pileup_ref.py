"""CPU test: the restatement of the candidate extraction (tests/pileup_ref.py) gives, on every golden case written as BAM, the bytes
Clair's own preprocess/ExtractVariantCandidates.py printed (tests/golden/candidates, made by tests/golden/make_candidates_golden.py)."""
import pytest

import pileup_cases as pc
import pileup_ref as ref


def restated(tmp_path, case):
    bam_fn, _, _ = pc.write_case(tmp_path, case)
    text = pc.text_of(bam_fn)
    o = case['options']
    ctg = o['ctgName']
    seq = dict((n, s) for n, s in case['contigs'])[ctg]
    bed = None if case['bed'] is None else ref.bed_intervals(case['bed'], ctg)
    took = ref.taken(text, ctg, o.get('minMQ', 0))
    rows = ref.candidates(ref.counts(text, ctg, o.get('minMQ', 0)), seq, o.get('ctgStart'), o.get('ctgEnd'), o['threshold'], o['minCoverage'], bed)
    return ref.lines(ctg, rows), took


def test_the_goldens_hold_what_they_should():
    cases = pc.golden_cases()
    assert len(cases) >= 20
    assert any(c['no_read'] for c in cases) and any(c['bed'] for c in cases) and any('ctgStart' in c['options'] for c in cases)
    assert {c['options']['threshold'] for c in cases} >= {0.125, 0.2, 1.0 / 3.0}
    assert {c['options']['minCoverage'] for c in cases} >= {4, 2.5}
    by = {c['name']: c['stdout'] for c in cases}
    # the streaming quirk: three leading insertions count once, or not at all behind a taken record of the same POS; a record that
    # --minMQ skips does not stand in their way
    assert ' I 1 ' in by['09_lead_first'] and ' D 1 ' in by['09_lead_first']
    assert ' I 0 ' in by['11_lead_later']
    assert ' I 1 ' in by['12_lead_lowq'] and ' I 1 ' in by['13_lead_lowq']
    # second count 1 of depth 8 passes 0.125 and not 0.126; 2 of 6 passes 1/3
    assert 'ctgA 41 ' in by['00_basic'] and 'ctgA 41 ' not in by['03_basic']
    assert 'ctgA 151 ' in by['02_basic']


@pytest.mark.parametrize('case', pc.golden_cases(), ids=lambda c: c['name'])
def test_restatement_prints_the_reference_bytes(tmp_path, case):
    got, took = restated(tmp_path, case)
    assert got == case['stdout']
    assert (len(took) == 0) == case['no_read']
