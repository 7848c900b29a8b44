"""CPU test: the restatement of Clair's preprocess/CreateTensor.py (tests/tensor_ref.py) reproduces the standard output the
reference's own script wrote for every golden case (tests/golden/tensors), from the BAM bytes and random.Random(seed)."""
import platform
import random

import pytest

import pileup_cases as pc
import tensor_cases as tc
import tensor_ref as ref


@pytest.mark.parametrize('name', [c['name'] for c in tc.golden_cases()])
def test_restatement_reproduces_the_reference(tmp_path, name):
    case = tc.case_named(name)
    assert platform.python_implementation() == tc.golden()['implementation']     # the order of a set and random.sample are its own
    bam_fn, _ = tc.write_case(tmp_path, case)
    ctg, seq = case['contigs'][0]
    got = ref.lines(pc.text_of(bam_fn), seq, case['positions'], ctg, left_edge=not case['options'].get('stop_consider_left_edge', False),
                    rng=random.Random(case['seed']), **tc.keywords(case))
    assert got == case['stdout']


def test_the_cases_cover_what_they_are_named_for():
    by = {c['name']: c for c in tc.golden_cases()}
    assert len(by['deep_cap']['stdout'].splitlines()) == 100
    assert by['min_coverage_first']['stdout'] == '' and len(by['min_coverage_second']['stdout'].splitlines()) == 1
    assert sum(n for n, _ in by['deep_cap']['reads']) == 10050
    # the set of the 120 scattered indices does not come out in ascending order
    high = [i for i, line in enumerate(tc.expand(by['deep_1000_scattered']['reads'])) if '%' not in line.split('\t')[10]]
    assert len(high) == 120 and list(set(high)) != sorted(high)
    assert all(len(l.split()) == 3 + 1056 for c in tc.golden_cases() for l in c['stdout'].splitlines() if len(l.split()[2]) == 33)
