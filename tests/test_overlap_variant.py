"""CPU test: clair_ensemble.overlap_filter and bin/mpn-overlap-variant print, byte for byte, what the reference's own
overlap_variant.py printed (tests/golden/clair_ensemble/), and refuse with a line number where that script raises."""
import os
import subprocess
import sys

import pytest

import clair_ensemble_cases as ec
import clair_ensemble_ref as ref
from megapath_nano_amd import clair_ensemble

TOOL = os.path.join(ec.ROOT, 'bin', 'mpn-overlap-variant')


@pytest.mark.parametrize('name', ec.OVERLAP_NAMES)
def test_overlap_filter_on_the_goldens(name):
    case = ec.overlap_case(name)
    lines = case['input'].splitlines(keepends=True)
    assert ''.join(r + '\n' for r in clair_ensemble.overlap_filter(lines)) == case['output']
    assert ''.join(r + '\n' for r in clair_ensemble.overlap_filter([l.encode() for l in lines])) == case['output']


def test_the_tool_is_a_filter_from_stdin_to_stdout():
    case = ec.overlap_case('chains')
    p = subprocess.run([sys.executable, TOOL], input=case['input'].encode(), capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert p.stdout.decode() == case['output']


def test_random_rows_equal_the_restatement():
    import random
    rng = random.Random(4)
    rows = []
    for i in range(3000):
        ref_len = rng.choice([1, 1, 1, 2, 3, 6])
        alts = ['A' * rng.choice([1, 1, ref_len, ref_len + 1, 4]) for _ in range(rng.choice([1, 1, 2]))]
        q = rng.choice([str(rng.randrange(40)), '%.2f' % (rng.random() * 40)])
        rows.append((rng.choice(['c1', 'c2']), rng.randrange(1, 900), '\t'.join(['.', 'C' * ref_len, ','.join(alts), q, 'PASS', '.', 'GT:GQ:DP:AF',
                                                                              '0/1:%s:%d:%.4f' % (q, rng.randrange(1, 99), rng.random())])))
    rows.sort(key=lambda r: r[:2])
    text = '#h\n' + ''.join('%s\t%d\t%s\n' % r for r in rows)
    got = clair_ensemble.overlap_filter(text.splitlines(keepends=True))
    assert ''.join(r + '\n' for r in got) == ref.overlap_text(text) and 500 < len(got) < 2900


def test_refusals_name_the_line():
    head = '#CHROM\n'
    good = 'c\t5\t.\tAC\tA\t10\t.\t.\tGT:GQ:DP:AF\t0/1:10:9:0.5000\n'
    for bad, no in ((good.replace('0/1:10:9:0.5000', '0/1:10:9'), 2), ('c\t5\t.\tAC\tA\n', 2), (good.replace('\t5\t', '\tx\t'), 3), (good.replace('\t10\t', '\tq\t'), 3),
                    ('\n', 2)):
        lines = [head] + ([good] if no == 3 else []) + [bad]
        with pytest.raises(ValueError, match=f'line {no}'):
            clair_ensemble.overlap_filter(lines)
    p = subprocess.run([sys.executable, TOOL], input=(head + good.replace('0/1:10:9:0.5000', '0/1')).encode(), capture_output=True, timeout=120)
    assert p.returncode == 1 and b'line 2' in p.stderr and p.stdout == b''
