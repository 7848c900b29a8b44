"""CPU tests of local_realign.extract_vcf_position (no GPU is needed for it) against the VCF and the standard output that the
reference's own extract_vcf_position.py wrote (tests/golden/local_realign)."""
import gzip
import io
import os

import pytest

import local_realign_cases as lc
from megapath_nano_amd import local_realign


def run(tmp_path, vcf_text, alt, gz=False, **kw):
    vcf_fn, out_fn = os.path.join(str(tmp_path), 'in.vcf' + ('.gz' if gz else '')), os.path.join(str(tmp_path), 'out.vcf')
    with (gzip.open(vcf_fn, 'wt') if gz else open(vcf_fn, 'w')) as f:
        f.write(vcf_text)
    said = io.StringIO()
    local_realign.extract_vcf_position(vcf_fn, alt, out_fn, said=said, **kw)
    with open(out_fn) as f:
        return f.read(), said.getvalue()


@pytest.mark.parametrize('gz', [False, True])
@pytest.mark.parametrize('case', lc.golden_cases(), ids=lambda c: c['name'])
def test_the_golden_vcf_and_standard_output(tmp_path, case, gz):
    vcf, said = run(tmp_path, case['vcf'], case['expected_lines'].encode(), gz)
    assert vcf == case['expected_vcf'] and said == case['expected_stdout'] and not vcf.endswith('\n')


def test_updated_rows_unchanged_rows_and_duplicate_positions(tmp_path):
    case = next(c for c in lc.golden_cases() if c['name'] == 'snp')
    alt_fn = os.path.join(str(tmp_path), 'alt')
    with open(alt_fn, 'w') as f:
        f.write(case['expected_lines'])
    vcf, said = run(tmp_path, case['vcf'], alt_fn)
    before, after = [[r for r in t.splitlines() if r[0] != '#'] for t in (case['vcf'], vcf)]
    assert len(after) == 3 and after[0] == after[2] != before[0] and after[1] == before[1] and said.count('[INFO]') == 2
    dp, af = after[0].split('\t')[-1].split(':')[2:]
    assert (dp, af) == ('30', '0.4000')


def test_rows_without_a_line_and_rows_without_four_fields(tmp_path):
    case = next(c for c in lc.golden_cases() if c['name'] == 'indel')
    other = 'other\t5\t.\tA\tC\t100\t.\t.\tGT:GQ:DP:AF\t0/1:100:30:0.5000'
    text = case['vcf'] + other + '\n'
    assert run(tmp_path, text, case['expected_lines'].encode())[0] == case['expected_vcf']                 # as in the script: not written
    assert run(tmp_path, text, case['expected_lines'].encode(), keep=lambda ctg, pos: ctg == 'other')[0] == case['expected_vcf'] + '\n' + other
    bad = case['vcf'].replace('0/1:100:30:0.5000', '0/1:100:30')
    with pytest.raises(ValueError, match='GT:GQ:DP:AF'):
        run(tmp_path, bad, case['expected_lines'].encode())
    with pytest.raises(ValueError, match='Index error'):
        run(tmp_path, case['vcf'], b'ctg\t5\n')
