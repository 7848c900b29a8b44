"""GPU tests (-m gpu) of the candidate extraction (megapath_nano_amd/candidates.py, bin/mpn-candidates): on every golden case
(tests/golden/candidates: the inputs and the bytes Clair's own ExtractVariantCandidates.py printed for them) the drop-in writes the
reference's bytes, through the function and through the command line, to standard output and to a gzip file; and what it refuses."""
import gzip
import io
import os
import subprocess
import sys

import pytest

import pileup_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'bin', 'mpn-candidates')
CASES = pc.golden_cases()


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    monkeypatch.delenv('MPN_INGEST_BATCH_BYTES', raising=False)
    monkeypatch.delenv('MPN_BAM_WALK_RECORDS', raising=False)


def argv_of(case, files, can_fn):
    bam_fn, ref_fn, bed_fn = files
    o = case['options']
    argv = ['--bam_fn', bam_fn, '--ref_fn', ref_fn, '--can_fn', can_fn, '--samtools', '/nowhere/samtools']
    if bed_fn:
        argv += ['--bed_fn', bed_fn]
    for k, v in o.items():
        argv += ['--' + k, repr(v) if isinstance(v, float) else str(v)]
    return argv


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_function_writes_the_reference_bytes(libmpn, tmp_path, capsys, case):
    from megapath_nano_amd import candidates
    bam_fn, ref_fn, bed_fn = pc.write_case(tmp_path, case)
    o = case['options']
    out = io.BytesIO()
    n = candidates.extract_variant_candidates(bam_fn, ref_fn, o['ctgName'], o.get('ctgStart'), o.get('ctgEnd'), o['threshold'], o['minCoverage'],
                                              o.get('minMQ', 0), bed_fn, out=out)
    assert out.getvalue().decode() == case['stdout']
    assert n == len(case['stdout'].splitlines())
    assert ('No read has been process' in capsys.readouterr().err) == case['no_read']


@pytest.mark.parametrize('k', range(len(CASES)), ids=[c['name'] for c in CASES])
def test_command_line_in_process(libmpn, tmp_path, capfdbinary, k):
    """the argument names of the reference script; PIPE for the even cases, a gzip file for the odd ones"""
    from megapath_nano_amd import candidates
    case = CASES[k]
    files = pc.write_case(tmp_path, case)
    can_fn = 'PIPE' if k % 2 == 0 else str(tmp_path / 'out.can.gz')
    assert candidates.main(argv_of(case, files, can_fn)) == 0
    printed = capfdbinary.readouterr().out
    if can_fn == 'PIPE':
        assert printed.decode() == case['stdout']
    else:
        assert printed == b''
        with gzip.open(can_fn, 'rb') as f:
            assert f.read().decode() == case['stdout']


def test_the_tool_itself(libmpn, tmp_path):
    """bin/mpn-candidates as a process: once to standard output, once to a gzip file"""
    case = next(c for c in CASES if c['bed'] and 'ctgStart' in c['options'])
    files = pc.write_case(tmp_path, case)
    p = subprocess.run([sys.executable, TOOL] + argv_of(case, files, 'PIPE'), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr[-500:]
    assert p.stdout.decode() == case['stdout'] and case['stdout']
    case = CASES[0]
    files = pc.write_case(tmp_path, case)
    can_fn = str(tmp_path / 'tool.can.gz')
    p = subprocess.run([sys.executable, TOOL] + argv_of(case, files, can_fn), capture_output=True, timeout=300)
    assert p.returncode == 0 and p.stdout == b'', p.stderr[-500:]
    with gzip.open(can_fn, 'rb') as f:
        assert f.read().decode() == case['stdout']


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
CTG = 'ACGTTGCAAGCTTAGGCATC' * 10


def small(tmp_path, reads, contigs=None):
    contigs = contigs or [('c', CTG)]
    return pc.write_bam(tmp_path / 'in.bam', contigs, reads), pc.write_fasta(tmp_path / 'ref.fa', contigs)


def test_unsorted_input_is_refused(libmpn, tmp_path):
    from megapath_nano_amd import candidates
    reads = [pc.sam_line('a', 0, 'c', 31, 60, '20M', CTG[30:50]), pc.sam_line('b', 0, 'c', 11, 60, '20M', CTG[10:30])]
    bam_fn, ref_fn = small(tmp_path, reads)
    with pytest.raises(ValueError, match='record b: .*not sorted'):
        candidates.extract_variant_candidates(bam_fn, ref_fn, 'c', out=io.BytesIO())
    # a record that is not taken may stand anywhere
    reads[1] = pc.sam_line('b', 0x100, 'c', 11, 60, '20M', CTG[10:30])
    bam_fn, ref_fn = small(tmp_path, reads)
    assert candidates.extract_variant_candidates(bam_fn, ref_fn, 'c', min_coverage=1, out=io.BytesIO()) == 0


@pytest.mark.parametrize('min_coverage', [0, -1, 0.0])
def test_min_coverage_must_be_positive(libmpn, tmp_path, min_coverage):
    from megapath_nano_amd import candidates
    bam_fn, ref_fn = small(tmp_path, [pc.sam_line('a', 0, 'c', 31, 60, '20M', CTG[30:50])])
    with pytest.raises(ValueError, match='minCoverage'):
        candidates.extract_variant_candidates(bam_fn, ref_fn, 'c', min_coverage=min_coverage, out=io.BytesIO())


@pytest.mark.parametrize('extra', [['--gen4Training'], ['--var_fn', 'x.vcf'], ['--outputProb', '0.1']])
def test_training_options_are_refused(libmpn, tmp_path, capsys, extra):
    from megapath_nano_amd import candidates
    bam_fn, ref_fn = small(tmp_path, [pc.sam_line('a', 0, 'c', 31, 60, '20M', CTG[30:50])])
    assert candidates.main(['--bam_fn', bam_fn, '--ref_fn', ref_fn, '--ctgName', 'c'] + extra) == 2
    io_ = capsys.readouterr()
    assert 'training' in io_.err and io_.out == ''


def test_cg_placeholder_is_refused(libmpn, tmp_path):
    from megapath_nano_amd import candidates
    ctg = 'ACGT' * 10000
    n = 32768                                  # 65536 operations: one more than n_cigar_op holds
    reads = [pc.sam_line('first', 0, 'c', 1, 60, '50M', ctg[:50]), pc.sam_line('ultra', 0, 'c', 5, 60, '1M1I' * n, 'AG' * n)]
    bam_fn, ref_fn = small(tmp_path, reads, [('c', ctg)])
    with pytest.raises(ValueError, match='record ultra: .*CG tag'):
        candidates.extract_variant_candidates(bam_fn, ref_fn, 'c', out=io.BytesIO())


def test_code_0_under_m_and_no_bases_are_refused(libmpn, tmp_path):
    from megapath_nano_amd import candidates
    good = pc.sam_line('a', 0, 'c', 11, 60, '20M', CTG[10:30])
    bam_fn, ref_fn = small(tmp_path, [good, pc.sam_line('eq', 0, 'c', 31, 60, '4S16M', CTG[30:40] + '=' + CTG[41:50])])
    with pytest.raises(ValueError, match='record eq: .*code 0'):
        candidates.extract_variant_candidates(bam_fn, ref_fn, 'c', out=io.BytesIO())
    # '=' under a soft clip or an insertion is never looked at
    bam_fn, ref_fn = small(tmp_path, [good, pc.sam_line('eq', 0, 'c', 31, 60, '2S8M1I9M', '=' + CTG[31:40] + '=' + CTG[41:50])])
    assert candidates.extract_variant_candidates(bam_fn, ref_fn, 'c', min_coverage=1, out=io.BytesIO()) >= 0
    bam_fn, ref_fn = small(tmp_path, [good, pc.sam_line('nb', 0, 'c', 31, 60, '20M', '*')])
    with pytest.raises(ValueError, match='record nb: '):
        candidates.extract_variant_candidates(bam_fn, ref_fn, 'c', out=io.BytesIO())


def test_contig_missing_from_the_bed_or_the_fasta(libmpn, tmp_path):
    from megapath_nano_amd import candidates
    bam_fn, ref_fn = small(tmp_path, [pc.sam_line('a', 0, 'c', 31, 60, '20M', CTG[30:50])])
    bed = tmp_path / 'x.bed'
    bed.write_text('other\t0\t100\n')
    with pytest.raises(ValueError, match=r'ctg_name\(c\) not exists in bed file'):
        candidates.extract_variant_candidates(bam_fn, ref_fn, 'c', bed_fn=str(bed), out=io.BytesIO())
    with pytest.raises(ValueError, match='Failed to load reference'):
        candidates.extract_variant_candidates(bam_fn, ref_fn, 'nowhere', out=io.BytesIO())
    assert candidates.main(['--bam_fn', bam_fn, '--ref_fn', ref_fn, '--ctgName', 'c', '--bed_fn', str(bed)]) == 1
