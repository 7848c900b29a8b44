"""GPU tests (-m gpu) of the tensor creation (megapath_nano_amd/clair_tensor.py, bin/mpn-create-tensor): on every golden case
(tests/golden/tensors: the inputs, the seed and the bytes Clair's own CreateTensor.py printed for them) the drop-in writes the
reference's bytes, through the function, through the command line and through the tool as a child process, to standard output and to
a gzip file, from a pipe of bin/mpn-candidates, and from a BAM cut into several texts; and what it refuses."""
import gzip
import io
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import pileup_cases as pc
import tensor_cases as tc
import tensor_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'bin', 'mpn-create-tensor')
CANDIDATES = os.path.join(ROOT, 'bin', 'mpn-candidates')
CASES = tc.golden_cases()
CTG = 'ctgT'
# runs the tool as the golden generator runs the reference script: a child whose `random` is seeded first
SEEDED = 'import random, runpy, sys\nrandom.seed(int(sys.argv[1]))\nsys.argv = sys.argv[2:]\nrunpy.run_path(sys.argv[0], run_name="__main__")\n'


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    monkeypatch.delenv('MPN_INGEST_BATCH_BYTES', raising=False)
    monkeypatch.delenv('MPN_BAM_WALK_RECORDS', raising=False)


def call(case, files, out=None, rng=None, **more):
    from megapath_nano_amd import clair_tensor
    kw = tc.keywords(case)
    kw.update(more)
    return clair_tensor.create_tensor(files[0], files[1], io.StringIO(tc.candidate_text(case)), case['contigs'][0][0],
                                      consider_left_edge=not case['options'].get('stop_consider_left_edge', False),
                                      rng=rng or random.Random(case['seed']), out=out, **kw)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_function_writes_the_reference_bytes(libmpn, tmp_path, case):
    out = io.BytesIO()
    n = call(case, tc.write_case(tmp_path, case), out)
    assert out.getvalue().decode() == case['stdout']
    assert n == len(case['stdout'].splitlines())


@pytest.mark.parametrize('name', ['ops', 'ends', 'region', 'deep_250', 'deep_1000_scattered'])
def test_tensors_stay_resident(libmpn, tmp_path, name):
    from megapath_nano_amd import clair_tensor
    case = tc.case_named(name)
    bam_fn, ref_fn = tc.write_case(tmp_path, case)
    centres, block, strings = clair_tensor.tensors(bam_fn, ref_fn, np.array(case['positions']), CTG, rng=random.Random(case['seed']), **tc.keywords(case))
    assert block.is_cuda and tuple(block.shape) == (len(centres), 33, 8, 4) and str(block.dtype) == 'torch.int32'
    got = ''.join(ref.line(CTG, c, s, t) for c, s, t in zip(centres, strings, block.cpu().numpy()))
    assert got == case['stdout']


@pytest.mark.parametrize('k', range(len(CASES)), ids=[c['name'] for c in CASES])
def test_command_line_in_process(libmpn, tmp_path, capfdbinary, monkeypatch, k):
    """the argument names of the reference script; PIPE both ways for the even cases, gzip files for the odd ones"""
    from megapath_nano_amd import clair_tensor
    case = CASES[k]
    bam_fn, ref_fn = tc.write_case(tmp_path, case)
    argv = ['--bam_fn', bam_fn, '--ref_fn', ref_fn, '--ctgName', CTG, '--samtools', '/nowhere/samtools'] + tc.argv(case)
    tensor_fn = 'PIPE'
    if k % 2 == 0:
        monkeypatch.setattr(sys, 'stdin', io.StringIO(tc.candidate_text(case)))
        argv += ['--can_fn', 'PIPE']
    else:
        tensor_fn = str(tmp_path / 'out.tensor.gz')
        with gzip.open(tmp_path / 'in.can.gz', 'wt') as f:
            f.write(tc.candidate_text(case))
        argv += ['--can_fn', str(tmp_path / 'in.can.gz'), '--tensor_fn', tensor_fn]
    random.seed(case['seed'])
    assert clair_tensor.main(argv) == 0
    printed = capfdbinary.readouterr().out
    if tensor_fn == 'PIPE':
        assert printed.decode() == case['stdout']
    else:
        assert printed == b''
        with gzip.open(tensor_fn, 'rb') as f:
            assert f.read().decode() == case['stdout']


@pytest.mark.parametrize('name', ['ops_no_left_edge', 'region', 'deep_250'])
def test_the_tool_itself(libmpn, tmp_path, name):
    case = tc.case_named(name)
    bam_fn, ref_fn = tc.write_case(tmp_path, case)
    cmd = [sys.executable, '-c', SEEDED, str(case['seed']), TOOL, '--bam_fn', bam_fn, '--ref_fn', ref_fn, '--ctgName', CTG] + tc.argv(case)
    p = subprocess.run(cmd, input=tc.candidate_text(case).encode(), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert p.stdout.decode() == case['stdout']


def test_no_arguments_print_the_help(libmpn):
    p = subprocess.run([sys.executable, TOOL], capture_output=True, timeout=300)
    assert p.returncode == 1 and b'--stop_consider_left_edge' in p.stdout


@pytest.fixture(scope='module')
def variant(tmp_path_factory):
    """twelve reads over one position where six of them differ, and four more reads with an insertion: shallow, so no draw shows"""
    rng = random.Random(5)
    ctg = pc.random_contig(rng, 300)
    lines = []
    for i in range(12):
        seq = list(ctg[80:140])
        if i < 6:
            seq[19] = 'A' if ctg[99] != 'A' else 'C'
        lines.append(tc.sam_line(f'v{i}', 16 if i & 1 else 0, CTG, 81, 60, '60M', ''.join(seq)))
    for i in range(4):
        lines.append(tc.sam_line(f'w{i}', 0, CTG, 101, 60, '30M2I30M', ctg[100:130] + 'GG' + ctg[130:160]))
    d = tmp_path_factory.mktemp('variant')
    return pc.write_bam(d / 'in.bam', [(CTG, ctg)], lines), pc.write_fasta(d / 'ref.fa', [(CTG, ctg)]), ctg


def test_pipe_from_the_candidate_tool(libmpn, variant):
    bam_fn, ref_fn, ctg = variant
    common = ['--bam_fn', bam_fn, '--ref_fn', ref_fn, '--ctgName', CTG]
    first = subprocess.Popen([sys.executable, CANDIDATES] + common + ['--minCoverage', '4'], stdout=subprocess.PIPE)
    second = subprocess.run([sys.executable, TOOL] + common, stdin=first.stdout, capture_output=True, timeout=300)
    first.stdout.close()
    assert first.wait(timeout=300) == 0 and second.returncode == 0, second.stderr.decode()[-2000:]
    lines = subprocess.run([sys.executable, CANDIDATES] + common + ['--minCoverage', '4'], capture_output=True, timeout=300).stdout.decode()
    positions = [int(l.split()[1]) for l in lines.splitlines()]
    assert 100 in positions and len(positions) >= 2
    assert second.stdout.decode() == ref.lines(pc.text_of(bam_fn), ctg, positions, CTG, rng=random.Random(0))


def test_several_texts_give_the_same_bytes(libmpn, tmp_path, monkeypatch):
    """1000 reads on one POS: three BGZF blocks, a text each, and the deep centre needs the records of all of them"""
    from megapath_nano_amd import ingest
    case = tc.case_named('deep_1000_scattered')
    files = tc.write_case(tmp_path, case)
    assert len(pc.text_of(files[0])) > 2 * 65536
    monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', '1')
    monkeypatch.setenv('MPN_BAM_WALK_RECORDS', '50')
    texts, real = [], ingest._BgzfTexts.next_text

    def counted(self, carry):
        got = real(self, carry)
        texts.append(got[1])
        return got
    monkeypatch.setattr(ingest._BgzfTexts, 'next_text', counted)
    out = io.BytesIO()
    call(case, files, out)
    assert len(texts) >= 3 and texts[-1] > texts[0]          # the carry grows: the centre keeps its records
    assert out.getvalue().decode() == case['stdout']


def test_several_texts_finish_centres_on_the_way(libmpn, tmp_path, monkeypatch):
    """reads along a contig with candidates every 50 bases: centres are finished text by text, the draws stay in order"""
    from megapath_nano_amd import clair_tensor
    rng = random.Random(9)
    ctg = pc.random_contig(rng, 6000)
    lines, starts = [], sorted(rng.randrange(0, 5000) for _ in range(900))
    for i, s in enumerate(starts):
        cigar = rng.choice(['400M', '100M3I200M2D97M', '5S395M', '150M20D230M'])
        lines.append(tc.sam_line(f'r{i}', 16 if i & 1 else 0, CTG, s + 1, 60, cigar, pc.read_for(rng, ctg, s, cigar)))
    bam_fn, ref_fn = pc.write_bam(tmp_path / 'in.bam', [(CTG, ctg)], lines), pc.write_fasta(tmp_path / 'ref.fa', [(CTG, ctg)])
    positions = list(range(40, 5400, 50))
    want = ref.lines(pc.text_of(bam_fn), ctg, positions, CTG, rng=random.Random(3), dcov=2)
    whole = io.BytesIO()
    clair_tensor.create_tensor(bam_fn, ref_fn, np.array(positions), CTG, dcov=2, rng=random.Random(3), out=whole)
    assert whole.getvalue().decode() == want and want.count('\n') > 100
    monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', '1')
    monkeypatch.setenv('MPN_BAM_WALK_RECORDS', '33')
    timings, cut = {}, io.BytesIO()
    clair_tensor.create_tensor(bam_fn, ref_fn, np.array(positions), CTG, dcov=2, rng=random.Random(3), out=cut, timings=timings)
    assert len(pc.text_of(bam_fn)) > 3 * 65536
    assert cut.getvalue().decode() == want


# ---- what is refused --------------------------------------------------------------------------------------------------------------
def small(tmp_path, lines, ctg_len=300, fasta_len=None, fasta_name=CTG):
    ctg = pc.random_contig(random.Random(1), ctg_len)
    return (pc.write_bam(tmp_path / 'in.bam', [(CTG, ctg_len)], lines), pc.write_fasta(tmp_path / 'ref.fa', [(fasta_name, ctg[:fasta_len or ctg_len])]))


def refused(files, positions, match, **kw):
    from megapath_nano_amd import clair_tensor
    with pytest.raises(ValueError, match=match):
        clair_tensor.create_tensor(files[0], files[1], np.array(positions), CTG, out=io.BytesIO(), **kw)


def test_candidates_that_are_not_ascending(libmpn, tmp_path):
    from megapath_nano_amd import clair_tensor
    files = small(tmp_path, [tc.sam_line('a', 0, CTG, 81, 60, '60M', 'A' * 60)])
    refused(files, [120, 100], 'ascending')
    out = io.BytesIO()
    assert clair_tensor.create_tensor(files[0], files[1], np.array([100, 100, 120]), CTG, out=out) == 2          # duplicates are merged


def test_unsorted_records(libmpn, tmp_path):
    lines = [tc.sam_line('a', 0, CTG, 91, 60, '60M', 'A' * 60), tc.sam_line('b', 0, CTG, 81, 60, '60M', 'A' * 60)]
    refused(small(tmp_path, lines), [100], 'not sorted')


def test_cg_placeholder(libmpn, tmp_path):
    lines = [tc.sam_line('a', 0, CTG, 81, 60, '60S100N', 'A' * 60)]
    refused(small(tmp_path, lines), [100], 'CG tag')


def test_contig_missing_from_the_fasta(libmpn, tmp_path):
    files = small(tmp_path, [tc.sam_line('a', 0, CTG, 81, 60, '60M', 'A' * 60)], fasta_name='other')
    refused(files, [100], 'reference')


@pytest.mark.parametrize('seq, qual, what', [('*', '*', 'without bases'), ('A' * 60, '*', 'without qualities')])
def test_a_read_without_bases_or_qualities_in_a_window(libmpn, tmp_path, seq, qual, what):
    from megapath_nano_amd import clair_tensor
    files = small(tmp_path, [tc.sam_line('a', 0, CTG, 81, 60, '60M', seq, qual)])
    refused(files, [100], 'without bases or without qualities')
    assert clair_tensor.create_tensor(files[0], files[1], np.array([250]), CTG, out=io.BytesIO()) == 0      # no window: the script passes too


def test_a_read_past_the_end_of_the_reference(libmpn, tmp_path):
    from megapath_nano_amd import clair_tensor
    files = small(tmp_path, [tc.sam_line('a', 0, CTG, 81, 60, '60M', 'A' * 60)], fasta_len=130)
    refused(files, [120], 'past the end of the reference')
    # a window that the read has left before the sequence ends is written
    assert clair_tensor.create_tensor(files[0], files[1], np.array([90]), CTG, out=io.BytesIO()) == 1
