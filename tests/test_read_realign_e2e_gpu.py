"""GPU tests of megapath_nano_amd/read_realign.py from end to end: every record that the reference's unmodified script printed for
the golden cases (tests/golden/read_realign/) through realign_file; bin/mpn-realign-reads with a BAM as output (the records of the BAM
equal the text's, it is sorted, its .bai exists) and with PIPE, every refusal by the record's name, and the argument refusals of
the tool."""
import io
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import read_realign_cases as rc

GOLDEN, load = rc.GOLDEN, rc.load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'bin', 'mpn-realign-reads')


@pytest.fixture(scope='module')
def rr(libmpn):
    from megapath_nano_amd import read_realign
    return read_realign


def tool(*args):
    return subprocess.run([sys.executable, TOOL] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


@pytest.mark.parametrize('path', GOLDEN, ids=[os.path.basename(p)[:-8] for p in GOLDEN])
def test_golden_cases_through_realign_file(rr, tmp_path, path):
    gold, case = load(path)
    bam_fn, ref_fn = rc.write_case(tmp_path, case)
    out = io.BytesIO()
    got = rr.realign_file(bam_fn, ref_fn, rc.CTG, out, min_mq=gold['args']['minMQ'], min_coverage=gold['args']['minCoverage'])
    lines = out.getvalue().decode().splitlines(keepends=True)
    assert [l for l in lines if l[0] != '@'] == gold['records']
    assert [l for l in lines if l[0] == '@'] == gold['header']
    assert got['reads'] == len(gold['records']) and got['changed'] == gold['changed']


def test_the_tool_writes_the_text_and_the_same_records_as_a_sorted_bam(rr, tmp_path):
    from megapath_nano_amd import candidates, ingest
    case = rc.plain_variants()
    bam_fn, ref_fn = rc.write_case(tmp_path, case)
    out = io.BytesIO()
    got = rr.realign_file(bam_fn, ref_fn, rc.CTG, out)
    text = out.getvalue().decode()
    assert got['changed'] > 0 and text.startswith(rc.header_text(case))
    piped = tool('--bam_fn', bam_fn, '--ref_fn', ref_fn, '--ctgName', rc.CTG, '--samtools', 'nowhere', '--ctgStart', 5, '--ctgEnd', 9, '--threshold', 0.5,
                 '--chunk_id', 3, '--chunk_num', 7, '--test_pos', 4)
    assert piped.returncode == 0 and piped.stdout.decode() == text, piped.stderr.decode()
    out_bam = tmp_path / 'out.bam'
    done = tool('--bam_fn', bam_fn, '--ref_fn', ref_fn, '--ctgName', rc.CTG, '--read_fn', out_bam, '--minMQ', 5, '--minCoverage', 2)
    assert done.returncode == 0 and done.stdout == b'', done.stderr.decode()
    assert os.path.getsize(str(out_bam) + '.bai') > 0
    # the lines of the text, sorted as the BAM is (position, then strand; stable), against the records of the BAM
    lines = [l.split('\t') for l in text.splitlines() if not l.startswith('@')]
    assert all(l[11] == '' or l[11].startswith('HP:i:') for l in lines) and any(l[11] == '' for l in lines)
    order = sorted(range(len(lines)), key=lambda k: (int(lines[k][3]), (int(lines[k][1]) >> 4) & 1))
    reads = ingest.read_bam(str(out_bam))
    assert [r[0] for r in reads] == [lines[k][0] for k in order]
    assert [(r[1].decode(), r[2].decode()) for r in reads] == [(lines[k][9], lines[k][10]) for k in order]          # (no read of the case is reversed)
    with ingest.BamTexts(str(out_bam)) as texts:
        t = next(texts)
        assert t.final
        recs = candidates.pileup_records(t.text, t.text_len, t.rows)
        mine = rr.rr_records(t.text, t.text_len, t.rows)
    assert recs['pos'].tolist() == [int(lines[k][3]) - 1 for k in order] == sorted(recs['pos'].tolist())
    assert recs['mapq'].tolist() == [int(lines[k][4]) for k in order] and t.rows['flag'].tolist() == [int(lines[k][1]) for k in order]
    assert [chr(h) if h else '' for h in mine['hp'].tolist()] == [lines[k][11][5:] for k in order]
    for k, r in zip(order, recs):
        parsed = rc.ops_of(lines[k][5])
        assert r['n_cigar'] == len(parsed) and r['total'] == sum(n for n, _ in parsed) and r['soft'] == sum(n for n, c in parsed if c == 'S')


def test_a_contig_without_a_record(rr, tmp_path):
    from megapath_nano_amd import ingest
    case = rc.plain_variants()
    case = dict(case, name='empty', records=[dict(r, mapq=3) for r in case['records'][:5]])            # below --minMQ: not viewed
    bam_fn, ref_fn = rc.write_case(tmp_path, case)
    out = io.BytesIO()
    assert rr.realign_file(bam_fn, ref_fn, rc.CTG, out)['reads'] == 0 and out.getvalue() == b''
    got = rr.realign_to_bam(bam_fn, ref_fn, rc.CTG, str(tmp_path / 'none.bam'))
    assert got['reads'] == 0 and ingest.read_bam(str(tmp_path / 'none.bam')) == []
    assert rr.realign_file(bam_fn, ref_fn, rc.CTG, out, min_mq=0)['reads'] == 5


def set_op(rec):
    """the first CIGAR operation gets code 9"""
    at = 32 + rec[8]
    return rec[:at] + bytes([rec[at] & 0xf0 | 9]) + rec[at + 1:]


REFUSALS = [
    ('unsorted', dict(pos=300), None, 'not sorted'),
    ('no_bases', dict(seq='*', qual='*'), None, 'past the bases'),
    ('no_qualities', dict(qual='*'), None, 'no qualities'),
    ('base_eq', 'eq', None, 'a base `=`'),
    ('cigar_past_bases', dict(cigar='70M'), None, 'past the bases'),
    ('past_contig', dict(pos=2960), None, 'past the end of the contig'),           # (the last record of the file)
    ('bad_op', dict(), set_op, 'operation code above 8'),
    ('placeholder', dict(cigar='60S100N'), None, 'CG tag'),
    ('hp_text', dict(aux=[('XT', 'Z', 'seeHP:i:2')]), None, 'HP:i:'),
]


@pytest.mark.parametrize('name,change,patch,why', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_record_before_any_output(rr, tmp_path, name, change, patch, why):
    ctg, rng = rc.contig(3000, 51), random.Random(52)
    recs = [rc.read(ctg, 100 + 40 * k, '60M', rng, mism=(9,)) for k in range(20)]
    bad = rc.read(ctg, 560, '60M', rng)
    if change == 'eq':
        bad['seq'] = bad['seq'][:10] + '=' + bad['seq'][11:]
    else:
        bad.update(change)
    bad['patch'] = patch
    at = 20 if name == 'past_contig' else 12
    recs.insert(at, bad)                     # (case() is not used: the records stay in this order)
    case = dict(name=name, contig=ctg, records=recs, min_mq=5, min_coverage=2)
    bam_fn, ref_fn = rc.write_case(tmp_path, case)
    out = io.BytesIO()
    with pytest.raises(ValueError) as e:
        rr.realign_file(bam_fn, ref_fn, rc.CTG, out)
    assert f'record r{at}:' in str(e.value) and why in str(e.value), str(e.value)
    assert out.getvalue() == b''
    if name == 'unsorted':
        done = tool('--bam_fn', bam_fn, '--ref_fn', ref_fn, '--ctgName', rc.CTG)
        assert done.returncode == 1 and done.stdout == b'' and b'record r12:' in done.stderr


def test_a_dropped_record_is_not_refused_for_its_bases(rr, tmp_path):
    """a record without a CIGAR or with too much of it clipped takes an index and is not looked at any further"""
    ctg, rng = rc.contig(3000, 53), random.Random(54)
    recs = [rc.read(ctg, 100 + 40 * k, '60M', rng, mism=(9,)) for k in range(6)]
    recs.insert(2, dict(rc.read(ctg, 150, '*', rng, bases='*'), qual='*'))
    recs.insert(4, dict(rc.read(ctg, 200, '40S20M', rng), qual='*'))
    case = dict(name='dropped', contig=ctg, records=recs, min_mq=5, min_coverage=2)
    bam_fn, ref_fn = rc.write_case(tmp_path, case)
    out = io.BytesIO()
    assert rr.realign_file(bam_fn, ref_fn, rc.CTG, out)['reads'] == 6
    names = [l.split('\t')[0] for l in out.getvalue().decode().splitlines() if l[0] != '@']
    assert names == ['00000', '00001', '00003', '00005', '00006', '00007']


def test_the_tool_refuses_what_it_does_not_take(tmp_path):
    for args in (['--bed_fn', 'x.bed'], ['--extend_confident_bed_fn', 'x.bed']):
        done = tool('--bam_fn', 'x.bam', '--ref_fn', 'x.fa', '--ctgName', 'c', *args)
        assert done.returncode == 2 and done.stdout == b'' and b'not taken' in done.stderr
    assert tool().returncode == 1
    done = tool('--bam_fn', str(tmp_path / 'none.bam'), '--ref_fn', str(tmp_path / 'none.fa'), '--ctgName', 'c')
    assert done.returncode == 1 and done.stdout == b''
