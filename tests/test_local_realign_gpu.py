"""GPU tests (-m gpu) of the local realignment (megapath_nano_amd/local_realign.py, csrc/local_realign_kernels.hip) against the
restatement (tests/local_realign_ref.py) and the goldens that the reference's own programs wrote: every line byte for byte, no
site omitted except those the rules leave out."""
import io
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest

import local_realign_cases as lc
import local_realign_ref as ref
import pileup_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'bin', 'mpn-local-realign')


@pytest.fixture(scope='module')
def lr(libmpn, oracle_built):
    from megapath_nano_amd import local_realign
    return local_realign


@pytest.fixture(autouse=True)
def default_groups(monkeypatch):
    monkeypatch.delenv('MPN_INGEST_BATCH_BYTES', raising=False)
    monkeypatch.delenv('MPN_LR_SSW_CHUNK', raising=False)


_SSW = {}


def cached_ssw(query, window):
    key = (query, window)
    if key not in _SSW:
        _SSW[key] = ref.oracle_ssw(query, window)
    return _SSW[key]


def got_lines(lr, tmp_path, seq, lines, positions, name='case'):
    bam_fn, ref_fn, _ = lc.write_case(tmp_path, dict(seq=seq, lines=lines), name)
    out = io.BytesIO()
    lr.local_realignment(bam_fn, ref_fn, lc.CTG, positions, out)
    return out.getvalue().decode()


def want_lines(seq, lines, positions):
    return ref.lines([ref.ccr.read_of(l) for l in lines], seq, lc.CTG, positions, ssw=cached_ssw)


def by_start(lines):
    return sorted(lines, key=lambda l: int(l.split('\t')[3]))


# ---- the goldens ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', lc.golden_cases(), ids=lambda c: c['name'])
def test_files_give_the_golden_lines_and_the_golden_vcf(lr, tmp_path, case, capsys):
    """SNP, insertion, deletion, both strands, bases that are not ACGT, flags, missing columns before and behind the centre, the
    edges of the window (reads from pos-200, pos+200 and pos+201, one up to pos-201, insertions behind pos-201 and pos+200, deletions
    over the window's start and over pos, an insertion spelled at a deleted column), position 301, 100 bases before the contig's end"""
    bam_fn, ref_fn, vcf_fn = lc.write_case(tmp_path, case)
    out = io.BytesIO()
    n = lr.local_realignment(bam_fn, ref_fn, lc.CTG, case['positions'], out)
    assert out.getvalue().decode() == case['expected_lines'] and n == len(set(case['positions']))
    capsys.readouterr()
    out_fn = os.path.join(str(tmp_path), 'out.vcf')
    lr.extract_vcf_position(vcf_fn, out.getvalue(), out_fn)
    with open(out_fn) as f:
        assert f.read() == case['expected_vcf']
    assert capsys.readouterr().out == case['expected_stdout']


def test_the_deep_golden_where_the_real_depth_rule_acts(lr, tmp_path, capsys):
    """11200 reads over eight starts, recorded with the real mpileup -d 8000"""
    case = lc.deep_golden()
    bam_fn, ref_fn, vcf_fn = lc.write_case(tmp_path, case)
    out = io.BytesIO()
    lr.local_realignment(bam_fn, ref_fn, lc.CTG, case['positions'], out)
    assert out.getvalue().decode() == case['expected_lines']
    lr.extract_vcf_position(vcf_fn, out.getvalue(), os.path.join(str(tmp_path), 'out.vcf'))
    with open(os.path.join(str(tmp_path), 'out.vcf')) as f:
        assert f.read() == case['expected_vcf']
    assert capsys.readouterr().out == case['expected_stdout']


# ---- sites and reads -----------------------------------------------------------------------------------------------------------------
def grid(n_sites, per_site, seed=5, sub=0.02):
    rng = random.Random(seed)
    seq = pc.random_contig(rng, 1200 + 600 * max(n_sites, 1))
    sites = [900 + 600 * c for c in range(n_sites)]
    lines = []
    for c, pos in enumerate(sites):
        for i in range(per_site):
            a = rng.randrange(20, 90)
            cig = rng.choice([f'{a}M{160 - a}M', f'{a}M2I{158 - a}M', f'{a}M3D{157 - a}M'])
            lines.append(lc.span_read(rng, seq, f's{c}_{i}', pos - a - rng.randrange(0, 30), cig, flag=16 * (i & 1), sub=sub if i % 3 == 0 else 0.0))
    return seq, by_start(lines), sites


@pytest.mark.parametrize('n_sites,per_site', [(0, 1), (1, 0), (1, 1), (1, 64), (2, 65), (63, 1), (64, 2), (65, 1)])
def test_sites_and_reads(lr, tmp_path, n_sites, per_site, capsys):
    """every site has its line, or is one at which the script raises and says so"""
    seq, lines, sites = grid(n_sites, per_site)
    want = want_lines(seq, lines, sites)
    assert got_lines(lr, tmp_path, seq, lines, sites) == want
    assert want.count('\n') + capsys.readouterr().err.count('the reference script raises there') == n_sites and want.count('\n') >= n_sites - 1


@pytest.mark.parametrize('seed', range(100, 106))
def test_random_read_sets(lr, tmp_path, seed, capsys):
    """indels, clips, N and IUPAC bases, gaps, an insertion right before and behind a deletion; sites at which the script's parser
    raises are left out with a message"""
    from test_local_realign_ref import random_set
    seq, reads = random_set(seed)
    lines = [pc.sam_line(f'q{i}', r[0], lc.CTG, r[1] + 1, 60, ''.join('%d%s' % (n, op) for op, n in r[2]), r[3]) for i, r in enumerate(reads)]
    want = want_lines(seq, lines, [700, 640, 790])
    assert got_lines(lr, tmp_path, seq, lines, [700, 640, 790]) == want
    assert capsys.readouterr().err.count('left out') == 3 - want.count('\n')


# ---- the depth rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('starts', ['one', 'distinct', 'mixed'])
@pytest.mark.parametrize('n', [7999, 8000, 8001])
def test_the_depth_rule(lr, tmp_path, n, starts):
    rng = random.Random(9)
    seq = pc.random_contig(rng, 2000)
    pos = 1000
    if starts == 'one':
        lines = lc.pile(seq, pos - 30, n)
    elif starts == 'distinct':                       # 40 neighbouring starts: all of them alive at the last
        lines = by_start([l for k in range(40) for l in lc.pile(seq, pos - 50 + k, n // 40 + (1 if k < n % 40 else 0), name=f'd{k}_')])
    else:                                            # a deep start, then first reads of their starts: those are piled up beyond 8000
        lines = lc.pile(seq, pos - 40, n) + [l for k in range(6) for l in lc.pile(seq, pos - 30 + 3 * k, 1, name=f'm{k}_')]
    reads = [ref.ccr.read_of(l) for l in lines]
    kept = len(ref.members(reads, pos))
    assert kept == {'one': min(n, 8000), 'distinct': min(n, 8000), 'mixed': min(n, 8000) + 6}[starts]
    want = want_lines(seq, lines, [pos])
    assert got_lines(lr, tmp_path, seq, lines, [pos]) == want and want.split('\t')[2] == str(kept)


# ---- fragments of every SSW class ------------------------------------------------------------------------------------------------------
def test_ssw_size_classes(lr, tmp_path):
    """fragments of 255 / 256 / 257 and 511 / 512 / 513 bytes, and one of more than 2048 bytes from a long insertion"""
    rng = random.Random(12)
    seq = pc.random_contig(rng, 2000)
    pos, lo = 1000, 800
    lines = [lc.span_read(rng, seq, 'bg', 500, '1000M')]
    for n in (255, 256, 257):
        lines.append(lc.span_read(rng, seq, f'f{n}', lo, f'{n}M'))
    for n in (511, 512, 513):
        lines.append(lc.span_read(rng, seq, f'f{n}', lo, f'210M{n - 401}I300M'))
    lines.append(lc.span_read(rng, seq, 'long', lo, '205M1700I300M'))
    lines = by_start(lines)
    reads = [ref.ccr.read_of(l) for l in lines]
    sizes = sorted(len(f) for f in ref.fragments(reads, pos))
    assert sizes == [255, 256, 257, 401, 511, 512, 513, 2101]
    assert got_lines(lr, tmp_path, seq, lines, [pos]) == want_lines(seq, lines, [pos])


# ---- a pair with score 0 ---------------------------------------------------------------------------------------------------------------
def score0_case(first):
    rng = random.Random(21)
    seq = ''.join(rng.choice('CGT') for _ in range(2000))                # no A anywhere: a fragment of A alone scores 0
    pos = 1000
    lines = [lc.span_read(rng, seq, f'n{i}', 880 + 7 * i, '300M') for i in range(5)]
    lines.append(pc.sam_line('zero', 0, lc.CTG, 850 if first else 950, 60, '12M', 'A' * 12))
    return seq, by_start(lines), pos


def test_a_pair_with_score_0_contributes_nothing(lr, tmp_path):
    seq, lines, pos = score0_case(first=False)
    detail = []
    ref.site([ref.ccr.read_of(l) for l in lines], seq, pos, detail=detail)
    assert [isinstance(res, tuple) and res[0] > 0 for f, res in detail if f == 'A' * 12] == [False]       # (score 0: ssw.c's result is undefined)
    want = want_lines(seq, lines, [pos])
    assert got_lines(lr, tmp_path, seq, lines, [pos]) == want and want.split('\t')[2] == '5'


def test_a_site_whose_first_read_scores_0_is_left_out(lr, tmp_path, capsys):
    seq, lines, pos = score0_case(first=True)
    with pytest.raises(ref.SiteRaises):
        ref.site([ref.ccr.read_of(l) for l in lines], seq, pos)
    assert got_lines(lr, tmp_path, seq, lines, [pos, pos + 400]) == want_lines(seq, lines, [pos + 400])
    assert 'score 0' in capsys.readouterr().err


# ---- where a site lies -----------------------------------------------------------------------------------------------------------------
def test_positions_300_and_301_and_the_contig_end(lr, tmp_path, capsys):
    start = next(c for c in lc.golden_cases() if c['name'] == 'contig_start')
    got = got_lines(lr, tmp_path, start['seq'], start['lines'], [300, 301, 1, 5000])
    assert got == start['expected_lines'].splitlines(keepends=True)[0] and got.split('\t')[1] == '301'
    err = capsys.readouterr().err
    assert ':300:' in err and ':1:' in err and ':5000:' in err
    end = next(c for c in lc.golden_cases() if c['name'] == 'contig_end')
    assert len(end['seq']) - 1500 == 100 and got_lines(lr, tmp_path, end['seq'], end['lines'], [1500], 'end') == end['expected_lines'].splitlines(keepends=True)[0]


# ---- text groups -----------------------------------------------------------------------------------------------------------------------
def test_a_second_text_group_and_twice_the_same(lr, tmp_path, monkeypatch):
    seq, lines, sites = grid(40, 30, seed=8)                   # (several BGZF blocks)
    want = want_lines(seq, lines, sites)
    a = got_lines(lr, tmp_path, seq, lines, sites)
    b = got_lines(lr, tmp_path, seq, lines, sites)
    assert a == b == want
    for size, chunk in (('4096', '1'), ('20000', '40')):
        monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', size)
        monkeypatch.setenv('MPN_LR_SSW_CHUNK', chunk)
        timings = {}
        bam_fn, ref_fn, _ = lc.write_case(tmp_path, dict(seq=seq, lines=lines), 'groups' + size)
        info = lr.alt_info(bam_fn, ref_fn, lc.CTG, sites, timings=timings)
        assert ''.join(lr.format_line(lc.CTG, p, d, m) for p, (d, m) in info.items()) == want
        assert timings['pairs'] == len(lines)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def write_patched(path, seq, lines, patch):
    """a BAM whose records go through patch(index, record bytes) -> record bytes"""
    from megapath_nano_amd import bam
    ref_id = {lc.CTG: 0}
    recs = []
    for i, line in enumerate(lines):
        tid, pos0, end0, flag, rec = bam.encode_record(line.split('\t'), ref_id)
        recs.append((tid, pos0, end0, flag, patch(i, rec)))
    bam.write_bam(str(path), f'@SQ\tSN:{lc.CTG}\tLN:{len(seq)}\n', [lc.CTG], [len(seq)], iter(recs))
    return str(path)


@pytest.mark.parametrize('what,match', [('N', 'N or P'), ('P', 'N or P'), ('code', 'above 8'), ('nobases', 'without bases'), ('eq', 'base `=`'),
                                        ('short', 'past the bases'), ('paired', 'paired'), ('unsorted', 'not sorted')])
def test_refusals(lr, tmp_path, what, match):
    rng = random.Random(31)
    seq = pc.random_contig(rng, 1500)
    pos = 700
    good = [lc.span_read(rng, seq, f'g{i}', 600 + i, '200M') for i in range(3)]
    bad = {'N': lc.span_read(rng, seq, 'bad', 650, '40M10N40M'), 'P': lc.span_read(rng, seq, 'bad', 650, '40M2P2I40M'),
           'code': lc.span_read(rng, seq, 'bad', 650, '40M2I40M'), 'nobases': pc.sam_line('bad', 0, lc.CTG, 650, 60, '80M', '*'),
           'eq': lc.mutate(lc.span_read(rng, seq, 'bad', 650, '80M'), 55, '='), 'short': pc.sam_line('bad', 0, lc.CTG, 650, 60, '80M', seq[649:700]),
           'paired': lc.span_read(rng, seq, 'bad', 650, '80M', flag=1), 'unsorted': lc.span_read(rng, seq, 'bad', 400, '80M')}[what]
    lines = good + [bad] if what == 'unsorted' else by_start(good + [bad])
    at = next(i for i, l in enumerate(lines) if l.startswith('bad\t'))

    def patch(i, rec):
        if what != 'code' or i != at:
            return rec
        cigar = 32 + rec[8]                          # (l_read_name is the ninth byte of a record without its size word)
        word, = struct.unpack_from('<I', rec, cigar + 4)
        return rec[:cigar + 4] + struct.pack('<I', (word & ~15) | 9) + rec[cigar + 8:]
    bam_fn = write_patched(os.path.join(str(tmp_path), 'bad.bam'), seq, lines, patch)
    ref_fn = pc.write_fasta(os.path.join(str(tmp_path), 'ref.fa'), [(lc.CTG, seq)])
    with pytest.raises(ValueError, match=match) as e:
        lr.alt_info(bam_fn, ref_fn, lc.CTG, [pos])
    assert what == 'unsorted' or 'record bad' in str(e.value)
    # outside every region the same record is not looked at
    if what not in ('unsorted',):
        assert list(lr.alt_info(bam_fn, ref_fn, lc.CTG, [1250])) == [1250]


# ---- the resident SSW entry ------------------------------------------------------------------------------------------------------------
def resident(lr, reads, refs, masks, mat, score_size, gap_open, gap_extend, flag, filters, filterd):
    """mpn_ssw_align_resident on pairs that are uploaded with torch -> one dict per pair, as ssw_batch.ssw_align_batch gives them"""
    import torch
    n = len(reads)
    rl, fl = np.array([len(r) for r in reads], dtype=np.int32), np.array([len(r) for r in refs], dtype=np.int32)
    ro, fo = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    ro[1:], fo[1:] = np.cumsum(rl[:-1]), np.cumsum(fl[:-1])
    d_reads = torch.from_numpy(np.concatenate(reads).astype(np.int8)).cuda()
    d_refs = torch.from_numpy(np.concatenate(refs).astype(np.int8)).cuda()
    cap = int(rl.sum() + fl.sum() + 8 * n)
    d_res, d_cig = torch.zeros(9 * n, dtype=torch.int32, device='cuda'), torch.zeros(cap, dtype=torch.int32, device='cuda')
    mat, mask = np.ascontiguousarray(mat, dtype=np.int8), np.ascontiguousarray(masks, dtype=np.int32)
    coff, clen, status = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    torch.cuda.synchronize()
    rc = lr._lib().mpn_ssw_align_resident(n, d_reads.data_ptr(), ro.ctypes.data, rl.ctypes.data, d_refs.data_ptr(), fo.ctypes.data, fl.ctypes.data,
                                          mat.ctypes.data, 5, score_size, gap_open, gap_extend, flag, filters, filterd, mask.ctypes.data, d_res.data_ptr(),
                                          d_cig.data_ptr(), cap, coff.ctypes.data, clen.ctypes.data, status.ctypes.data)
    assert rc == 0
    res, cig = d_res.cpu().numpy().reshape(9, n), d_cig.cpu().numpy().view(np.uint32)
    out = []
    for i in range(n):
        assert int(res[7, i]) == int(status[i])
        if status[i] in (3, 4) or (status[i] == 1 and not 0 <= score_size <= 2):       # refused before the launch: the batch entry's fixed row
            out.append(dict(score1=0, score2=0, ref_begin1=-1, ref_end1=0, read_begin1=-1, read_end1=0, ref_end2=0, cigar=[], status=int(status[i])))
            continue
        out.append(dict(score1=int(res[0, i]) & 0xffff, score2=int(res[1, i]) & 0xffff, ref_begin1=int(res[2, i]), ref_end1=int(res[3, i]),
                        read_begin1=int(res[4, i]), read_end1=int(res[5, i]), ref_end2=int(res[6, i]), cigar=[int(x) for x in cig[coff[i]:coff[i] + clen[i]]],
                        status=int(status[i])))
    return out


def test_the_resident_ssw_entry_equals_the_batch_entry(lr, libmpn):
    """the seeded cases of tests/ssw_cases.py: each with its own options, and all pairs in one call with the options of the realignment"""
    from megapath_nano_amd.ssw_batch import ssw_align_batch
    from ssw_cases import make_cases
    cases = make_cases(11, 24)
    with_cigar = 0
    for c in cases:
        opts = (c['mat'], c['score_size'], c['gap_open'], c['gap_extend'], c['flag'], c['filters'], c['filterd'])
        want = ssw_align_batch([c['read']], [c['ref']], opts[0], 5, *opts[1:], [c['mask']])
        assert resident(lr, [c['read']], [c['ref']], [c['mask']], *opts) == want
        with_cigar += bool(want[0]['cigar'])
    assert with_cigar > 4
    reads, refs = [c['read'] for c in cases], [c['ref'] for c in cases]
    masks = [15 if len(r) <= 30 else len(r) for r in reads]
    opts = (ref.MAT, 2, 8, 2, 2, 0, 0)
    want = ssw_align_batch(reads, refs, opts[0], 5, *opts[1:], masks)
    assert resident(lr, reads, refs, masks, *opts) == want and all(w['cigar'] for w in want if w['score1'] > 0)


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_the_command_line_end_to_end(lr, tmp_path):
    case = next(c for c in lc.golden_cases() if c['name'] == 'indel')
    bam_fn, ref_fn, vcf_fn = lc.write_case(tmp_path, case)
    with open(vcf_fn, 'a') as f:
        f.write('other\t5\t.\tA\tC\t100\t.\t.\tGT:GQ:DP:AF\t0/1:100:30:0.5000\n')
    out = os.path.join(str(tmp_path), 'out')
    p = subprocess.run([sys.executable, TOOL, '-b', bam_fn, '-v', vcf_fn, '-r', ref_fn, '-c', lc.CTG, '-p', 'ont', '-o', out, '-t', '4'], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    with open(os.path.join(out, 'tmp', '0_all_alt_info')) as f:
        assert f.read() == case['expected_lines']
    with open(os.path.join(out, '0_realign.vcf')) as f:
        assert f.read() == case['expected_vcf'] + '\nother\t5\t.\tA\tC\t100\t.\t.\tGT:GQ:DP:AF\t0/1:100:30:0.5000'
    assert p.stdout == case['expected_stdout']
    p = subprocess.run([sys.executable, TOOL, '-b', bam_fn, '-v', vcf_fn, '-r', ref_fn, '-c', lc.CTG, '-p', 'illumina', '-o', out], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 2 and 'illumina' in p.stderr
    # a VCF without a row of the contig: nothing to realign, the rows pass through
    only = os.path.join(str(tmp_path), 'only.vcf')
    with open(only, 'w') as f:
        f.write('#CHROM\tPOS\nother\t5\t.\tA\tC\t100\t.\t.\tGT:GQ:DP:AF\t0/1:100:30:0.5000\n')
    p = subprocess.run([sys.executable, TOOL, '-b', bam_fn, '-v', only, '-r', ref_fn, '-c', lc.CTG, '-p', 'ont', '-o', out + '2'], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr
    with open(os.path.join(out + '2', '0_realign.vcf')) as f:
        assert f.read() == '#CHROM\tPOS\nother\t5\t.\tA\tC\t100\t.\t.\tGT:GQ:DP:AF\t0/1:100:30:0.5000'
