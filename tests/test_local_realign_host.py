"""CPU test: the local-realignment arithmetic the kernels run (csrc/local_realign_core.h), built for the host with g++
(scripts/local_realign_host_check.cpp with oracle/ssw_oracle.c compiled in, under AddressSanitizer and UBSan where the toolchain has
their runtimes), takes the golden cases, a lowered depth rule and malformed records to the depths and mappings of the restatement
(tests/local_realign_ref.py) -- before any of them meets a GPU."""
import os
import random
import struct
import subprocess

import pytest

import local_realign_cases as lc
import local_realign_ref as ref
import pileup_cases as pc
from test_pileup_host import pack, raw_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAST, BAD_OP, SKIP_PAD, NO_BASES, EQ_BASE, PAST_BASES = range(1, 7)
M, I, D, N, S, H, P = range(7)


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp('lr_host')
    out, obj = d / 'local_realign_host_check', d / 'ssw_oracle.o'
    src, orc = os.path.join(ROOT, 'scripts', 'local_realign_host_check.cpp'), os.path.join(ROOT, 'oracle', 'ssw_oracle.c')
    for flags in (['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], ['-O2']):
        if subprocess.run(['gcc'] + flags + ['-c', orc, '-o', str(obj)]).returncode == 0 and \
                subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror'] + flags + ['-o', str(out), src, str(obj)]).returncode == 0:
            print('local_realign_host_check built with', ' '.join(flags))
            return out
    raise RuntimeError('the host check does not build')


def rows_of(text):
    """the records of an inflated BAM that mpileup may take on the first contig -> [(off, pos, end)]"""
    l_text, = struct.unpack_from('<i', text, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from('<i', text, at)
    at += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from('<i', text, at)
        at += 8 + l_name
    out = []
    while at < len(text):
        size, ref_id, pos, l_name, _, _, n_cigar, flag = struct.unpack_from('<iiiBBHHH', text, at)
        if ref_id == 0 and not (flag & ref.FILTER_FLAG):
            cigar = struct.unpack_from('<%dI' % n_cigar, text, at + 36 + l_name)
            rlen = sum(w >> 4 for w in cigar if (w & 15) in (0, 2, 3, 7, 8))
            out.append((at, pos, pos + max(rlen, 1)))
        at += 4 + size
    return out


def run(exe, tmp_path, cases):
    """cases: [(text, contig bytes, maxcnt, [(off, pos, end)], [site])] -> [[(state, bad row, depth, reads, {key: count})]]"""
    src, dst = tmp_path / 'cases.bin', tmp_path / 'results.bin'
    with open(src, 'wb') as f:
        f.write(struct.pack('<I', len(cases)))
        for text, contig, maxcnt, rows, sites in cases:
            f.write(struct.pack('<QQiII', len(text), len(contig), maxcnt, len(rows), len(sites)) + text + contig)
            f.write(b''.join(struct.pack('<qqq', *r) for r in rows) + b''.join(struct.pack('<i', s) for s in sites))
    subprocess.run([str(exe), str(src), str(dst)], check=True, timeout=300)
    blob, p, out = dst.read_bytes(), 0, []
    for text, contig, maxcnt, rows, sites in cases:
        per = []
        for _ in sites:
            state, bad, depth, reads, n_keys = struct.unpack_from('<iqiII', blob, p)
            p += 24
            keys = {}
            for _ in range(n_keys):
                count, n = struct.unpack_from('<iI', blob, p)
                keys[blob[p + 8:p + 8 + n].decode()] = count
                p += 8 + n
            per.append((state, bad, depth, reads, keys))
        out.append(per)
    assert p == len(blob)
    return out


def want_of(reads, seq, pos, maxcnt=ref.MAXCNT):
    """the restatement's depth and mapping with the contig's own base still in it, as the device leaves it"""
    return ref.site(reads, seq, pos, maxcnt=maxcnt, keep_ref=True)


def test_golden_cases_through_the_host_build(exe, tmp_path, oracle_built):
    cases = []
    for case in lc.golden_cases():
        text = pc.text_of(lc.write_case(tmp_path, case)[0])
        cases.append((text, case['seq'].encode(), ref.MAXCNT, rows_of(text), case['positions']))
    for case, got in zip(lc.golden_cases(), run(exe, tmp_path, cases)):
        reads = lc.reads_of(case)
        for pos, (state, bad, depth, n_reads, keys) in zip(case['positions'], got):
            want_depth, want = want_of(reads, case['seq'], pos)
            assert (state, depth) == (0, want_depth) and list(keys.items()) == list(want.items()) and n_reads == len(ref.fragments(reads, pos))
            gold = [l for l in case['expected_lines'].splitlines() if l.split('\t')[1] == str(pos)][0].split('\t')
            assert gold[2] == str(depth) and ref.json.loads(gold[3]) == {k: v for k, v in keys.items() if k != case['seq'][pos - 1]}


def test_the_deep_golden_through_the_host_build(exe, tmp_path, oracle_built):
    case = lc.deep_golden()
    text = pc.text_of(lc.write_case(tmp_path, case)[0])
    (state, bad, depth, n_reads, keys), = run(exe, tmp_path, [(text, case['seq'].encode(), ref.MAXCNT, rows_of(text), case['positions'])])[0]
    gold = case['expected_lines'].split('\t')
    assert state == 0 and str(depth) == gold[2] and {k: v for k, v in keys.items() if k != case['seq'][case['positions'][0] - 1]} == ref.json.loads(gold[3])
    assert 8000 <= n_reads < len(case['lines'])


@pytest.mark.parametrize('seed', range(3))
def test_a_lowered_depth_rule(exe, tmp_path, oracle_built, seed):
    rng = random.Random(seed)
    seq = pc.random_contig(rng, 1400)
    lines = []
    for i in range(60):
        s = rng.choice([480, 480, 500, 500, 500, 530, 600, 640])
        lines.append(lc.span_read(rng, seq, f'd{i}', s, f'{rng.choice([20, 60, 150, 300])}M', sub=0.01))
    lines.sort(key=lambda l: int(l.split('\t')[3]))
    case = dict(name=f'low{seed}', seq=seq, lines=lines)
    text = pc.text_of(lc.write_case(tmp_path, case)[0])
    reads = lc.reads_of(case)
    got = run(exe, tmp_path, [(text, seq.encode(), maxcnt, rows_of(text), [700, 520]) for maxcnt in (3, 4, 5, 6)])
    for maxcnt, per in zip((3, 4, 5, 6), got):
        for pos, (state, bad, depth, n_reads, keys) in zip([700, 520], per):
            want_depth, want = want_of(reads, seq, pos, maxcnt)
            assert (state, depth) == (0, want_depth) and list(keys.items()) == list(want.items())
            assert n_reads == len(ref.fragments(reads, pos, maxcnt)) < len(ref.fragments(reads, pos))


def test_random_read_sets_through_the_host_build(exe, tmp_path, oracle_built):
    """indels, clips, N and IUPAC bases, gaps, rows at which the parser raises; the depth rule lowered and not"""
    from test_local_realign_ref import random_set
    sites, cases, sets = [700, 640, 790], [], []
    for seed in range(100, 106):
        seq, reads = random_set(seed)
        lines = [pc.sam_line(f'q{i}', r[0], lc.CTG, r[1] + 1, 60, ''.join('%d%s' % (n, op) for op, n in r[2]), r[3]) for i, r in enumerate(reads)]
        text = pc.text_of(lc.write_case(tmp_path, dict(name=f'rand{seed}', seq=seq, lines=lines))[0])
        for maxcnt in (4, ref.MAXCNT):
            cases.append((text, seq.encode(), maxcnt, rows_of(text), sites))
            sets.append((seq, reads, maxcnt))
    raised = 0
    for (seq, reads, maxcnt), per in zip(sets, run(exe, tmp_path, cases)):
        for pos, (state, bad, depth, n_reads, keys) in zip(sites, per):
            try:
                want_depth, want = want_of(reads, seq, pos, maxcnt)
            except ref.SiteRaises:
                raised += 1
                assert state == 1
                continue
            assert (state, depth) == (0, want_depth) and list(keys.items()) == list(want.items())
    assert raised > 0


def test_malformed_records_end_in_a_reason(exe, tmp_path, oracle_built):
    header = b'BAM\1' + struct.pack('<i', 0) + struct.pack('<i', 1) + struct.pack('<i', 2) + b'c\0' + struct.pack('<i', 2000)
    acgt = pack([1, 2, 4, 8] * 20)                 # 80 bases
    contig = (b'ACGT' * 500)
    pos = 700                                      # region 0-based [466, 934)
    recs = [
        ('good', raw_record(0, 650, 60, 0, 'good', [80 << 4 | M], 80, acgt), 0),
        ('N inside the region', raw_record(0, 650, 60, 0, 'n', [40 << 4 | M, 5 << 4 | N, 40 << 4 | M], 80, acgt), SKIP_PAD),
        ('P inside the region', raw_record(0, 650, 60, 0, 'p', [40 << 4 | M, 1 << 4 | P, 40 << 4 | M], 80, acgt), SKIP_PAD),
        ('N before the region is nothing', raw_record(0, 300, 60, 0, 'nb', [10 << 4 | M, 100 << 4 | N, 70 << 4 | M], 80, acgt), 0),
        ('code 0 under a column', raw_record(0, 650, 60, 0, 'eq', [80 << 4 | M], 80, pack([1, 2, 0, 8] * 20)), EQ_BASE),
        ('code 0 outside the window is nothing', raw_record(0, 440, 60, 0, 'eqo', [80 << 4 | M], 80, pack([0, 0, 0, 0] * 10 + [1, 2, 4, 8] * 10)), 0),
        ('no bases', raw_record(0, 650, 60, 0, 'nb', [80 << 4 | M], 0, b''), NO_BASES),
        ('M past l_seq', raw_record(0, 650, 60, 0, 'short', [5 << 4 | S, 90 << 4 | M], 80, acgt), PAST_BASES),
        ('an insertion past l_seq', raw_record(0, 650, 60, 0, 'ins', [80 << 4 | M, 0xfffffff << 4 | I, 1 << 4 | M], 80, acgt), PAST_BASES),
        ('CIGAR past the record', raw_record(0, 650, 60, 0, 'past', [80 << 4 | M], 80, acgt, n_cigar=4000), PAST),
        ('bases past the record', raw_record(0, 650, 60, 0, 'pastq', [80 << 4 | M], 4000, acgt, block_size=32 + 6 + 4 + 10), PAST),
    ]
    recs += [(f'operation code {op}', raw_record(0, 650, 60, 0, f'op{op}', [40 << 4 | M, 3 << 4 | op, 37 << 4 | M], 80, acgt), BAD_OP) for op in range(9, 16)]
    cases = []
    for what, rec, why in recs:
        text = header + rec
        cases.append((text, contig, ref.MAXCNT, [(len(header), 650 if why or what == 'good' else struct.unpack_from('<i', rec, 8)[0], 1000)], [pos]))
    # the last record of the text: off lies inside, its fixed bytes do not
    cases.append((header + b'\x10\0\0\0' + b'\0' * 8, contig, ref.MAXCNT, [(len(header), 650, 1000)], [pos]))
    got = run(exe, tmp_path, cases)
    for (what, rec, why), per in zip(recs, got):
        state, bad, depth, n_reads, keys = per[0]
        assert (state, bad) == ((100 + why, 0) if why else (0, -1)), what
    assert got[-1][0][:2] == (100 + PAST, 0)
    assert got[0][0][3] == 1
