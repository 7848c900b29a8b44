"""CPU test: the pile-up arithmetic the kernels run (csrc/pileup_core.h), built for the host with g++ (scripts/pileup_host_check.cpp,
under AddressSanitizer and UBSan where the toolchain has their runtimes), takes the golden cases and malformed records to the
statuses, counters and candidate rows of the restatement (tests/pileup_ref.py) -- before any of them meets a GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pileup_cases as pc
import pileup_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = struct.Struct('<qqqiiHBBii')        # mpn_pileup_rec + the rc of the counting
CAND = struct.Struct('<ii7i7sB')


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp('pileup_host') / 'pileup_host_check'
    src = os.path.join(ROOT, 'scripts', 'pileup_host_check.cpp')
    base = ['g++', '-std=c++17', '-Wall', '-Werror', '-o', str(out), src]
    if subprocess.run(base + ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']).returncode != 0:
        subprocess.run(base + ['-O2'], check=True)
    return out


def run(exe, tmp_path, cases):
    """cases: [(text, lo, hi, min_coverage, threshold, window reference bytes, [(off, take, lead)])]
    -> [([(status, soft, total, span, ref_id, pos, n_cigar, mapq, rc)], counters (hi - lo, 7), [(pos, ref base, depth, [(label, count)])])]"""
    src, dst = tmp_path / 'cases.bin', tmp_path / 'results.bin'
    with open(src, 'wb') as f:
        f.write(struct.pack('<I', len(cases)))
        for text, lo, hi, cov, thr, refb, rows in cases:
            assert len(refb) == hi - lo
            f.write(struct.pack('<QqqddI', len(text), lo, hi, cov, thr, len(rows)) + text + refb)
            f.write(b''.join(struct.pack('<qii', *r) for r in rows))
    subprocess.run([str(exe), str(src), str(dst)], check=True, timeout=300)
    blob, p, out = dst.read_bytes(), 0, []
    for text, lo, hi, cov, thr, refb, rows in cases:
        recs = []
        for _ in rows:
            soft, total, span, ref_id, pos, n_cigar, mapq, status, _, rc = REC.unpack_from(blob, p)
            recs.append((status, soft, total, span, ref_id, pos, n_cigar, mapq, rc))
            p += REC.size
        counts = np.frombuffer(blob, dtype='<i4', count=(hi - lo) * 7, offset=p).reshape(hi - lo, 7)
        p += counts.nbytes
        n_cand, = struct.unpack_from('<Q', blob, p)
        p += 8
        cands = []
        for _ in range(n_cand):
            v = CAND.unpack_from(blob, p)
            cands.append((v[0], chr(v[10]), v[1], list(zip(v[9].decode(), v[2:9]))))
            p += CAND.size
        out.append((recs, counts, cands))
    assert p == len(blob)
    return out


def test_golden_cases_through_the_host_build(exe, tmp_path):
    cases, want = [], []
    for case in pc.golden_cases():
        o = case['options']
        ctg, min_mq = o['ctgName'], o.get('minMQ', 0)
        text = pc.text_of(pc.write_case(tmp_path, case)[0])
        seq = dict((n, s) for n, s in case['contigs'])[ctg]
        hi = len(seq) + 20                                 # past the end of the sequence: reads overhang it
        took = {rec['off']: lead for rec, lead in ref.taken(text, ctg, min_mq)}
        recs = ref.records(text)
        rows = [(r['off'], int(r['off'] in took), int(took.get(r['off'], False))) for r in recs]
        cases.append((text, 0, hi, float(o['minCoverage']), float(o['threshold']), seq.encode() + bytes(20), rows))
        pile = ref.counts(text, ctg, min_mq)
        want.append((recs, ref.counts_array(text, ctg, 0, hi, min_mq), ref.candidates(pile, seq, None, None, o['threshold'], o['minCoverage'])))
    for case, (g_recs, g_counts, g_cands), (recs, counts, cands) in zip(pc.golden_cases(), run(exe, tmp_path, cases), want):
        for g, r in zip(g_recs, recs):
            assert g[:4] == ref.summary(r) and g[4:8] == (r['ref_id'], r['pos'], len(r['ops']), r['mapq']), (case['name'], r['name'])
            assert g[8] in (-1, 0)
        assert np.array_equal(g_counts, counts), case['name']
        assert g_cands == [(p, rb, d, [(l, c) for l, c in order]) for p, rb, d, order in cands], case['name']


def raw_record(ref_id, pos, mapq, flag, name, cigar, l_seq, packed, n_cigar=None, block_size=None):
    """-> a BAM record with its block_size word; n_cigar and block_size may lie"""
    nm = name.encode() + b'\0'
    body = (struct.pack('<iiBBHHHiiii', ref_id, pos, len(nm), mapq, 0, len(cigar) if n_cigar is None else n_cigar, flag, l_seq, -1, -1, 0) + nm +
            struct.pack('<%dI' % len(cigar), *cigar) + packed + b'\xff' * l_seq)
    return struct.pack('<i', len(body) if block_size is None else block_size) + body


def pack(codes):
    codes = list(codes) + [0] * (len(codes) & 1)
    return bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(codes), 2))


def test_malformed_records_end_in_a_status(exe, tmp_path):
    header = b'BAM\1' + struct.pack('<i', 0) + struct.pack('<i', 1) + struct.pack('<i', 2) + b'c\0' + struct.pack('<i', 100)
    assert ref.refs(header) == [('c', 100)]
    acgt = pack([1, 2, 4, 8] * 5)                  # 20 bases
    recs = [
        ('good', raw_record(0, 10, 60, 0, 'good', [20 << 4 | ref.M], 20, acgt), ref.OK, 0),
        ('negative pos', raw_record(0, -5, 60, 0, 'neg', [20 << 4 | ref.M], 20, acgt), ref.OK, 0),
        ('pos beyond the contig', raw_record(0, 95, 60, 0, 'far', [20 << 4 | ref.M], 20, acgt), ref.OK, 0),
        ('pos far beyond the window', raw_record(0, 0x7ffffff0, 60, 0, 'edge', [3 << 4 | ref.D, 20 << 4 | ref.M], 20, acgt), ref.OK, 0),
        ('code 0 under M', raw_record(0, 30, 60, 0, 'eq', [20 << 4 | ref.M], 20, pack([1, 2, 0, 8] * 5)), ref.OK, 1),
        ('no bases', raw_record(0, 30, 60, 0, 'nb', [20 << 4 | ref.M], 0, b''), ref.NO_BASE, 1),
        ('M past l_seq', raw_record(0, 40, 60, 0, 'short', [5 << 4 | ref.S, 16 << 4 | ref.M], 20, acgt), ref.NO_BASE, 1),
        ('a long I past l_seq is no error', raw_record(0, 40, 60, 0, 'ins', [10 << 4 | ref.M, 0xfffffff << 4 | ref.I], 20, acgt), ref.OK, 0),
        ('placeholder', raw_record(0, 10, 60, 0, 'cg', [20 << 4 | ref.S, 70000 << 4 | ref.N], 20, acgt), ref.PLACEHOLDER, None),
    ]
    recs += [(f'operation code {op}', raw_record(0, 50, 60, 0, f'op{op}', [5 << 4 | ref.M, 3 << 4 | op, 5 << 4 | ref.M], 20, acgt), ref.BAD_OP, 1)
             for op in range(9, 16)]
    recs += [
        ('CIGAR past the record', raw_record(0, 10, 60, 0, 'past', [20 << 4 | ref.M], 20, acgt, n_cigar=40), ref.CIGAR_PAST, 1),
        ('bases past the record', raw_record(0, 10, 60, 0, 'pastq', [20 << 4 | ref.M], 4000, acgt, block_size=32 + 6 + 4 + 10), ref.CIGAR_PAST, 1),
        # the last record of the text: its CIGAR would run far past the end of the text
        ('CIGAR past the text', raw_record(0, 10, 60, 0, 'end', [20 << 4 | ref.M], 20, acgt, n_cigar=65535, block_size=1 << 20), ref.CIGAR_PAST, 1),
    ]
    text, rows, offs = header, [], []
    for _, raw, status, _ in recs:
        offs.append(len(text))
        rows.append((len(text), int(status != ref.PLACEHOLDER), 1))
        text += raw
    rows.append((len(text) - 20, 1, 1))               # a row whose fixed bytes pass the end of the text
    rows.append((-4, 1, 1))
    lo, hi = 0, 100
    (g_recs, g_counts, _), = run(exe, tmp_path, [(text, lo, hi, 1.0, 0.1, b'A' * 100, rows)])
    assert [g[0] for g in g_recs[-2:]] == [255, 255]
    want = np.zeros((hi - lo, 7), dtype=np.int32)
    for (name, raw, status, rc), off, g in zip(recs, offs, g_recs):
        assert g[0] == status, name
        if rc is not None:
            assert g[8] == rc, name
        if status == ref.OK and rc == 0:
            n_cigar, l_seq = struct.unpack_from('<H', raw, 16)[0], struct.unpack_from('<i', raw, 20)[0]
            c0 = 36 + raw[12]
            ops = [(w & 15, w >> 4) for w in struct.unpack_from('<%dI' % n_cigar, raw, c0)]
            packed = raw[c0 + 4 * n_cigar:]
            rec = dict(name=name, pos=struct.unpack_from('<i', raw, 8)[0], ops=ops, codes=[(packed[i >> 1] >> (0 if i & 1 else 4)) & 15 for i in range(l_seq)])
            assert g[1:4] == ref.summary(rec)[1:], name
            for p, c in ref.add_record({}, rec, True).items():
                if lo <= p < hi:
                    want[p - lo] += np.array(c, dtype=np.int32)
    # 'code 0 under M' stops at its third base: what it added up to there stays (the counters of such a file are not used)
    want[30, 0] += 1
    want[31, 1] += 1
    # 'M past l_seq' stops behind the last base there is: query 5 .. 19 at 40 .. 54
    for j in range(15):
        want[40 + j, (5 + j) % 4] += 1
    # an operation code above 8 stops the serial count at that operation: the five bases before it stay, once per such record
    for k in range(7):
        for p, slot in zip(range(50, 55), (0, 1, 2, 3, 0)):
            want[p, slot] += 1
    assert np.array_equal(g_counts, want)
