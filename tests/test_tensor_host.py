"""CPU test: the tensor arithmetic the kernels run (csrc/tensor_core.h), built for the host with g++ (scripts/tensor_host_check.cpp,
under AddressSanitizer and UBSan where the toolchain has their runtimes), takes the golden cases and malformed records to the record
facts, joins, centre flags and tensors of the restatement (tests/tensor_ref.py) -- before any of them meets a GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pileup_cases as pc
import tensor_cases as tc
import tensor_ref as ref
from test_pileup_host import pack, raw_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW = struct.Struct('<qiBBHqii')        # mpn_tensor_rec, span, pos, reverse
OK, CIGAR_PAST, BAD_OP, PLACEHOLDER, NO_BASE = range(5)


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp('tensor_host') / 'tensor_host_check'
    src = os.path.join(ROOT, 'scripts', 'tensor_host_check.cpp')
    base = ['g++', '-std=c++17', '-Wall', '-Werror', '-o', str(out), src]
    if subprocess.run(base + ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']).returncode != 0:
        subprocess.run(base + ['-O2'], check=True)
    return out


def run(exe, tmp_path, cases):
    """cases: [(text, reference bytes, ref_start, left_edge, [off], [(c0, begin, end)])]
    -> [([(hts_len, l_seq, has_qual, status, span, pos, reverse)], [([(joins, flag, rc)], tensor (33, 8, 4))])]"""
    src, dst = tmp_path / 'cases.bin', tmp_path / 'results.bin'
    with open(src, 'wb') as f:
        f.write(struct.pack('<I', len(cases)))
        for text, refb, ref_start, left, offs, centres in cases:
            f.write(struct.pack('<QqQiII', len(text), ref_start, len(refb), int(left), len(offs), len(centres)) + text + refb)
            f.write(b''.join(struct.pack('<q', o) for o in offs))
            f.write(b''.join(struct.pack('<iII', *c) for c in centres))
    subprocess.run([str(exe), str(src), str(dst)], check=True, timeout=300)
    blob, p, out = dst.read_bytes(), 0, []
    for text, refb, ref_start, left, offs, centres in cases:
        rows = []
        for _ in offs:
            hts, l_seq, has_qual, status, _, span, pos, rev = ROW.unpack_from(blob, p)
            rows.append((hts, l_seq, has_qual, status, span, pos, rev))
            p += ROW.size
        per = []
        for c0, begin, end in centres:
            trip = [struct.unpack_from('<Bbh', blob, p + 4 * i) for i in range(end - begin)]
            p += 4 * (end - begin)
            per.append((trip, np.frombuffer(blob, dtype='<i4', count=1056, offset=p).reshape(33, 8, 4)))
            p += 4 * 1056
        out.append((rows, per))
    assert p == len(blob)
    return out


def test_golden_cases_through_the_host_build(exe, tmp_path):
    cases, want = [], []
    for case in tc.golden_cases():
        o = case['options']
        left = not o.get('stop_consider_left_edge', False)
        ctg, seq = case['contigs'][0]
        text = pc.text_of(tc.write_case(tmp_path, case)[0])
        kw = tc.keywords(case)
        recs = ref.taken(text, ctg, kw['ctg_start'], kw['ctg_end'], kw['min_mq'], kw['dcov'])
        window, ref_start = ref.reference_window(seq, kw['ctg_start'], kw['ctg_end'])
        centres = [p - 1 for p in case['positions']]
        cases.append((text, window.encode(), ref_start, left, [r['off'] for r in recs], [(c0, 0, len(recs)) for c0 in centres]))
        want.append((recs, centres, left, window, ref_start))
    for case, (rows, per), (recs, centres, left, window, ref_start) in zip(tc.golden_cases(), run(exe, tmp_path, cases), want):
        for g, r in zip(rows, recs):
            assert g == (r['hts_len'], r['l_seq'], int(r['has_qual']), OK, r['span'], r['pos'], int(r['reverse'])), (case['name'], r['name'])
        for c0, (trip, tensor) in zip(centres, per):
            joined = [r for r in recs if ref.joins(r, c0, left)]
            assert [t[0] for t in trip] == [int(ref.joins(r, c0, left)) for r in recs], (case['name'], c0)
            assert [t[1] for t in trip] == [int(ref.joins(r, c0, left) and ref.high_quality(r, c0, left)) for r in recs], (case['name'], c0)
            assert all(t[2] == (0 if t[0] else -1) for t in trip), (case['name'], c0)
            assert np.array_equal(tensor, ref.fill(joined, c0, left, window, ref_start)), (case['name'], c0)


def test_malformed_records_end_in_a_status(exe, tmp_path):
    header = b'BAM\1' + struct.pack('<i', 0) + struct.pack('<i', 1) + struct.pack('<i', 2) + b'c\0' + struct.pack('<i', 200)
    acgt = pack([1, 2, 4, 8] * 5)                  # 20 bases; raw_record gives them the quality 0xff
    M, I, D = ref.M, ref.I, ref.D
    # (what, the record, status of mpn_tensor_rec, joins centre 100 (c0 = 99), rc of its fill)
    recs = [
        ('good', raw_record(0, 90, 60, 0, 'good', [20 << 4 | M], 20, acgt), OK, 1, 0),
        ('good and far away', raw_record(0, 10, 60, 0, 'far', [20 << 4 | M], 20, acgt), OK, 0, -1),
        ('M past l_seq', raw_record(0, 90, 60, 0, 'short', [5 << 4 | ref.S, 16 << 4 | M], 20, acgt), NO_BASE, 1, 1),
        ('M past l_seq behind the window', raw_record(0, 70, 60, 0, 'short2', [20 << 4 | M, 30 << 4 | M], 20, acgt), NO_BASE, 1, 1),
        ('no bases', raw_record(0, 95, 60, 0, 'nb', [20 << 4 | M], 0, b''), NO_BASE, 1, 1),
        ('an I past l_seq in the window', raw_record(0, 90, 60, 0, 'ins', [10 << 4 | M, 0xffffff << 4 | I, 5 << 4 | M], 20, acgt), NO_BASE, 1, 1),
        ('a D needs no base', raw_record(0, 90, 60, 0, 'del', [2 << 4 | M, 40 << 4 | D], 2, pack([1, 2])), OK, 1, 0),
        ('CIGAR past the record', raw_record(0, 90, 60, 0, 'past', [20 << 4 | M], 20, acgt, n_cigar=40), CIGAR_PAST, 0, -1),
        ('bases past the record', raw_record(0, 90, 60, 0, 'pastq', [20 << 4 | M], 4000, acgt, block_size=32 + 6 + 4 + 10), CIGAR_PAST, 0, -1),
    ]
    recs += [(f'operation code {op}', raw_record(0, 90, 60, 0, f'op{op}', [5 << 4 | M, 3 << 4 | op, 5 << 4 | M], 20, acgt), BAD_OP, 0, -1)
             for op in range(9, 16)]
    # the last records of the text: qualities that would pass its end (the pile-up's layout still holds: the read joins), and a CIGAR
    # that would run far past it
    short = raw_record(0, 90, 60, 0, 'endq', [20 << 4 | M], 20, acgt)[:-8]
    recs.append(('qualities past the text', short, CIGAR_PAST, 1, 1))
    text, offs = header, []
    for _, raw, _, _, _ in recs:
        offs.append(len(text))
        text += raw
    offs += [len(text) - 20, -4]                  # rows whose fixed bytes pass the end of the text
    (rows, ((trip, tensor),)), = run(exe, tmp_path, [(text, b'ACGT' * 50, 0, True, offs, [(99, 0, len(offs))])])
    assert [g[3] for g in rows[-2:]] == [255, 255] and [t[0] for t in trip[-2:]] == [0, 0]
    for (name, raw, status, joins, rc), g, t in zip(recs, rows, trip):
        assert g[3] == status, name
        assert (t[0], t[2]) == (joins, rc), name
        if name in ('qualities past the text', 'no bases'):
            assert t[1] == -1, name
    # every good base of these records has the quality 0xff: a high-quality one
    assert trip[0][1] == 1 and trip[6][1] == 1
    assert int(tensor[:, :, 0].sum()) > 0
