"""CPU test: the arithmetic the read-realignment kernels run (csrc/read_realign_core.h), built for the host with g++
(scripts/read_realign_host_check.cpp, under AddressSanitizer and UBSan where the toolchain has their runtimes), takes the constructed
cases to the rows and memberships of the restatement (tests/read_realign_ref.py), and malformed records to a status -- before any of
them meets a GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import read_realign_cases as rc
import read_realign_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = struct.Struct('<qqqqiiiiiHHBBBBBB2xi')        # mpn_rr_rec + the rc of the counting on a row of the record's own
ROW = 5041
OK, PAST, BAD_OP, PLACEHOLDER, BAD_AUX, HP_TEXT, BASE_EQ, NO_BASE = range(8)


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp('read_realign_host') / 'read_realign_host_check'
    src = os.path.join(ROOT, 'scripts', 'read_realign_host_check.cpp')
    base = ['g++', '-std=c++17', '-Wall', '-Werror', '-o', str(out), src]
    if subprocess.run(base + ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']).returncode != 0:
        subprocess.run(base + ['-O2'], check=True)
    return out


def run(exe, tmp_path, cases):
    """cases: [(text, contig bytes, min_mq, [off], (pos, end, [[(start, end)]]))]
    -> [(recs: [dict], viewed: [(row, chunk_of, taken, counted)], epochs: [(chunk_start, bad, row)], assign: (splits, reads) array)]"""
    src, dst = tmp_path / 'cases.bin', tmp_path / 'results.bin'
    with open(src, 'wb') as f:
        f.write(struct.pack('<I', len(cases)))
        for text, contig, min_mq, offs, (pos, end, splits) in cases:
            f.write(struct.pack('<QQiI', len(text), len(contig), min_mq, len(offs)) + text + contig + struct.pack('<%dq' % len(offs), *offs))
            flat = [w for s in splits for w in s]
            begin = np.concatenate([[0], np.cumsum([len(s) for s in splits])]).astype('<i4')
            f.write(struct.pack('<II', len(pos), len(splits)) + np.asarray(pos, '<i4').tobytes() + np.asarray(end, '<i4').tobytes() + begin.tobytes() +
                    np.asarray([w[0] for w in flat], '<i4').tobytes() + np.asarray([w[1] for w in flat], '<i4').tobytes())
    subprocess.run([str(exe), str(src), str(dst)], check=True, timeout=300)
    blob, p, out = dst.read_bytes(), 0, []
    for text, contig, min_mq, offs, (pos, end, splits) in cases:
        recs = []
        for _ in offs:
            v = REC.unpack_from(blob, p)
            recs.append(dict(zip(('soft', 'total', 'del', 'span', 'ref_id', 'pos', 'l_seq', 'next_ref', 'next_pos', 'flag', 'n_cigar', 'mapq', 'has_seq',
                                  'has_qual', 'hp', 'status', 'clipped', 'rc'), v)))
            p += REC.size
        n, = struct.unpack_from('<I', blob, p)
        viewed = [struct.unpack_from('<4i', blob, p + 4 + 16 * i) for i in range(n)]
        p += 4 + 16 * n
        n, = struct.unpack_from('<I', blob, p)
        p += 4
        epochs = []
        for _ in range(n):
            cs, bad = struct.unpack_from('<ii', blob, p)
            epochs.append((cs, bad, np.frombuffer(blob, dtype='<i4', count=ROW, offset=p + 8)))
            p += 8 + 4 * ROW
        assign = np.frombuffer(blob, dtype='<i4', count=len(splits) * len(pos), offset=p).reshape(len(splits), len(pos))
        p += assign.nbytes
        out.append((recs, viewed, epochs, assign))
    assert p == len(blob)
    return out


def restated(case):
    """the restatement with the realigner switched off: rows, windows and memberships do not depend on it"""
    trace = []
    ref.realign(rc.sam_lines(case), case['contig'], rc.CTG, case['min_mq'], case['min_coverage'], consensus=lambda *a: [], trace=trace)
    return trace


@pytest.mark.parametrize('case', rc.edge_cases() + [rc.plain_variants()], ids=lambda c: c['name'])
def test_rows_and_memberships_equal_the_restatement(exe, tmp_path, case):
    text, offs = rc.text_of(case)
    trace = restated(case)
    lines = rc.sam_lines(case)
    fields = [l.split('\t') for l in lines]
    (recs, viewed, epochs, _), = run(exe, tmp_path, [(text, case['contig'].upper().encode(), case['min_mq'], offs, ([], [], []))])
    for r, f in zip(recs, fields):
        assert r['status'] == OK and (r['pos'], r['mapq'], r['flag']) == (int(f[3]) - 1, int(f[4]), int(f[1])), f[0]
        hp = ref.hp_digit('\t'.join(f).strip().split()[11:])
        assert (chr(r['hp']) if r['hp'] else None) == hp, f[0]
        assert r['pos'] + r['l_seq'] + r['del'] == r['pos'] + ref.read_span(f[9], f[5]), f[0]
        if f[5] != '*':
            assert ref.too_clipped(f[5]) == bool(r['clipped']), f[0]
    assert len(epochs) == len(trace)
    for (cs, bad, row), want in zip(epochs, trace):
        assert cs == want['chunk_start'] and bad == 0
        assert np.array_equal(row, np.asarray(want['row'], dtype=np.int32)), (case['name'], cs)
    # the assignment: the member reads of every yield that is not skipped against its windows
    row_of = [v[0] for v in viewed]
    todo = []
    for want in trace:
        if want['windows'] is None:
            continue
        assert all(viewed[k][2] for k in want['reads'])            # the restatement's members are taken records
        pos = [recs[row_of[k]]['pos'] for k in want['reads']]
        end = [recs[row_of[k]]['pos'] + recs[row_of[k]]['l_seq'] + recs[row_of[k]]['del'] for k in want['reads']]
        todo.append((want, (b'', b'', 0, [], (pos, end, want['windows']))))
    for (want, _), (_, _, _, assign) in zip(todo, run(exe, tmp_path, [t[1] for t in todo]) if todo else []):
        for s, (windows, members) in enumerate(zip(want['windows'], want['members'])):
            got = [[k for i, k in enumerate(want['reads']) if assign[s][i] == w] for w in range(len(windows))]
            assert got == (members or [[] for _ in windows]), (case['name'], want['chunk_start'], s)


def raw_record(ref_id, pos, mapq, flag, name, cigar, l_seq, packed, qual=None, aux=b'', n_cigar=None, block_size=None):
    """-> a BAM record with its block_size word; n_cigar and block_size may lie"""
    nm = name.encode() + b'\0'
    body = (struct.pack('<iiBBHHHiiii', ref_id, pos, len(nm), mapq, 0, len(cigar) if n_cigar is None else n_cigar, flag, l_seq, -1, -1, 0) + nm +
            struct.pack('<%dI' % len(cigar), *cigar) + packed + (bytes([30]) * l_seq if qual is None else qual) + aux)
    return struct.pack('<i', len(body) if block_size is None else block_size) + body


def pack(codes):
    codes = list(codes) + [0] * (len(codes) & 1)
    return bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(codes), 2))


M, I, D, N, S = 0, 1, 2, 3, 4


def test_malformed_records_end_in_a_status(exe, tmp_path):
    header = b'BAM\1' + struct.pack('<i', 0) + struct.pack('<i', 1) + struct.pack('<i', 2) + b'c\0' + struct.pack('<i', 100)
    acgt = pack([1, 2, 4, 8] * 5)                  # 20 bases
    m20 = [20 << 4 | M]
    recs = [
        ('good', raw_record(0, 10, 60, 0, 'good', m20, 20, acgt), OK),
        ('HP of type c', raw_record(0, 10, 60, 0, 'hp', m20, 20, acgt, aux=b'NMC\x01HPc\x02'), OK),
        ('pos beyond the contig', raw_record(0, 95, 60, 0, 'far', m20, 20, acgt), OK),
        ('pos far beyond', raw_record(0, 0x7ffffff0, 60, 0, 'edge', [3 << 4 | D, 20 << 4 | M], 20, acgt), OK),
        ('a deletion of 2^28 - 1', raw_record(0, 10, 60, 0, 'del', [5 << 4 | M, 0xfffffff << 4 | D, 15 << 4 | M], 20, acgt), OK),
        ('code 0 under M', raw_record(0, 30, 60, 0, 'eq', m20, 20, pack([1, 2, 0, 8] * 5)), BASE_EQ),
        ('no bases', raw_record(0, 30, 60, 0, 'nb', m20, 0, b''), NO_BASE),
        ('M past l_seq', raw_record(0, 40, 60, 0, 'short', [5 << 4 | S, 16 << 4 | M], 20, acgt), NO_BASE),
        ('a long I past l_seq', raw_record(0, 40, 60, 0, 'ins', [10 << 4 | M, 0xfffffff << 4 | I], 20, acgt), NO_BASE),
        ('a long S past l_seq', raw_record(0, 40, 60, 0, 'clip', [0xfffffff << 4 | S, 10 << 4 | M], 20, acgt), NO_BASE),
        ('placeholder', raw_record(0, 10, 60, 0, 'cg', [20 << 4 | S, 70000 << 4 | N], 20, acgt), PLACEHOLDER),
        ('CIGAR past the record', raw_record(0, 10, 60, 0, 'past', m20, 20, acgt, n_cigar=40), PAST),
        ('bases past the record', raw_record(0, 10, 60, 0, 'pastq', m20, 4000, acgt, block_size=32 + 6 + 4 + 10), PAST),
        ('qualities past the record', raw_record(0, 10, 60, 0, 'pq', m20, 20, acgt, qual=b'\x1e' * 5), PAST),
        ('aux past the record: a tag cut short', raw_record(0, 10, 60, 0, 'a1', m20, 20, acgt, aux=b'NM'), PAST),
        ('aux past the record: a value cut short', raw_record(0, 10, 60, 0, 'a2', m20, 20, acgt, aux=b'NMi\x01\x02'), PAST),
        ('aux past the record: a Z without its NUL', raw_record(0, 10, 60, 0, 'a3', m20, 20, acgt, aux=b'XZZabc'), PAST),
        ('a B array with a huge count', raw_record(0, 10, 60, 0, 'a4', m20, 20, acgt, aux=b'XBBi' + struct.pack('<I', 0xffffffff) + b'\0' * 8), PAST),
        ('a B array cut short', raw_record(0, 10, 60, 0, 'a5', m20, 20, acgt, aux=b'XBBs' + struct.pack('<I', 3) + b'\0' * 5), PAST),
        ('a B array of an unknown subtype', raw_record(0, 10, 60, 0, 'a6', m20, 20, acgt, aux=b'XBBZ' + struct.pack('<I', 1) + b'\0'), BAD_AUX),
        ('an aux field of an unknown type', raw_record(0, 10, 60, 0, 'a7', m20, 20, acgt, aux=b'XQq\x01'), BAD_AUX),
        ('a Z value with HP:i:', raw_record(0, 10, 60, 0, 'a8', m20, 20, acgt, aux=b'XZZHHP:i:3\0'), HP_TEXT),
    ]
    recs += [(f'operation code {op}', raw_record(0, 50, 60, 0, f'op{op}', [5 << 4 | M, 3 << 4 | op, 5 << 4 | M], 20, acgt), BAD_OP) for op in range(9, 16)]
    # the last record of the text: its CIGAR would run far past the end of the text
    recs.append(('CIGAR past the text', raw_record(0, 10, 60, 0, 'end', m20, 20, acgt, n_cigar=65535, block_size=1 << 20), PAST))
    text, offs = header, []
    for _, raw, _ in recs:
        offs.append(len(text))
        text += raw
    offs += [len(text) - 20, -4]                        # rows whose fixed bytes do not lie inside the text
    (got, viewed, epochs, _), = run(exe, tmp_path, [(text, b'ACGT' * 25, 0, offs, ([], [], []))])
    assert [g['status'] for g in got[-2:]] == [255, 255]
    for (name, _, status), g in zip(recs, got):
        assert g['status'] == status, name
    assert got[1]['hp'] == ord('2')
    assert {g['rc'] for g in got[:-2]} <= {0, 1} and got[0]['rc'] == 0
    assert got[2]['rc'] == 1                            # its bases run past the contig's end: no contig byte is read there
    n_ok = sum(status == OK for _, _, status in recs)
    assert all(0 <= bad <= n_ok for _, bad, _ in epochs)        # only records with status 0 were counted


def test_overlap_rule(exe, tmp_path):
    """ties go to the first window, no overlap and a start above the last window's end to none"""
    windows = [[(100, 200), (300, 400)], [], [(0, 50)]]
    reads = [(150, 350), (150, 250), (250, 350), (200, 300), (401, 500), (400, 500), (0, 1000), (120, 130), (50, 100)]
    (_, _, _, assign), = run(exe, tmp_path, [(b'', b'', 0, [], ([r[0] for r in reads], [r[1] for r in reads], windows))])
    want = [[ref.best_window(r[0], r[1], w) if w and r[0] <= max(x[1] for x in w) else None for r in reads] for w in windows]
    assert assign.tolist() == [[-1 if x is None else x for x in row] for row in want]
    assert assign[0].tolist() == [0, 0, 1, -1, -1, -1, 0, 0, -1]
