"""A plain restatement of mpn_fastq_scan (include/mpn_ingest.h) and the texts its tests share.

scan(text, final) -> (rows, consumed, status): the longest prefix of plain four-line records of `text`, line kinds by line index
modulo 4 counted from the start of the text.  records(text, rows) reads the rows back as iter_fastx would yield them.
"""
import io
import os
import re

import numpy as np

from megapath_nano_amd import fastx

OK, UNSUPPORTED = 0, 14
ROW = np.dtype([('seq_off', '<i8'), ('qual_off', '<i8'), ('name_off', '<i8'), ('len', '<i4'), ('name_len', '<i4')])
BLANK = b' \t\v\f'
HERE = os.path.dirname(os.path.abspath(__file__))
HTSLIB_FASTQ = os.path.join(HERE, 'golden', 'htslib', 'fastq')


def header_tile():
    """MPN_FASTQ_TILE as the header states it (the GPU tests ask the library)"""
    with open(os.path.join(HERE, '..', 'include', 'mpn_ingest.h')) as f:
        return int(re.search(r'#define\s+MPN_FASTQ_TILE\s+(\d+)', f.read()).group(1))


def scan(text, final):
    text = bytes(text)
    L = len(text)
    starts = [0] + [m.end() for m in re.finditer(b'\n', text)]
    n_lf = len(starts) - 1
    starts.append(L + 1)            # the line feed imagined behind the text
    whole = n_lf + (1 if final and starts[n_lf] < L else 0)

    def line(i):
        """-> (start, end without LF and without the CR before it, flagged)"""
        s, e = starts[i], starts[i + 1] - 1
        kind, bad = i & 3, False
        if kind != 2:
            for m in re.finditer(b'\r', text[s:e]):
                p = s + m.start()
                bad |= p + 1 < L and text[p + 1] != 10
            if kind == 1:
                bad |= any(c in BLANK for c in text[s:e])
        if e > s and text[e - 1] == 13:
            e -= 1
        return s, e, bad

    rows, r = [], 0
    while 4 * r + 3 < whole:
        (s0, e0, b0), (s1, e1, b1), (s2, e2, _), (s3, e3, b3) = (line(4 * r + i) for i in range(4))
        n = e1 - s1
        plain = not (b0 or b1 or b3) and e0 > s0 and text[s0:s0 + 1] == b'@' and e2 > s2 and text[s2:s2 + 1] == b'+' and e3 - s3 == n and n <= 0x7fffffff
        if plain and n:
            plain = text[s1:s1 + 1] not in (b'@', b'>', b'+')
        if not plain:
            break
        a = s0 + 1
        while a < e0 and text[a] in BLANK + b'\r':
            a += 1
        z = a
        while z < e0 and text[z] not in BLANK + b'\r':
            z += 1
        rows.append((s1, s3, a, n, z - a))
        r += 1
    consumed = min(starts[4 * r], L)
    status = OK
    if consumed < L and (4 * r + 3 < whole or final):
        status = UNSUPPORTED
    return np.array(rows, dtype=ROW), consumed, status


def records(text, rows):
    out = []
    for w in rows:
        so, qo, no, n, nn = (int(w[k]) for k in ('seq_off', 'qual_off', 'name_off', 'len', 'name_len'))
        out.append((bytes(text[no:no + nn]).decode(), bytes(text[so:so + n]), bytes(text[qo:qo + n])))
    return out


def host_records(data):
    """what iter_fastx yields for these bytes; where it raises, the records before that and the marker 'ValueError'"""
    out = []
    try:
        for rec in fastx.iter_fastx(io.BytesIO(bytes(data))):
            out.append(rec)
    except ValueError:
        out.append('ValueError')
    return out


# ---- texts ---------------------------------------------------------------------------------------------------------------------
def rec(name, seq, qual=None, plus=b'+', eol=b'\n', last_eol=None):
    qual = b'I' * len(seq) if qual is None else qual
    return b'@' + name + eol + seq + eol + plus + eol + qual + (eol if last_eol is None else last_eol)


def _bases(n, seed=0):
    rng = np.random.default_rng(1000 + n + seed)
    return np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def _quals(n, seed=0):
    rng = np.random.default_rng(2000 + n + seed)
    return rng.integers(33, 127, n).astype(np.uint8).tobytes()


GOOD = [rec(b'g%d' % i, _bases(5 + 3 * i), _quals(5 + 3 * i)) for i in range(3)]


def plain_cases(tile):
    """[(id, text, final)]: every record of the text is plain (the last one may be cut where final is False)"""
    out = [
        ('qual_starts', rec(b'a', b'ACGT', b'@III') + rec(b'b', b'ACGT', b'+III') + rec(b'c', b'ACGT', b'>III') + rec(b'd', b'A', b'@') +
         rec(b'e', b'ACGT', b'@@@@') + rec(b'f', b'AC', b'+@') + GOOD[0], True),
        ('plus_name', rec(b'a', b'ACGT', plus=b'+a') + rec(b'b comment', b'AC', plus=b'+b comment \t x') + GOOD[1], True),
        ('crlf', b''.join(rec(b'r%d' % i, _bases(7 + i), _quals(7 + i), eol=b'\r\n') for i in range(5)), True),
        ('no_last_lf_final', GOOD[0] + rec(b'z', b'ACGTA', b'IIII@', last_eol=b''), True),
        ('no_last_lf_open', GOOD[0] + rec(b'z', b'ACGTA', b'IIII@', last_eol=b''), False),
        ('no_last_lf_cr_final', GOOD[0] + rec(b'z', b'ACGTA', b'IIII@', eol=b'\r\n', last_eol=b'\r'), True),
        ('one_base', b''.join(rec(b'o%d' % i, b'ACGT'[i % 4:i % 4 + 1], _quals(1, i)) for i in range(9)), True),
        ('empty_read', GOOD[0] + rec(b'e', b'') + GOOD[1], True),
        ('long_reads', b''.join(rec(b'L%d' % n, _bases(n), _quals(n)) for n in (tile - 1, tile, tile + 1, 70001)) + GOOD[2], True),
        ('long_header', GOOD[0] + rec(b'h' * (tile + 37) + b' c' * tile, b'ACGTT') + rec(b'x ' + b'y' * (2 * tile + 5), b'AC') + GOOD[1], True),
        ('names', rec(b'', b'AC') + rec(b' only a comment', b'ACG') + rec(b'n\tc', b'A') + rec(b'm', b'AG', eol=b'\r\n') + rec(b'\t \x0b k\x0cq', b'T') +
         rec(b'k\x1cz', b'TT'), True),
        ('short_3000', b''.join(rec(b's%d' % i, _bases(1 + i % 7, i), _quals(1 + i % 7, i)) for i in range(3000)), True),
        ('empty_text', b'', True),
        ('empty_text_open', b'', False),
    ]
    # a record start -- and the start of each of its other lines -- on the bytes edge - 2 .. edge + 2 of the first and second tile edge
    for m in (1, 2):
        for d in range(-2, 3):
            for k in range(4):
                second = rec(b'b', b'ACGTAC', b'@+>III')
                rel = (0, 3, 10, 12)[k]
                want = m * tile + d - rel            # the length of the record in front
                h = 1 if want % 2 == 1 else 2
                n = (want - 6 - h) // 2
                first = rec(b'a' * h, _bases(n), _quals(n))
                assert len(first) == want
                out.append((f'edge{m}_{d:+d}_line{k}', first + second + GOOD[0], True))
    return out


def cut_cases():
    """[(id, text, cut)]: three plain records; the text up to `cut` is scanned without final"""
    text = GOOD[0] + rec(b'mid dle', b'ACGTACGTAC', b'@@+>IIIIII', plus=b'+mid') + GOOD[2]
    a = len(GOOD[0])                         # the middle record: header a .. a + 9, bases .. a + 20, '+mid' .. a + 25, qualities .. a + 36
    where = {'nothing': 0, 'first_byte': a + 1, 'header': a + 4, 'header_end': a + 9, 'bases': a + 13, 'bases_end': a + 20, 'plus': a + 22,
             'plus_end': a + 25, 'quals': a + 30, 'quals_no_lf': a + 35, 'record_end': a + 36}
    assert text[a + 35:a + 37] == b'\n@' and text[a + 8:a + 10] == b'\nA' and text[a + 20:a + 21] == b'+'
    return [(k, text, c) for k, c in where.items()]


REASONS = [
    ('multiline_seq', b'@m\nACGT\nACGT\n+\nIIIIIIII\n'),
    ('blank_line', b'\n' + rec(b'm', b'ACGT')),
    ('missing_plus', b'@m\nACGT\nIIII\n'),
    ('qual_short', rec(b'm', b'ACGT', b'III')),
    ('qual_long', rec(b'm', b'ACGT', b'IIIII')),
    ('blank_in_seq', rec(b'm', b'AC GT', b'IIIII')),
    ('tab_in_seq', rec(b'm', b'AC\tGT', b'IIIII')),
    ('lone_cr_seq', rec(b'm', b'AC\rGT', b'IIIII')),
    ('lone_cr_qual', rec(b'm', b'ACGTA', b'II\rII')),
    ('fasta_record', b'>f\nACGT\n'),
    ('seq_starts_plus', rec(b'm', b'+CGT')),
    ('seq_starts_at', rec(b'm', b'@CGT')),
    ('no_at', b'm\nACGT\n+\nIIII\n'),
]
TRUNCATED = [('truncated_1', b'@t\n'), ('truncated_2', b'@t\nACGT\n'), ('truncated_3', b'@t\nACGT\n+\n'), ('truncated_3_nolf', b'@t\nACGT\n+')]


def unsupported_cases():
    """[(id, text, final, plain records before the offending one)]"""
    out = []
    for name, bad in REASONS:
        out.append((name + '_first', bad + GOOD[0] + GOOD[1], True, 0))
        out.append((name + '_middle', GOOD[0] + GOOD[1] + bad + GOOD[2], True, 2))
        out.append((name + '_middle_open', GOOD[0] + GOOD[1] + bad + GOOD[2], False, 2))
        out.append((name + '_last', GOOD[0] + GOOD[1] + GOOD[2] + bad, True, 3))
    for name, bad in TRUNCATED:
        out.append((name + '_first', bad, True, 0))
        out.append((name + '_second', GOOD[0] + bad, True, 1))
        out.append((name + '_last', GOOD[0] + GOOD[1] + GOOD[2] + bad, True, 3))
    return out


def htslib_cases():
    """[(file name, text, records the device takes before it hands over to the host: None = all)]"""
    out = []
    for name, n in (('single.fq', None), ('minimal.fq', None), ('interleaved.fq', None), ('multiline.fq', 0)):
        with open(os.path.join(HTSLIB_FASTQ, name), 'rb') as f:
            out.append((name, f.read(), n))
    return out
