"""The restatement of the pile-up and of Clair's candidate extraction (test infrastructure): what
preprocess/ExtractVariantCandidates.py (make_candidates, without --gen4Training) writes for a sorted BAM, as WHOLE-FILE semantics in
plain Python -- no streaming, no flushes.  It works from BAM bytes through tests/bam_in_ref.py; tests/test_pileup_ref.py pins it to
the reference's own output (tests/golden/candidates), and the GPU tests compare the kernels with it.

    refs(text)                         -> [(name, length)] of the header
    records(text)                      -> a dict per record, in file order: fixed fields, CIGAR operations, base codes
    summary(rec)                       -> (status, soft, total, span) as include/mpn_pileup.h mpn_pileup_rec
    taken(text, ctg_name, min_mq)      -> [(record, lead)]: the records that count and whether their leading I / D does
    counts(text, ctg_name, min_mq)     -> {position: [A, C, G, T, I, D, N]}
    counts_array(.., lo, hi)           -> the same as an (hi - lo, 7) int32 array
    candidates(..) / lines(..)         -> the rows that pass / the text the reference prints
"""
import struct

import numpy as np

import bam_in_ref

LABELS = 'ACGTIDN'
OK, CIGAR_PAST, BAD_OP, PLACEHOLDER, NO_BASE = 0, 1, 2, 3, 4
FILTER_FLAG = 2316
# read bases by 4-bit code (=ACMGRSVTWYHKDBN): IUPAC_base_to_ACGT_base_dict, N stays N, '=' has no entry
SLOT_OF_CODE = [None, 0, 1, 0, 2, 0, 1, 0, 3, 0, 1, 0, 2, 0, 1, 6]
REF_BASE = dict(zip('ACGTURYSWKMBDHVN', 'ACGTTACCAGACAAAA'))
REF_BASE['N'] = 'N'
M, I, D, N, S, H, P, EQ, X = range(9)


def refs(text):
    l_text, = struct.unpack_from('<i', text, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from('<i', text, p)
    p += 4
    out = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from('<i', text, p)
        out.append((text[p + 4:p + 4 + l_name - 1].decode(), struct.unpack_from('<i', text, p + 4 + l_name)[0]))
        p += 8 + l_name
    return out


def records(text):
    out = []
    for row in bam_in_ref.walk(text):
        o = row['off']
        ref_id, pos, _, mapq, _, n_cigar, flag, l_seq = struct.unpack_from('<iiBBHHHi', text, o + 4)
        c0 = o + 36 + row['l_read_name']
        ops = [(w & 15, w >> 4) for w in struct.unpack_from('<%dI' % n_cigar, text, c0)]
        packed = text[row['seq']:row['qual']]
        codes = [(packed[i >> 1] >> (0 if i & 1 else 4)) & 15 for i in range(l_seq)]
        out.append(dict(off=o, name=text[o + 36:c0 - 1].decode(), ref_id=ref_id, pos=pos, mapq=mapq, flag=flag, ops=ops, codes=codes))
    return out


def summary(rec):
    """-> (status, soft, total, span).  After a status the sums are not compared."""
    ops, l_seq = rec['ops'], len(rec['codes'])
    if any(op > 8 for op, _ in ops[:1]):
        return BAD_OP, 0, 0, 0
    if len(ops) == 2 and ops[0] == (S, l_seq) and ops[1][0] == N:
        return PLACEHOLDER, 0, 0, 0
    if any(op > 8 for op, _ in ops):
        return BAD_OP, 0, 0, 0
    soft = sum(n for op, n in ops if op == S)
    total = sum(n for _, n in ops)
    span = sum(n for op, n in ops if op in (M, EQ, X, D))
    q, status = 0, OK
    for op, n in ops:
        if op in (M, EQ, X, I, S):
            q += n
            if op in (M, EQ, X) and n > 0 and q > l_seq:
                status = NO_BASE
    return status, soft, total, span


def taken(text, ctg_name, min_mq=0):
    names = [n for n, _ in refs(text)]
    out, last = [], None
    for rec in records(text):
        if rec['flag'] & FILTER_FLAG or rec['ref_id'] < 0 or rec['ref_id'] >= len(names) or names[rec['ref_id']] != ctg_name:
            continue
        if rec['mapq'] < min_mq or not rec['ops']:
            continue
        status, soft, total, _ = summary(rec)
        if status == PLACEHOLDER:
            raise ValueError(f'{rec["name"]}: the CIGAR is in a CG tag')
        if 1.0 - float(soft) / (total + 1) < 0.55:
            continue
        if last is not None and rec['pos'] < last:
            raise ValueError(f'{rec["name"]}: the taken records are not sorted by position')
        out.append((rec, last is None or rec['pos'] > last))
        last = rec['pos']
    return out


def add_record(pile, rec, lead):
    rp, qp = rec['pos'], 0
    for op, n in rec['ops']:
        if op in (M, EQ, X):
            for _ in range(n):
                if qp >= len(rec['codes']) or SLOT_OF_CODE[rec['codes'][qp]] is None:
                    raise ValueError(f'{rec["name"]}: no base, or code 0, under a matched stretch')
                pile.setdefault(rp, [0] * 7)[SLOT_OF_CODE[rec['codes'][qp]]] += 1
                rp += 1
                qp += 1
        elif op in (I, D):
            if rp != rec['pos'] or lead:
                pile.setdefault(rp - 1, [0] * 7)[4 if op == I else 5] += 1
            if op == I:
                qp += n
            else:
                rp += n
        elif op == S:
            qp += n
        elif op > 8:
            raise ValueError(f'{rec["name"]}: operation code {op}')
    return pile


def counts(text, ctg_name, min_mq=0):
    pile = {}
    for rec, lead in taken(text, ctg_name, min_mq):
        add_record(pile, rec, lead)
    return pile


def counts_array(text, ctg_name, lo, hi, min_mq=0):
    out = np.zeros((max(hi - lo, 0), 7), dtype=np.int32)
    for p, c in counts(text, ctg_name, min_mq).items():
        if lo <= p < hi:
            out[p - lo] = c
    return out


def bed_intervals(bed_text, ctg_name):
    """-> [(start, end)] of ctg_name, a zero-length interval widened to one base; None if the contig does not occur"""
    out = None
    for line in bed_text.splitlines():
        col = line.split()
        if not col or col[0] != ctg_name:
            continue
        s, e = int(col[1]), int(col[2])
        out = (out or []) + [(s, e + 1 if s == e else e)]
    return out


def candidates(pile, ref_seq, ctg_start=None, ctg_end=None, threshold=0.125, min_coverage=4, bed=None):
    """pile: {position: counts}; ref_seq: the contig as str -> [(position, reference base, depth, [(label, count)] * 7)]"""
    out = []
    for p in sorted(pile):
        if ctg_start is not None and ctg_end is not None and not ctg_start <= p + 1 <= ctg_end:
            continue
        if bed is not None and not any(s <= p < e for s, e in bed):
            continue
        if p < 0 or p >= len(ref_seq) or ref_seq[p] not in REF_BASE:
            continue
        c = pile[p]
        depth = c[0] + c[1] + c[2] + c[3] + c[6]
        if depth < min_coverage:
            continue
        order = sorted(zip(LABELS, c), key=lambda x: -x[1])
        if order[0][0] != REF_BASE[ref_seq[p]] or float(order[1][1]) / (depth if depth > 0 else 1) >= threshold:
            out.append((p, REF_BASE[ref_seq[p]], depth, order))
    return out


def lines(ctg_name, rows):
    return ''.join(' '.join([ctg_name, str(p + 1), rb, str(depth)] + ['%s %d' % x for x in order]) + '\n' for p, rb, depth, order in rows)
