"""The restatement of Clair's preprocess/CreateTensor.py (test infrastructure): what OutputAlnTensor writes for a sorted BAM, a
reference sequence and a list of candidate positions, as WHOLE-FILE semantics in plain Python -- no streaming, no flushes, no
dictionaries of open windows.  It works from BAM bytes through tests/bam_in_ref.py and tests/pileup_ref.py;
tests/test_tensor_ref.py pins it to the reference's own output (tests/golden/tensors), and the GPU tests compare the kernels with it.

    records(text)                          -> pileup_ref.records with l_seq, the raw qualities and htslib's reference length
    taken(text, ctg, start, end, mq, dcov) -> the records the script walks, in file order
    joins(rec, c0, left_edge)              -> whether the record joins the centre c0 (0-based)
    high_quality(rec, c0, left_edge)       -> whether it has a high-quality base at the centre
    fill(recs, c0, left_edge, seq, start)  -> the (33, 8, 4) tensor of these records
    tensors(...) / lines(...)              -> [(centre, reference string, tensor)] / the text the reference prints

The rules.  A read joins a centre at join = max(POS, c0 - 16) (with left edges) if it has an M, =, X or D
there; the script then keeps its entries up to c0 + 18, of which c0 - 16 .. c0 + 16 have a tensor index.  An M base is kept from
`join` on, a D base only behind `join` (the script appends a D before it looks the position up), an I only if the next reference
position lies behind `join`.  N, H and P advance nothing, S the read."""
import random

import numpy as np

import bam_in_ref
import pileup_ref
from pileup_ref import M, I, D, N, S, EQ, X, FILTER_FLAG

FLANK = 16
DEPTH = 100
MAX_ITER = 100
QUAL = 7
EXPAND = 100000          # param.expandReferenceRegion
BASE2NUM = dict(zip('ACGTURYSWKMBDHVN', (0, 1, 2, 3, 3, 0, 1, 1, 0, 2, 0, 1, 0, 0, 0, 0)))
CODES = '=ACMGRSVTWYHKDBN'


def records(text):
    out = pileup_ref.records(text)
    for rec, row in zip(out, bam_in_ref.walk(text)):
        rec['l_seq'] = row['l_seq']
        rec['quals'] = text[row['qual']:row['qual'] + row['l_seq']]
        rec['has_qual'] = bool(row['has_qual'])
        rec['span'] = sum(n for op, n in rec['ops'] if op in (M, EQ, X, D))
        rec['hts_len'] = sum(n for op, n in rec['ops'] if op in (M, EQ, X, D, N))
        rec['reverse'] = bool(rec['flag'] & 16)
    return out


def taken(text, ctg_name, ctg_start=None, ctg_end=None, min_mq=10, dcov=1000):
    """What `samtools view -F 2316 bam region` prints and the script does not skip (MQ, then the dcov run)."""
    names = [n for n, _ in pileup_ref.refs(text)]
    out, previous, cap = [], 0, 0
    for rec in records(text):
        if rec['flag'] & FILTER_FLAG or not 0 <= rec['ref_id'] < len(names) or names[rec['ref_id']] != ctg_name:
            continue
        if ctg_start is not None and ctg_end is not None:
            end = rec['pos'] + (rec['hts_len'] or 1)
            if not (rec['pos'] < ctg_end and end > ctg_start - 1):
                continue
        if rec['mapq'] < min_mq:
            continue
        if previous != rec['pos']:
            previous, cap = rec['pos'], 0
        else:
            cap += 1
            if cap >= dcov:
                continue
        out.append(rec)
    return out


def join_pos(rec, c0, left_edge):
    return max(rec['pos'], c0 - FLANK) if left_edge else c0 - FLANK


def joins(rec, c0, left_edge=True):
    a, span = c0 - FLANK, rec['span']
    if span <= 0:
        return False
    if left_edge:
        return rec['pos'] <= c0 + FLANK + 1 and rec['pos'] + span > a
    return rec['pos'] <= a < rec['pos'] + span


def entries(rec, c0, left_edge=True):
    """The entries the script keeps for this read and centre that have a tensor index: ('M', p, code, quality), ('D', p) and
    ('I', p, k, code)."""
    join, last = join_pos(rec, c0, left_edge), c0 + FLANK
    rp, qp = rec['pos'], 0
    for op, n in rec['ops']:
        if op in (M, EQ, X):
            for j in range(max(rp, join) - rp, min(rp + n, last + 1) - rp):
                yield ('M', rp + j, rec['codes'][qp + j], rec['quals'][qp + j])
            rp += n
            qp += n
        elif op == D:
            for p in range(max(rp, join + 1), min(rp + n, last + 1)):
                yield ('D', p)
            rp += n
        elif op == I:
            if join < rp <= last:
                for k in range(n):
                    yield ('I', rp, k, rec['codes'][qp + k])
            qp += n
        elif op == S:
            qp += n
        if rp > last:
            return


def high_quality(rec, c0, left_edge=True):
    for e in entries(rec, c0, left_edge):
        if e[1] == c0 and (e[0] == 'D' or (e[0] == 'M' and e[3] >= QUAL)):
            return True
    return False


def fill(recs, c0, left_edge, seq, ref_start=0):
    t = np.zeros((2 * FLANK + 1, 8, 4), dtype=np.int32)
    for rec in recs:
        strand = 4 if rec['reverse'] else 0
        for e in entries(rec, c0, left_edge):
            index = e[1] - c0 + FLANK
            if e[0] == 'I':
                if e[3]:
                    t[min(index + e[2], 2 * FLANK), BASE2NUM[CODES[e[3]]] + strand, 1] += 1
                continue
            base = seq[e[1] - ref_start]          # IndexError past the end, as in the script
            if base not in BASE2NUM:
                continue
            if e[0] == 'D':
                t[index, BASE2NUM[base] + strand, 2] += 1
            elif e[2]:
                r, q = BASE2NUM[base] + strand, BASE2NUM[CODES[e[2]]] + strand
                t[index, r, 0] += 1
                t[index, q, 1] += 1
                t[index, r, 2] += 1
                t[index, q, 3] += 1
    return t


def reference_window(seq, ctg_start=None, ctg_end=None):
    """-> (the sequence the script loads, its 0-based start)"""
    if ctg_start is not None and ctg_end is not None:
        lo = max(ctg_start - EXPAND, 1)
        return seq[lo - 1:ctg_end + EXPAND], lo - 1
    return seq, 0


def selections(recs, c0, left_edge, rng):
    """The lists of reads the script makes tensors of for one centre, one list per iteration.  recs: those that joined."""
    alignments = list(recs)
    if len(alignments) > DEPTH:
        chosen = set()
        for i, rec in enumerate(alignments):
            if high_quality(rec, c0, left_edge):
                chosen.add(i)
        if len(chosen) > DEPTH:
            alignments = [alignments[i] for i in chosen]        # in the order of the set
    d = len(alignments)
    iterations = min(MAX_ITER, (d + DEPTH - 1) // DEPTH)
    sample = rng.sample(range(d), d)
    if iterations == 1:
        return [alignments]
    out = [[alignments[i] for i in sample[k * DEPTH:(k + 1) * DEPTH]] for k in range(iterations - 1)]
    out.append([alignments[i] for i in sample[-DEPTH:]])
    return out


def tensors(text, seq, positions, ctg_name, ctg_start=None, ctg_end=None, min_mq=10, dcov=1000, min_coverage=0, left_edge=True, rng=random):
    """positions: the 1-based candidate positions in file order -> [(1-based centre, reference string, tensor)]"""
    recs = taken(text, ctg_name, ctg_start, ctg_end, min_mq, dcov)
    window, ref_start = reference_window(seq, ctg_start, ctg_end)
    out = []
    for c in sorted(set(positions)):
        if ctg_start is not None and ctg_end is not None and not ctg_start <= c <= ctg_end:
            continue
        c0 = c - 1
        joined = [r for r in recs if joins(r, c0, left_edge)]
        if not joined:
            continue
        for chosen in selections(joined, c0, left_edge, rng):
            t = fill(chosen, c0, left_edge, window, ref_start)
            at = c - ref_start
            if at - (FLANK + 1) < 0 or int(t[FLANK, :, 0].sum()) < min_coverage:
                break
            out.append((c, window[at - (FLANK + 1):at + FLANK], t))
    return out


def line(ctg_name, centre, ref_string, t):
    return '%s %d %s %s\n' % (ctg_name, centre, ref_string, ' '.join('%d' % x for x in t.reshape(-1).tolist()))


def lines(text, seq, positions, ctg_name, **kw):
    return ''.join(line(ctg_name, c, s, t) for c, s, t in tensors(text, seq, positions, ctg_name, **kw))
