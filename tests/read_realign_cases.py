"""Constructed inputs for the tests of megapath_nano_amd/read_realign.py: records as SAM fields with explicitly typed aux fields, the
BAM file, the inflated BAM text and the SAM lines `samtools view` prints for them.  A case is dict(name, contig: its FASTA text as
it stands (case kept), records: [dict(pos, cigar, seq, qual, mapq, flag, aux, rnext, pnext; patch: a function applied to the bytes
of the BAM record)], min_mq, min_coverage, contigs: other references of the header).  Read bases follow the script's own walk of the CIGAR (an N does not move its reference position)."""
import glob
import gzip
import json
import os
import random
import struct

from megapath_nano_amd import bam

CTG = 'ctg'
OTHER = 'other'
HEADER = '@HD\tVN:1.6\tSO:coordinate\n'


def contig(n, seed, last='A'):
    rng = random.Random(seed)
    return ''.join(rng.choice('ACGT') for _ in range(n - 1)) + last


def ops_of(cigar):
    out, num = [], 0
    for ch in cigar:
        if ch.isdigit():
            num = num * 10 + int(ch)
        else:
            out.append((num, ch))
            num = 0
    return out


def read(ctg, pos, cigar, rng, mism=(), low=(), q=30, mapq=60, flag=0, aux=(), bases=None, rnext='*', pnext=0, fill=None):
    """A record whose bases equal the (upper-cased) contig under M, = and X by the script's walk, except at the query indices of
    `mism` (the next base of ACGT, or the letter given in a dict); inserted and clipped bases are random (or `fill`: a letter, or
    a list with the bases of every I and S in turn).  low: query
    indices of quality 19 (or a dict index -> quality)."""
    up = ctg.upper()
    seq, rp = [], pos
    for n, op in ops_of(cigar):
        if op in 'M=X':
            seq += [up[rp + i] if up[rp + i] in 'ACGT' else 'A' for i in range(n)]
            rp += n
        elif op in 'IS':
            seq += list(fill.pop(0)) if isinstance(fill, list) else [fill or rng.choice('ACGT') for _ in range(n)]
        elif op == 'D':
            rp += n
    for i in (mism if isinstance(mism, dict) else dict.fromkeys(mism)):
        seq[i] = (mism[i] if isinstance(mism, dict) and mism[i] else 'ACGT'[('ACGT'.index(seq[i]) + 1) % 4])
    qual = [q] * len(seq)
    for i in (low if isinstance(low, dict) else dict.fromkeys(low, 19)):
        qual[i] = low[i] if isinstance(low, dict) else 19
    return dict(pos=pos, cigar=cigar, seq=bases if bases is not None else ''.join(seq), qual=''.join(chr(x + 33) for x in qual), mapq=mapq, flag=flag,
                aux=list(aux), rnext=rnext, pnext=pnext)


_INT = {'c': '<b', 'C': '<B', 's': '<h', 'S': '<H', 'i': '<i', 'I': '<I'}


def aux_bytes(aux):
    out = b''
    for tag, typ, val in aux:
        t = tag.encode()
        if typ in _INT:
            out += t + typ.encode() + struct.pack(_INT[typ], val)
        elif typ == 'A':
            out += t + b'A' + val.encode()
        elif typ == 'f':
            out += t + b'f' + struct.pack('<f', val)
        elif typ in 'ZH':
            out += t + typ.encode() + val.encode() + b'\0'
        else:                                   # ('B', (subtype, [values]))
            sub, items = val
            out += t + b'B' + sub.encode() + struct.pack('<I', len(items)) + b''.join(struct.pack(_INT.get(sub, '<f'), x) for x in items)
    return out


def aux_text(aux):
    out = []
    for tag, typ, val in aux:
        if typ in _INT:
            out.append(f'{tag}:i:{val}')
        elif typ == 'f':
            out.append(f'{tag}:f:{val:g}')
        elif typ == 'B':
            out.append(f'{tag}:B:{val[0]},' + ','.join(str(x) for x in val[1]))
        else:
            out.append(f'{tag}:{typ}:{val}')
    return out


def fields(case, k, r):
    return [f'r{k}', str(r['flag']), r.get('rname', CTG), str(r['pos'] + 1), str(r['mapq']), r['cigar'], r['rnext'], str(r['pnext']), '0', r['seq'], r['qual']]


def references(case):
    return [(CTG, len(case['contig']))] + list(case.get('contigs', [(OTHER, 1000)]))


def sam_lines(case):
    """the lines of `samtools view` (without the header), tab-separated"""
    return ['\t'.join(fields(case, k, r) + aux_text(r['aux'])) + '\n' for k, r in enumerate(case['records'])]


def header_text(case):
    return HEADER + ''.join(f'@SQ\tSN:{n}\tLN:{l}\n' for n, l in references(case))


def bam_records(case):
    ref_id = {n: i for i, (n, _) in enumerate(references(case))}
    for k, r in enumerate(case['records']):
        tid, pos0, end0, flag, rec = bam.encode_record(fields(case, k, r), ref_id)
        rec += aux_bytes(r['aux'])
        yield tid, pos0, end0, flag, r['patch'](rec) if r.get('patch') else rec


def write_case(tmp, case):
    """-> (the BAM's path, the FASTA's path)"""
    refs = references(case)
    bam_fn, ref_fn = os.path.join(str(tmp), case['name'] + '.bam'), os.path.join(str(tmp), case['name'] + '.fa')
    bam.write_bam(bam_fn, header_text(case), [n for n, _ in refs], [l for _, l in refs], bam_records(case))
    with open(ref_fn, 'w') as f:
        f.write(f'>{OTHER}\nACGTACGTAC\n>{CTG} the contig\n')
        f.write(''.join(case['contig'][i:i + 60] + '\n' for i in range(0, len(case['contig']), 60)))
    return bam_fn, ref_fn


def text_of(case):
    """-> (the inflated BAM text, the offsets of its records)"""
    refs = references(case)
    head = header_text(case).encode()
    text = bytearray(b'BAM\1' + struct.pack('<i', len(head)) + head + struct.pack('<i', len(refs)))
    for n, l in refs:
        text += struct.pack('<i', len(n) + 1) + n.encode() + b'\0' + struct.pack('<i', l)
    offs = []
    for _, _, _, _, rec in bam_records(case):
        offs.append(len(text))
        text += struct.pack('<i', len(rec)) + rec
    return bytes(text), offs


def case(name, ctg, records, min_mq=5, min_coverage=2):
    records = sorted(records, key=lambda r: r['pos'])          # (stable: records of one position stay in the order given)
    return dict(name=name, contig=ctg, records=records, min_mq=min_mq, min_coverage=min_coverage)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def long_cigars():
    """CIGARs of 63, 64, 65 and 130 operations (1M alternating with 1D and 1I), twice each: every indel is a candidate"""
    ctg, rng, recs = contig(3000, 1), random.Random(2), []
    for j, n_ops in enumerate((63, 64, 65, 130)):
        cigar = '20M' + ''.join(('2M1D', '2M1I')[i & 1] for i in range((n_ops - 2) // 2)) + ('3M' if n_ops & 1 else '') + '20M'
        assert len(ops_of(cigar)) == n_ops, (n_ops, len(ops_of(cigar)))
        recs += [read(ctg, 100 + 600 * j + d, cigar, rng) for d in (0, 3)]
    return case('long_cigars', ctg, recs)


def long_insertions():
    """an insertion and a soft clip of 65 and 130 bases: all of quality 30 (they count), and with a single base of quality 19 in the
    last step of 64 (they do not)"""
    ctg, rng, recs = contig(4000, 3), random.Random(4), []
    for j, n in enumerate((65, 130)):
        at = 200 + 900 * j
        for low in ((), (20 + n - 1,)):
            recs += [read(ctg, at + d, f'20M{n}I100M', rng, low=low) for d in (0, 2)]
            at += 400
        at = 2200 + 800 * j
        for low in ((), (n - 1,)):
            recs += [read(ctg, at + d, f'{n}S{2 * n}M', rng, low=low) for d in (0, 2)]
            at += 400
    return case('long_insertions', ctg, recs)


def chunk_edges():
    """counts at chunk_start - 22 / -21 and chunk_end + 19 / + 20 of the second chunk, deletions at chunk_end + 20 / + 21 of the first
    (the second is out of its record's region), a clip of the record that triggers the first yield reaching back into the first
    row, a dropped record that triggers the second yield, and a record at POS 0 whose leading clip reaches below 0 (the base before
    is the contig's last: N in one case, A in the other)"""
    out = []
    for last in 'NA':
        ctg, rng, recs = contig(16000, 5, last), random.Random(6), []
        recs += [read(ctg, 0, '10S60M', rng) for _ in range(2)]                                   # chunk 0 starts at 0
        for p in (4978, 4979, 10019, 10020):                                                      # mismatches, twice each
            recs += [read(ctg, p - 30, '80M', rng, mism=(30,)) for _ in range(2)]
        for p in (5020, 5021):                                                                    # a deletion at chunk_end + 20 / + 21
            recs += [read(ctg, p - 31, '31M3D40M', rng) for _ in range(2)]
        recs += [read(ctg, 5030, '30S70M', rng) for _ in range(2)]                                # behind the trigger at 5020
        recs += [read(ctg, 10025, '60S40M', rng), read(ctg, 10030, '*', rng, bases='ACGT' * 10)]    # dropped: too clipped; no CIGAR
        recs[-1]['qual'] = 'I' * 40
        recs += [read(ctg, 10100, '50M', rng, mism=(7,)) for _ in range(2)]
        out.append(case('chunk_edges_' + last, ctg, recs))
    return out


def lagging_chunks():
    """a coverage gap of 11 000 bases: the chunks lag behind the records, whose indels are then out of region while their
    mismatches still count"""
    ctg, rng, recs = contig(16000, 7), random.Random(8), []
    recs += [read(ctg, 50 + d, '40M2D40M', rng, mism=(10,)) for d in (0, 1, 2)]
    for at in (11200, 11400, 14000, 15500):
        recs += [read(ctg, at + d, '40M2D20M3I20M', rng, mism=(10,)) for d in (0, 1, 2)]
    return case('lagging_chunks', ctg, recs)


def qualities_and_letters():
    """MAPQ 13 / 14 and 19 / 20, N, H and P operations, lower-case contig bases, IUPAC read bases, HP tags of each integer type and
    the aux types that are walked over"""
    ctg = contig(3000, 9)
    ctg = ctg[:600] + ctg[600:900].lower() + ctg[900:1500] + 'NNRY' + ctg[1504:]
    rng, recs = random.Random(10), []
    for j, mapq in enumerate((13, 14, 19, 20)):
        recs += [read(ctg, 100 + 120 * j + d, '30M2D30M', rng, mism=(5,), mapq=mapq) for d in (0, 1)]
    recs += [read(ctg, 650 + d, '40M1I40M', rng, mism=(12, 60)) for d in (0, 1, 2)]                # over lower-case bases
    recs += [read(ctg, 1000 + d, '5H20M10N20M2P20M5H', rng, mism=(25, 45)) for d in (0, 1)]         # N does not move the script's position
    recs += [read(ctg, 1200 + d, '60M', rng, mism={10: 'R', 11: 'N', 12: 'Y', 13: 'M'}) for d in (0, 1)]
    recs += [read(ctg, 1470 + d, '60M', rng, mism=(20,)) for d in (0, 1)]                          # over N, N, R, Y of the contig
    recs += [read(ctg, 1700 + d, '20=5X20M', rng, mism=(22, 30)) for d in (0, 1)]
    tags = [('c', 1), ('c', -1), ('C', 2), ('s', 300), ('s', -2), ('S', 4000), ('i', 70000), ('i', -5), ('I', 3000000000), ('C', 0)]
    for j, (typ, val) in enumerate(tags):
        recs.append(read(ctg, 2000 + 10 * j, '50M', rng, mism=(9,), aux=[('NM', 'C', 1), ('XA', 'A', 'x'), ('XF', 'f', 1.5), ('XZ', 'Z', 'a HP:Z:i text'),
                                                                       ('XH', 'H', '1AE3'), ('XB', 'B', ('s', [1, -2, 3])), ('HP', 'Z', '7'), ('HP', typ, val),
                                                                       ('HP', 'C', 9), ('XC', 'B', ('f', [0.5]))],
                         flag=16 if j & 1 else 0, rnext='=' if j % 3 == 0 else (OTHER if j % 3 == 1 else '*'), pnext=0 if j % 3 == 2 else 100 + j))
    return case('qualities_and_letters', ctg, recs)


def windows():
    """a candidate in the overlap of two splits, candidates 160 and 161 apart, windows of 1000 and 1001 bases, a read that overlaps
    two windows by the same length and one that overlaps none"""
    ctg, rng, recs = contig(12000, 11), random.Random(12), []
    recs += [read(ctg, 0, '50M', rng)]                                                            # chunk 0 starts at 0

    def snp(p, n=2):
        return [read(ctg, p - 20 - d, '60M', rng, mism=(20 + d,)) for d in range(n)]
    recs += snp(990) + snp(1000)                                 # split 0 ends at 1020, split 1 starts at 979: both hold both candidates
    recs += snp(2100) + snp(2260)                                # one window
    recs += snp(3100) + snp(3261)                                # two windows
    recs += [read(ctg, 3131, '100M', rng)]                       # 3131 .. 3231: 49 bases of [3020, 3180) and 50 of [3181, 3341)
    recs += [read(ctg, 3130, '101M', rng)]                       # 50 and 50: the first
    for k in range(7):                                           # 5000 .. 5840: a window of 1000 bases, in the chunk that starts at 5000
        recs += snp(5100 + 140 * k)
    for k in range(7):                                           # a window of 1001 bases in the next chunk: not realigned
        recs += snp(10100 + 140 * k + (1 if k == 6 else 0))
    recs += [read(ctg, 11500, '50M', rng)]
    return case('windows', ctg, recs)


def deep_window(n=1001):
    """a window with 1001 reads of 40 bases: the first 1000 go to the realigner, all of them build the graph"""
    ctg, rng, recs = contig(1500, 13), random.Random(14), []
    for k in range(n):
        at = 300 + (k % 8)
        recs.append(read(ctg, at, '20M2D20M' if k % 3 == 0 else '40M', rng, mism=() if k % 3 == 0 else (330 - at,)))
    return case('deep_window', ctg, recs)


def plain_variants(seed=21, n=4000, depth=12, length=100):
    """reads of `length` bases at `depth` over a contig with planted SNPs, insertions and deletions, aligned as a mapper that misses
    the indels near read ends would (soft clips there): what the realignment is for"""
    rng = random.Random(seed)
    ctg = contig(n, seed + 1)
    sites = sorted(rng.sample(range(200, n - 200, 37), 6))
    recs = []
    for start in range(0, n - length - 5, max(1, length // depth)):
        pos, cigar, mism, qp, rp, done, fills = start, [], [], 0, start, set(), []
        while qp < length:
            nxt = next((s for s in sites if s >= rp and s not in done), None)
            run = length - qp if nxt is None else min(length - qp, nxt - rp)
            if run:
                cigar.append(f'{run}M')
                qp, rp = qp + run, rp + run
            if qp >= length or nxt is None:
                break
            kind = sites.index(nxt) % 3
            done.add(nxt)
            if kind == 0:
                mism.append(qp)
                cigar.append('1M')
                qp, rp = qp + 1, rp + 1
            elif length - qp < 12:                               # an indel near the end: the mapper clips
                cigar.append(f'{length - qp}S')
                fills.append((ctg[rp + 3:] if kind == 1 else 'GGGG' + ctg[rp:])[:length - qp])
                qp = length
            elif kind == 1:
                cigar.append('3D')
                rp += 3
            else:
                k = min(4, length - qp)
                cigar.append(f'{k}I')
                fills.append('GGGG'[:k])
                qp += k
        merged = []
        for n_, op in ops_of(''.join(cigar)):
            if merged and merged[-1][1] == op:
                merged[-1][0] += n_
            else:
                merged.append([n_, op])
        recs.append(read(ctg, pos, ''.join(f'{a}{b}' for a, b in merged), rng, mism=mism, fill=fills, mapq=rng.choice((60, 60, 30, 15)),
                         low=rng.sample(range(length), 3), aux=[('HP', 'C', 1 + start % 2)] if start % 5 else []))
    return case(f'plain_variants_{seed}', ctg, recs)


def edge_cases():
    return [long_cigars(), long_insertions()] + chunk_edges() + [lagging_chunks(), qualities_and_letters(), windows()]


# ---- the goldens ----------------------------------------------------------------------------------------------------------------
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'read_realign', '*.json.gz')))


def load_golden(path):
    """-> (what tests/golden/make_read_realign_golden.py stored, the case it names, generated again)"""
    with open(path, 'rb') as f:
        gold = json.loads(gzip.decompress(f.read()))
    fn, kw, index = gold['generator']
    got = globals()[fn](**kw)
    got = got if index is None else got[index]
    assert got['name'] == gold['name'] and (got['min_mq'], got['min_coverage']) == (gold['args']['minMQ'], gold['args']['minCoverage'])
    if 'sam_lines' in gold:
        assert gold['sam_lines'] == sam_lines(got) and gold['contig'] == got['contig']
    return gold, got
