"""Inputs of the call tests (test infrastructure): constructed reads as SAM lines, sites, tensors and probabilities, the same for the
host build (tests/test_clair_call_host.py) and the device (tests/test_clair_call_gpu.py, tests/test_call_indels_gpu.py), and what
the restatement (tests/clair_call_ref.py) says of them."""
import functools
import random
import struct

import numpy as np

import clair_call_ref as ref
import pileup_cases as pc

CTG = 'ctgC'


def contig(seed=5, n=400):
    rng = random.Random(seed)
    return ''.join(rng.choice('ACGT') for _ in range(n))


def sam(name, flag, pos0, cigar, seq):
    return '\t'.join([name, str(flag), CTG, str(pos0 + 1), '60', cigar, '*', '0', '0', seq, 'I' * len(seq) if seq != '*' else '*'])


def random_cigar(rng, lo=1, hi=30, ops=8, long_events=False):
    """M blocks with an event between them: I, D, N, P I, I P I, D I (an insertion right after a deletion)"""
    parts = [('M', rng.randint(lo, hi))]
    for _ in range(rng.randint(0, ops)):
        kind = rng.choice(['I', 'D', 'D', 'I', 'N', 'PI', 'IPI', 'DI', 'none'])
        n = rng.choice([1, 1, 2, 3, 15, 16, 17, 50, 51]) if long_events else rng.randint(1, 4)
        if kind == 'I':
            parts.append(('I', n))
        elif kind == 'D':
            parts.append(('D', n))
        elif kind == 'N':
            parts.append(('N', rng.randint(1, 5)))
        elif kind == 'PI':
            parts += [('P', 1), ('I', n)]
        elif kind == 'IPI':
            parts += [('I', 1), ('P', 2), ('I', n)]
        elif kind == 'DI':
            parts += [('D', rng.randint(1, 3)), ('I', n)]
        parts.append(('M', rng.randint(lo, hi)))
    return parts


def line_of(rng, name, flag, pos0, parts, soft=0):
    cigar = ('%dS' % soft if soft else '') + ''.join('%d%s' % (n, op) for op, n in parts)
    q = soft + sum(n for op, n in parts if op in 'MI=X')
    return sam(name, flag, pos0, cigar, ''.join(rng.choice('ACGT') for _ in range(q)))


def random_reads(seed, n, lo=60, hi=130, long_events=False, starts=None):
    """n reads that start in [lo, hi) (or at `starts`), sorted by position; flags 0, 16 and a few that the filter drops"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        pos0 = rng.choice(starts) if starts else rng.randrange(lo, hi)
        flag = rng.choice([0, 0, 0, 16, 16, 4, 256, 2048, 1024])
        out.append((pos0, i, line_of(rng, 'r%d' % i, flag, pos0, random_cigar(rng, long_events=long_events), soft=rng.choice([0, 0, 3]))))
    out.sort(key=lambda t: (t[0], t[1]))
    return [t[2] for t in out]


def window(seq, site):
    """the reference string of a 1-based site"""
    return seq[max(site - 17, 0):site + 16]


def random_tensor(rng):
    x = np.zeros((33, 8, 4), dtype=np.int32)
    x[...] = np.array([[[rng.randint(0, 30) for _ in range(4)] for _ in range(8)] for _ in range(33)], dtype=np.int32)
    if rng.random() < 0.05:
        x[16, :, 0] = 0
        x[16, :, 2] = 0
    return x


def random_probs(rng, style):
    """90 float32: eighths (many exact ties between and within the lists), peaked draws, or all zero"""
    if style == 'zero':
        return np.zeros(90, dtype=np.float32)
    if style == 'eighths':
        return np.array([rng.choice([0, 0, 1, 2, 4, 8]) / 8 for _ in range(90)], dtype=np.float32)
    out = []
    for size, peaks in ((21, 2), (3, 1), (33, 2), (33, 2)):
        v = np.array([rng.random() * 0.02 for _ in range(size)])
        for _ in range(peaks):
            v[rng.randrange(size)] += rng.random()
        out.append(v / v.sum())
    return np.concatenate(out).astype(np.float32)


def decode_case(seed, n_sites=120, reads=160, long_events=False, seq=None):
    """{'seq', 'lines', 'sites' (ascending 1-based), 'x' (n, 33, 8, 4), 'probs' (n, 90), 'refs'}"""
    rng = random.Random(seed)
    seq = seq or contig()
    lines = random_reads(seed + 1, reads, long_events=long_events)
    sites = sorted(rng.sample(range(40, 200), n_sites))
    styles = ['peaked'] * 6 + ['eighths'] * 3 + ['zero']
    return dict(seq=seq, lines=lines, sites=sites, x=np.stack([random_tensor(rng) for _ in sites]),
                probs=np.stack([random_probs(rng, rng.choice(styles)) for _ in sites]), refs=[window(seq, s) for s in sites])


@functools.lru_cache(maxsize=None)
def cached_case(seed, n_sites=120, reads=160, long_events=False):
    return decode_case(seed, n_sites, reads, long_events)


def reset_case():
    """two deletions of 3 and 5 bases win at a site two bases before the end of the contig: the fetched bases are clipped to 2, both
    alternates would be the centre alone, the loop resets and goes on to the reference call"""
    seq, rng = contig(), random.Random(9)
    site = len(seq) - 2
    probs = np.zeros(90, dtype=np.float32)
    probs[10] = probs[23] = probs[24 + 16 - 3] = probs[57 + 16 - 5] = 1
    x = random_tensor(rng)
    x[16, 0, 0] = 7
    return dict(seq=seq, lines=[line_of(rng, 'end', 0, site - 20, [('M', 20), ('D', 5), ('M', 5)])], sites=[site], x=x[None], probs=probs[None],
                refs=[window(seq, site)])


def insdel_case():
    """three reads with an insertion directly followed by a deletion (the pile-up spells `+2xx-2NN`, the script takes `XX-2NN` for
    the inserted bases), one with a deletion too long for the key; a homozygous insertion of 2 wins at site 100"""
    seq, rng = contig(), random.Random(10)
    body = [('M', 20), ('I', 2), ('D', 2), ('M', 20)]
    first = line_of(rng, 'a', 0, 80, body)
    lines = [first, first.replace('a\t0', 'b\t16', 1), line_of(rng, 'c', 0, 80, body), line_of(rng, 'd', 0, 80, [('M', 20), ('I', 3), ('D', 46), ('M', 20)])]
    probs = np.zeros((2, 90), dtype=np.float32)
    probs[0, 15] = probs[0, 22] = probs[0, 24 + 18] = probs[0, 57 + 18] = 1          # homo insertion of 2
    probs[1, 15] = probs[1, 22] = probs[1, 24 + 19] = probs[1, 57 + 19] = 1          # homo insertion of 3: the key is too long
    x = random_tensor(rng)
    x[16, 0, 0] = 5
    return dict(seq=seq, lines=lines, sites=[100, 100], x=np.stack([x, x]), probs=probs, refs=[window(seq, 100)] * 2)


def fetcher(seq):
    return lambda a, b: seq[a:b]


def expected_events(case):
    reads = [ref.read_of(l) for l in case['lines']]
    return [ref.events_of(ref.closed_sequences(reads, s), s, len(case['seq'])) for s in case['sites']]


def expected_rows(case, pysam_all=False, haploid=False, show_ref=False, qual=None, trace=None):
    """[(line, parts) or None per site] by the restatement in 'legacy'"""
    reads = [ref.read_of(l) for l in case['lines']]
    fetch = fetcher(case['seq'])
    out = []
    for s, x, p, r in zip(case['sites'], case['x'], case['probs'], case['refs']):
        out.append(ref.output_with(CTG, s, r, x, p, ref.closed_sequences(reads, s), fetch, pysam_all, haploid, show_ref, qual, 'legacy', trace))
    return out


# ---- for the host build ----------------------------------------------------------------------------------------------------------------
def bam_text_reads(bam_path):
    """the text of a BAM file and its records that pass the flag filter -> (bytes, [(off, rlen, pos, reverse)])"""
    text = pc.text_of(bam_path)
    l_text, = struct.unpack_from('<i', text, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from('<i', text, at)
    at += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from('<i', text, at)
        at += 8 + l_name
    reads = []
    while at < len(text):
        size, = struct.unpack_from('<i', text, at)
        pos, = struct.unpack_from('<i', text, at + 8)
        l_name = text[at + 12]
        n_cigar, flag = struct.unpack_from('<HH', text, at + 16)
        rlen = 0
        for k in range(n_cigar):
            w, = struct.unpack_from('<I', text, at + 36 + l_name + 4 * k)
            if (w & 15) in (0, 2, 3, 7, 8):
                rlen += w >> 4
        if not flag & ref.FILTER_FLAG:
            reads.append((at, rlen, pos, 1 if flag & 16 else 0))
        at += 4 + size
    return text, reads


def host_case_bytes(text, reads, contig_bytes, sites, ranges, refs, x, probs, options):
    out = [struct.pack('<5q', len(text), len(reads), len(sites), len(contig_bytes), options), text]
    out += [struct.pack('<qqii', *r) for r in reads]
    out.append(contig_bytes)
    for s, (b, e), r, t, p in zip(sites, ranges, refs, x, probs):
        out.append(struct.pack('<iiqq', s, len(r), b, e) + r.encode().ljust(33, b'\0'))
        out.append(np.ascontiguousarray(t, dtype='<i4').tobytes() + np.ascontiguousarray(p, dtype='<f4').tobytes())
    return b''.join(out)


# ---- the fixture recorded from the reference's own call_var.py (tests/golden/make_clair_call_golden.py) --------------------------------------
GOLDEN = __import__('os').path.join(__import__('os').path.dirname(__import__('os').path.abspath(__file__)), 'golden', 'clair_call', 'clair_call_golden.json.gz')


@functools.lru_cache(maxsize=None)
def golden():
    import gzip
    import json
    with gzip.open(GOLDEN, 'rt') as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def golden_case(name):
    """a case of the fixture as the other cases are, with its options and the reference's records"""
    g = next(c for c in golden()['cases'] if c['name'] == name)
    rows = [l.split('\t') for l in g['input'].splitlines()]
    o = g['options']
    return dict(seq=g['seq'], lines=g['lines'], sites=[int(r[1]) for r in rows], refs=[r[2] for r in rows],
                x=np.array([r[3:3 + 1056] for r in rows], dtype=np.float32).astype(np.int32).reshape(-1, 33, 8, 4),
                probs=np.array([r[3 + 1056:] for r in rows], dtype=np.float32), options=o, input=g['input'], vcf=g['vcf'],
                kw=dict(pysam_all='--pysam_for_all_indel_bases' in o, haploid='--haploid' in o, show_ref='--showRef' in o,
                        qual=int(o[o.index('--qual') + 1]) if '--qual' in o else None))


GOLDEN_NAMES = ['all_bases', 'tensor_bases', 'haploid', 'tensor_bases_long', 'reset', 'insdel', 'deep']


def records(vcf):
    return [l for l in vcf.splitlines() if not l.startswith('#')]


def without_float64_columns(line):
    """a record without QUAL, GQ and AF: the columns that hang on NumPy's promotion"""
    f = line.split('\t')
    s = f[9].split(':')
    return f[:5] + f[6:9] + [s[0], s[2]]
