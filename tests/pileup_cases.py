"""Inputs of the pile-up tests (test infrastructure): the golden cases of tests/golden/candidates as BAM files, and constructed
reads.  A BAM is written with bam.encode_record and bam.write_bam from SAM lines, as the mapper's own output is."""
import functools
import json
import os

import bam_in_ref
from megapath_nano_amd import bam

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'candidates', 'candidates_golden.json')


@functools.lru_cache(maxsize=None)
def golden_cases():
    with open(GOLDEN) as f:
        return json.load(f)['cases']


def sam_line(name, flag, ctg, pos1, mapq, cigar, seq, tags=()):
    return '\t'.join([name, str(flag), ctg, str(pos1), str(mapq), cigar, '*', '0', '0', seq, '*'] + list(tags))


def write_bam(path, contigs, sam_lines, level=-1):
    """contigs: [(name, length or sequence)]; sam_lines: SAM records in file order"""
    names = [n for n, _ in contigs]
    lens = [s if isinstance(s, int) else len(s) for _, s in contigs]
    ref_id = {n: i for i, n in enumerate(names)}
    header = ''.join(f'@SQ\tSN:{n}\tLN:{l}\n' for n, l in zip(names, lens))
    bam.write_bam(str(path), header, names, lens, (bam.encode_record(line.split('\t'), ref_id) for line in sam_lines), level=level)
    return str(path)


def write_fasta(path, contigs, width=60):
    with open(path, 'w') as f:
        for n, s in contigs:
            f.write(f'>{n} some words\n')
            f.write(''.join(s[i:i + width] + '\n' for i in range(0, len(s), width)))
    return str(path)


def text_of(path):
    with open(path, 'rb') as f:
        return bam_in_ref.inflate(f.read())


def write_case(tmp_path, case):
    """-> (bam path, fasta path, bed path or None) of a golden case"""
    d = os.path.join(str(tmp_path), case['name'])
    os.makedirs(d, exist_ok=True)
    bam_fn = write_bam(os.path.join(d, 'in.bam'), [tuple(c) for c in case['contigs']], case['reads'])
    ref_fn = write_fasta(os.path.join(d, 'ref.fa'), case['contigs'])
    bed_fn = None
    if case['bed'] is not None:
        bed_fn = os.path.join(d, 'in.bed')
        with open(bed_fn, 'w') as f:
            f.write(case['bed'])
    return bam_fn, ref_fn, bed_fn


def read_for(rng, ref, pos0, cigar, sub=0.1):
    """Bases for a read at pos0 (0-based) along a CIGAR text: the reference under M, = and X with a fraction `sub` replaced by a
    random letter of ACGTN and the IUPAC codes, random ACGT under I and S; past the end of the reference A.  rng: random.Random."""
    out, r, num = [], pos0, 0
    for ch in cigar:
        if ch.isdigit():
            num = num * 10 + int(ch)
            continue
        if ch in 'M=X':
            for _ in range(num):
                b = ref[r] if 0 <= r < len(ref) else 'A'
                out.append(rng.choice('ACGTNRYSWKMBDHV') if rng.random() < sub else b)
                r += 1
        elif ch in 'IS':
            out.append(''.join(rng.choice('ACGT') for _ in range(num)))
        elif ch in 'DN':
            r += num
        num = 0
    return ''.join(out)


def random_contig(rng, n):
    return ''.join(rng.choice('ACGT') for _ in range(n))


def ont_reads(seed, contig, depth, read_len, name='r'):
    """SAM lines of reads with the ONT error mix of synth.aligned_read, uniform starts, sorted by position"""
    import numpy as np
    from megapath_nano_amd import synth
    rng = np.random.default_rng(seed)
    g = np.frombuffer(contig[1].encode(), dtype=np.uint8)
    n = max(1, len(g) * depth // read_len)
    starts = np.sort(rng.integers(0, len(g) - read_len + 1, size=n))
    out = []
    for i, s in enumerate(starts.tolist()):
        cigar, seq = synth.aligned_read(rng, g, s, read_len)
        out.append(sam_line(f'{name}{i}', 16 if i & 1 else 0, contig[0], s + 1, int(rng.integers(0, 61)), cigar, seq.decode()))
    return out
