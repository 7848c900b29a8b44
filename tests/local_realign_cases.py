"""Inputs of the local-realignment tests (test infrastructure): the constructed cases that tests/golden/make_local_realign_golden.py
records with the reference's own programs, the goldens themselves, and further constructed reads for the GPU tests."""
import functools
import gzip
import json
import os
import random

import clair_call_ref as ccr
import pileup_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'local_realign', 'local_realign_golden.json.gz')
DEEP_GOLDEN = os.path.join(HERE, 'golden', 'local_realign', 'local_realign_deep.json')
CTG = 'ctgLR'


def span_read(rng, seq, name, start1, cigar, flag=0, sub=0.0):
    """a SAM line of a read at the 1-based start along `cigar`"""
    return pc.sam_line(name, flag, CTG, start1, 60, cigar, pc.read_for(rng, seq, start1 - 1, cigar, sub))


def mutate(line, at0, base):
    f = line.split('\t')
    f[9] = f[9][:at0] + base + f[9][at0 + 1:]
    return '\t'.join(f)


def vcf_text(seq, rows):
    """rows: (pos, ref, alt) -> a VCF as mpn-call-vcf writes it"""
    head = '##fileformat=VCFv4.1\n##contig=<ID=%s,length=%d>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n' % (CTG, len(seq))
    return head + ''.join('%s\t%d\t.\t%s\t%s\t100\t.\t.\tGT:GQ:DP:AF\t0/1:100:30:0.5000\n' % (CTG, p, r, a) for p, r, a in rows)


def other(base):
    return 'ACGT'[('ACGT'.index(base) + 1) % 4]


def constructed_cases():
    """[{name, seq, lines, positions, vcf}]: about a dozen cases of at most 60 reads"""
    out = []

    def add(name, seq, lines, positions, rows=None):
        lines = sorted(lines, key=lambda l: int(l.split('\t')[3]))       # (stable: file order within a start)
        rows = rows if rows is not None else [(p, seq[p - 1], other(seq[p - 1])) for p in positions]
        out.append(dict(name=name, seq=seq, lines=lines, positions=list(positions), vcf=vcf_text(seq, rows)))

    rng = random.Random(2401)
    seq = pc.random_contig(rng, 1600)
    pos = 800
    # a SNP carried by 12 of 30 reads; the VCF has the position twice and a second site without the SNP
    lines = []
    for i in range(30):
        s = 400 + 5 * i
        l = span_read(rng, seq, f'snp{i}', s, '600M')
        lines.append(mutate(l, pos - s, other(seq[pos - 1])) if i % 5 < 2 else l)
    add('snp', seq, lines, [pos, 900], [(pos, seq[pos - 1], other(seq[pos - 1])), (900, seq[899], other(seq[899])), (pos, seq[pos - 1], other(seq[pos - 1]))])
    # an insertion behind the site, a deletion behind it, both strands
    lines = []
    for i in range(24):
        s = 450 + 7 * i
        a = pos - s + 1
        cig = f'{a}M3I{560 - a}M' if i % 3 == 0 else (f'{a}M4D{560 - a}M' if i % 3 == 1 else '560M')
        lines.append(span_read(rng, seq, f'id{i}', s, cig, flag=16 if i & 1 else 0))
    ins = lines[0].split('\t')[9][pos - 450 + 1:pos - 450 + 4]
    add('indel', seq, lines, [pos], [(pos, seq[pos - 1], seq[pos - 1] + ins), (pos, seq[pos - 1:pos + 4], seq[pos - 1])])
    # bases that are not ACGT, in matched stretches and insertions
    lines = [span_read(rng, seq, f'iu{i}', 380 + 11 * i, f'{300 + i}M{1 + i % 4}I{250 - i}M', sub=0.15) for i in range(20)]
    add('iupac', seq, lines, [700, pos])
    # flags: supplementary is kept; unmapped, secondary, QC fail and duplicate are not
    lines = [span_read(rng, seq, f'fl{i}', 500 + 3 * i, '500M', flag=f, sub=0.02)
             for i, f in enumerate([0, 16, 2048, 2064, 256, 512, 1024, 4, 272, 0, 2048, 1040, 0, 16])]
    add('flags', seq, lines, [pos])
    # no column for a while before the centre: skipped; after the centre: the walk stops there
    lines = [span_read(rng, seq, f'gb{i}', 560 + i, f'{100 + i}M', sub=0.02) for i in range(6)] + \
            [span_read(rng, seq, f'gc{i}', 720 + i, '400M', sub=0.02) for i in range(8)]
    add('gap_before', seq, lines, [pos])
    lines = [span_read(rng, seq, f'ga{i}', 600 + i, f'{280 - 2 * i}M', sub=0.02) for i in range(8)] + \
            [span_read(rng, seq, f'gd{i}', 930 + i, '300M', sub=0.02) for i in range(6)]
    add('gap_after', seq, lines, [pos])
    # the edges of the window
    lo, hi = pos - 200, pos + 200
    lines = [span_read(rng, seq, 'e_all', 300, '900M'),
             span_read(rng, seq, 'e_lo', lo, '300M'), span_read(rng, seq, 'e_hi', hi, '80M'), span_read(rng, seq, 'e_hi1', hi + 1, '80M'),
             span_read(rng, seq, 'e_end', lo - 100, '99M'), span_read(rng, seq, 'e_end1', lo - 100, '100M'),
             span_read(rng, seq, 'e_insl', lo - 50, '49M2I200M'), span_read(rng, seq, 'e_insl1', lo - 50, '50M2I200M'),
             span_read(rng, seq, 'e_insh', hi - 100, '100M2I50M'), span_read(rng, seq, 'e_insh1', hi - 100, '101M2I50M'),
             span_read(rng, seq, 'e_dello', lo - 30, '25M10D300M'), span_read(rng, seq, 'e_delc', pos - 100, '98M5D200M'),
             span_read(rng, seq, 'e_deli', pos - 150, '100M3D2I200M'), span_read(rng, seq, 'e_lead', pos - 20, '5S3I100M4I6S'),
             span_read(rng, seq, 'e_hard', pos - 10, '7H60M3I'), span_read(rng, seq, 'e_ii', pos - 60, '30M2I3I90M')]
    add('edges', seq, lines, [pos, pos + 1])
    # a site 100 bases before the end of the contig, and the first site that is taken
    lines = [span_read(rng, seq, f'ce{i}', 1100 + 9 * i, f'{501 - 9 * i}M', sub=0.03) for i in range(20)]
    add('contig_end', seq, lines, [1500, 1590])
    lines = [span_read(rng, seq, f'cs{i}', 1 + 4 * i, '550M', sub=0.03) for i in range(20)]
    add('contig_start', seq, lines, [301, 320])
    # reads with the ONT error mix: several sites, clipped SSW alignments among them
    big = pc.random_contig(random.Random(2402), 3000)
    lines = pc.ont_reads(2403, (CTG, big), 30, 1500, name='ont')[:60]
    add('ont', big, lines, [700, 1200, 1500, 1501, 2300])
    return out


@functools.lru_cache(maxsize=None)
def golden_cases():
    with gzip.open(GOLDEN, 'rt') as f:
        return json.load(f)['cases']


def reads_of(case):
    return [ccr.read_of(l) for l in case['lines']]


def write_case(tmp_path, case, name=None):
    """-> (bam path, fasta path, vcf path)"""
    d = os.path.join(str(tmp_path), name or case['name'])
    os.makedirs(d, exist_ok=True)
    bam_fn = pc.write_bam(os.path.join(d, 'in.bam'), [(CTG, case['seq'])], case['lines'])
    ref_fn = pc.write_fasta(os.path.join(d, 'ref.fa'), [(CTG, case['seq'])])
    vcf_fn = os.path.join(d, 'in.vcf')
    with open(vcf_fn, 'w') as f:
        f.write(case.get('vcf', ''))
    return bam_fn, ref_fn, vcf_fn


def pile(seq, start1, n, length=60, name='p', flag=0):
    """n reads of `length` matched bases at one start"""
    body = seq[start1 - 1:start1 - 1 + length]
    return [pc.sam_line(f'{name}{i}', flag, CTG, start1, 60, f'{length}M', body) for i in range(n)]


def deep_case(seed):
    """More than 8000 reads over eight starts, so that samtools' -d 8000 acts: reads of 30 and of 150 bases (the short ones of a start
    have ended two starts later), a third of them with another base at the site.  Stored by its seed: the golden keeps the lines."""
    rng = random.Random(seed)
    seq = pc.random_contig(rng, 2000)
    pos = 1000
    lines = []
    for k in range(8):
        start = pos - 145 + 18 * k
        for i in range(1400):
            n = 30 if i % 4 == 3 else 150
            body = seq[start - 1:start - 1 + n]
            if i % 3 == 0 and start <= pos < start + n:
                body = body[:pos - start] + other(seq[pos - 1]) + body[pos - start + 1:]
            lines.append(pc.sam_line(f'k{k}_{i}', 16 * (i & 1), CTG, start, 60, f'{n}M', body))
    return dict(name='deep', seed=seed, seq=seq, lines=lines, positions=[pos], vcf=vcf_text(seq, [(pos, seq[pos - 1], other(seq[pos - 1]))]))


@functools.lru_cache(maxsize=None)
def deep_golden():
    with open(DEEP_GOLDEN) as f:
        gold = json.load(f)
    return dict(deep_case(gold['seed']), expected_lines=gold['expected_lines'], expected_vcf=gold['expected_vcf'], expected_stdout=gold['expected_stdout'])
