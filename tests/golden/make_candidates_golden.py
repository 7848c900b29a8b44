"""Regenerates tests/golden/candidates/candidates_golden.json: (SAM lines, reference FASTA, options) -> the standard output of the
REFERENCE's own candidate extraction, Clair's preprocess/ExtractVariantCandidates.py, run as a module from its directory.

    python tests/golden/make_candidates_golden.py <reference tree>

Run where the reference tree is; it does not exist on the GPU box.  The fixture is data (inputs and the recorded output as text).

The script under test starts `samtools view -F 2316 <bam> [region]` and `samtools faidx <fasta> <region>`.  Here --samtools points at a
stand-in of a few lines that this script writes: `view` prints the lines of a SAM file that pass the flag (the region is not
applied: the drop-in does not apply one to records either, and the emission applies the range to positions), `faidx` prints the
region of a FASTA file.  Read bases stay within upper-case ACGTN and the IUPAC letters, where the script itself does not raise."""
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CLAIR = 'bin/Clair-ensemble/Clair.beta.ensemble.cpu'

STAND_IN = r'''#!/usr/bin/env python3
import sys
a = sys.argv[1:]
if a[0] == 'view':
    flag = int(a[a.index('-F') + 1])
    for line in open(a[3]):
        if line[0] != '@' and not int(line.split('\t')[1]) & flag:
            sys.stdout.write(line)
elif a[0] == 'faidx':
    region = a[2]
    name, lo, hi = region, None, None
    if ':' in region:
        name, span = region.rsplit(':', 1)
        lo, hi = (int(x) for x in span.split('-'))
    seqs, cur = {}, None
    for line in open(a[1]):
        if line[0] == '>':
            cur = line[1:].split()[0]
            seqs[cur] = []
        else:
            seqs[cur].append(line.strip())
    if name not in seqs:
        sys.exit(1)
    s = ''.join(seqs[name])
    s = s if lo is None else s[lo - 1:hi]
    print('>' + region)
    for i in range(0, len(s), 60):
        print(s[i:i + 60])
else:
    sys.exit(2)
'''

OTHER = {'A': 'C', 'C': 'G', 'G': 'T', 'T': 'A'}


def contig(seed, n):
    rng = random.Random(seed)
    return ''.join(rng.choice('ACGT') for _ in range(n))


def seq_for(ref, pos1, cigar, subs=None):
    """The bases of a read that follows ref along the CIGAR: soft clips are T, insertions G, an X base differs from the reference,
    bases past the end of the reference are A; subs: {0-based reference position: base} put in afterwards."""
    subs = subs or {}
    out, r, num = [], pos1 - 1, 0
    for ch in cigar:
        if ch.isdigit():
            num = num * 10 + int(ch)
            continue
        if ch in 'M=X':
            for _ in range(num):
                b = ref[r].upper() if r < len(ref) else 'A'
                b = b if b in 'ACGT' else 'A'
                if ch == 'X':
                    b = OTHER[b]
                out.append(subs.get(r, b))
                r += 1
        elif ch == 'I':
            out.append('G' * num)
        elif ch == 'S':
            out.append('T' * num)
        elif ch in 'DN':
            r += num
        num = 0
    return ''.join(out)


def sam(name, flag, ctg, pos1, mapq, cigar, seq):
    return '\t'.join([name, str(flag), ctg, str(pos1), str(mapq), cigar, '*', '0', '0', seq, '*'])


def read_sets():
    sets = {}

    # ---- basic: clips on both ends, = and X, indels inside, H and P, mismatches at several frequencies, ties, I second-largest
    c = contig(1, 300)
    rd = []
    for i in range(8):      # depth 8 over 21..120; position 40 (0-based): one of eight differs; 50: two of eight; 60: four of eight (a tie)
        subs = {}
        if i == 0:
            subs[40] = OTHER[c[40]]
        if i < 2:
            subs[50] = OTHER[c[50]]
        if i < 4:
            subs[60] = OTHER[c[60]]
        rd.append(sam(f'b{i}', 16 if i & 1 else 0, 'ctgA', 21, 60, '4S100M3S', seq_for(c, 21, '4S100M3S', subs)))
    for i in range(6):      # depth 6 over 131..190; position 150: two of six differ; five insertions behind position 160
        subs = {150: OTHER[c[150]]} if i < 2 else {}
        cg = '31M2I29M' if i < 5 else '60M'
        rd.append(sam(f'c{i}', 0, 'ctgA', 131, 60, cg, seq_for(c, 131, cg, subs)))
    for i in range(5):      # = and X, a deletion, hard clips and a padding
        cg = '5H10=1X9=3D10=2P10=5H'
        rd.append(sam(f'd{i}', 0, 'ctgA', 201, 30, cg, seq_for(c, 201, cg)))
    for i in range(4):      # ties: A, C, G, T one each at 259 (0-based); two and two at 265; four N at 270
        cg = '30M'
        rd.append(sam(f'e{i}', 0, 'ctgA', 251, 60, cg, seq_for(c, 251, cg, {259: 'ACGT'[i], 265: 'AACC'[i], 270: 'N'})))
    sets['basic'] = dict(contigs=[['ctgA', c]], reads=rd)

    # ---- the leading insertion, three forms, and a leading deletion
    c = contig(2, 200)
    # two of the five covering reads differ at 59 and 69 (0-based), so that the lines of those positions, and their I and D, show
    cover = [sam(f'v{i}', 0, 'ctgL', 41, 60, '40M', seq_for(c, 41, '40M', {59: OTHER[c[59]], 69: OTHER[c[69]]} if i < 2 else {})) for i in range(5)]
    lead = [sam(f'l{i}', 0, 'ctgL', 61, 60, '3S2I20M', seq_for(c, 61, '3S2I20M')) for i in range(3)]
    plain = sam('p0', 0, 'ctgL', 61, 60, '20M', seq_for(c, 61, '20M'))
    lowq = sam('q0', 0, 'ctgL', 61, 3, '2I20M', seq_for(c, 61, '2I20M'))
    ldel = [sam(f'k{i}', 0, 'ctgL', 71, 60, '2D20M', seq_for(c, 71, '2D20M')) for i in range(3)]
    sets['lead_first'] = dict(contigs=[['ctgL', c]], reads=cover + lead + ldel)
    sets['lead_later'] = dict(contigs=[['ctgL', c]], reads=cover + [plain] + lead)
    sets['lead_lowq'] = dict(contigs=[['ctgL', c]], reads=cover + [lowq] + lead)

    # ---- N does not advance the reference; a D behind it
    c = contig(3, 200)
    rd = [sam(f'n{i}', 0, 'ctgN', 11, 60, '60M', seq_for(c, 11, '60M')) for i in range(5)]
    rd += [sam(f'm{i}', 0, 'ctgN', 21, 60, '20M4N5M2D3M', seq_for(c, 21, '20M4N5M2D3M')) for i in range(3)]
    sets['n_then_d'] = dict(contigs=[['ctgN', c]], reads=rd)

    # ---- IUPAC letters in reads and reference, a lower-case reference base under a candidate, a reference N, an overhang
    c = list(contig(4, 120))
    for p, ch in zip(range(20, 36), 'ACGTURYSWKMBDHVN'):
        c[p] = ch
    c[50] = c[50].lower()
    c[60] = 'N'
    c = ''.join(c)
    rd = []
    for i in range(6):
        subs = {50: 'G' if i < 3 else 'C', 60: 'ACGTNN'[i], 70: 'RYSWKM'[i], 71: 'BDHVNN'[i], 72: 'MRWSYK'[i]}
        for p in range(20, 36):
            subs[p] = 'ACGTTRYSWKMBDHVN'[(p - 20 + i) % 16]
        rd.append(sam(f'i{i}', 0, 'ctgI', 11, 60, '100M', seq_for(c, 11, '100M', subs)))
    for i in range(5):      # ten bases past the end of the reference
        rd.append(sam(f'o{i}', 0, 'ctgI', 91, 60, '40M', seq_for(c, 91, '40M', {95: 'T'} if i < 2 else {})))
    sets['iupac'] = dict(contigs=[['ctgI', c]], reads=rd)

    # ---- flags, a second contig, and the 0.55 test with hard clips in T
    c1, c2 = contig(5, 150), contig(6, 150)
    rd = []
    for i in range(5):
        rd.append(sam(f'f{i}', 0, 'ctg1', 11, 60, '50M', seq_for(c1, 11, '50M', {30: OTHER[c1[30]]} if i < 2 else {})))
    for j, fl in enumerate((4, 8, 0x100, 0x800, 0x900 | 16)):      # all of these carry a mismatch at position 30 that must not count
        rd.append(sam(f'x{j}', fl, 'ctg1', 11, 60, '50M', seq_for(c1, 11, '50M', {30: OTHER[OTHER[c1[30]]], 31: OTHER[c1[31]]})))
    rd.append(sam('star', 0, 'ctg1', 12, 60, '*', 'ACGT'))
    for j, cg in enumerate(('9S11M', '10S11M', '5H9S11M', '12S11M5H', '12S11M', '9S10M', '20S24M')):
        rd.append(sam(f's{j}', 0, 'ctg1', 71, 60, cg, seq_for(c1, 71, cg, {75: OTHER[c1[75]]})))
    for i in range(5):
        rd.append(sam(f'g{i}', 0, 'ctg2', 11 + i, 60, '50M', seq_for(c2, 11 + i, '50M', {30: OTHER[c2[30]]} if i < 3 else {})))
    sets['two_contigs'] = dict(contigs=[['ctg1', c1], ['ctg2', c2]], reads=rd)
    return sets


BED = 'ctgA\t30\t45\nctgA\t50\t50\nctgA\t148\t152\nother\t0\t1000\nctgA\t140\t149\nctgA\t259\t270\n'

# (read set, options, BED text or None)
CASES = [
    ('basic', dict(threshold=0.125, minCoverage=4), None),
    ('basic', dict(threshold=0.2, minCoverage=4), None),
    ('basic', dict(threshold=1.0 / 3.0, minCoverage=4), None),
    ('basic', dict(threshold=0.126, minCoverage=4), None),
    ('basic', dict(threshold=0.125, minCoverage=2.5, minMQ=40), None),
    ('basic', dict(threshold=0.125, minCoverage=6.5), None),
    ('basic', dict(threshold=0.125, minCoverage=4, ctgStart=45, ctgEnd=161), None),
    ('basic', dict(threshold=0.125, minCoverage=4), BED),
    ('basic', dict(threshold=0.125, minCoverage=4, ctgStart=35, ctgEnd=151), BED),
    ('lead_first', dict(threshold=0.125, minCoverage=4), None),
    ('lead_first', dict(threshold=0.125, minCoverage=2.5), None),
    ('lead_later', dict(threshold=0.125, minCoverage=4), None),
    ('lead_lowq', dict(threshold=0.125, minCoverage=4, minMQ=10), None),
    ('lead_lowq', dict(threshold=0.125, minCoverage=4), None),
    ('n_then_d', dict(threshold=0.125, minCoverage=2.5), None),
    ('iupac', dict(threshold=0.125, minCoverage=4), None),
    ('iupac', dict(threshold=0.2, minCoverage=2.5, ctgStart=15, ctgEnd=125), None),
    ('two_contigs', dict(threshold=0.125, minCoverage=4, ctgName='ctg1'), None),
    ('two_contigs', dict(threshold=0.125, minCoverage=2.5, ctgName='ctg2'), None),
    ('two_contigs', dict(threshold=0.2, minCoverage=4, ctgName='ctg2', minMQ=61), None),      # no record is taken
]


def main():
    tree = sys.argv[1]
    clair = os.path.join(tree, CLAIR)
    sets = read_sets()
    cases = []
    for k, (set_name, opts, bed) in enumerate(CASES):
        rs = sets[set_name]
        opts = dict(opts)
        opts.setdefault('ctgName', rs['contigs'][0][0])
        with tempfile.TemporaryDirectory(prefix='cand') as d:
            tool = os.path.join(d, 'samtools')
            with open(tool, 'w') as f:
                f.write(STAND_IN)
            os.chmod(tool, 0o755)
            with open(os.path.join(d, 'in.sam'), 'w') as f:
                for nm, s in rs['contigs']:
                    f.write(f'@SQ\tSN:{nm}\tLN:{len(s)}\n')
                f.write(''.join(r + '\n' for r in rs['reads']))
            off = 0
            with open(os.path.join(d, 'ref.fa'), 'w') as f, open(os.path.join(d, 'ref.fa.fai'), 'w') as fai:
                for nm, s in rs['contigs']:
                    head = f'>{nm}\n'
                    f.write(head + s + '\n')
                    fai.write(f'{nm}\t{len(s)}\t{off + len(head)}\t{len(s)}\t{len(s) + 1}\n')
                    off += len(head) + len(s) + 1
            cmd = [sys.executable, '-m', 'preprocess.ExtractVariantCandidates', '--samtools', tool, '--bam_fn', os.path.join(d, 'in.sam'),
                   '--ref_fn', os.path.join(d, 'ref.fa'), '--can_fn', 'PIPE']
            if bed is not None:
                with open(os.path.join(d, 'in.bed'), 'w') as f:
                    f.write(bed)
                cmd += ['--bed_fn', os.path.join(d, 'in.bed')]
            for key, v in opts.items():
                cmd += ['--' + key, repr(v) if isinstance(v, float) else str(v)]
            env = dict(os.environ, PYTHONPATH=os.path.join(tree, 'bin/realignment'))
            p = subprocess.run(cmd, cwd=clair, env=env, capture_output=True, text=True, timeout=120)
            assert p.returncode == 0, (set_name, opts, p.stderr[-2000:])
        no_read = 'No read has been process' in p.stderr
        cases.append(dict(name=f'{k:02d}_{set_name}', contigs=rs['contigs'], reads=rs['reads'], options=opts, bed=bed, stdout=p.stdout,
                          no_read=no_read))
        print(cases[-1]['name'], opts, len(p.stdout.splitlines()), 'lines', 'no read taken' if no_read else '')
    os.makedirs(os.path.join(HERE, 'candidates'), exist_ok=True)
    json.dump(dict(generator='tests/golden/make_candidates_golden.py',
                   reference_module=CLAIR + '/preprocess/ExtractVariantCandidates.py (make_candidates, without --gen4Training)', cases=cases),
              open(os.path.join(HERE, 'candidates', 'candidates_golden.json'), 'w'), indent=1)
    print(len(cases), 'cases')


if __name__ == '__main__':
    main()
