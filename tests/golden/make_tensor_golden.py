"""Regenerates tests/golden/tensors/tensor_golden.json.gz: (SAM lines, reference FASTA, candidate positions, options, seed) -> the
standard output of the REFERENCE's own tensor creation, Clair's preprocess/CreateTensor.py, run as a module from its directory.

    python tests/golden/make_tensor_golden.py <reference tree>

Run where the reference tree is; it does not exist on the GPU box.  The fixture is data (inputs and the recorded output as text).

The script draws from Python's `random`, so it is started through a driver given to `python -c` that seeds `random`, sets sys.argv and
runs the module with runpy as __main__: the script's own `random` is the seeded one.  The fixture records the seed and the
interpreter's version (the order of a set of small integers and random.sample are CPython's).

The script starts `samtools view -F 2316 <bam> <region>` and `samtools faidx <fasta> <region>`.  Here --samtools points at a stand-in
that this script writes: `view` prints the lines of a SAM file that pass the flag, lie on the contig and, for a region, overlap it by
htslib's rule (the end counts M, D, N, = and X; a record of length 0 is one base), with their real qualities; `faidx` prints the
region of a FASTA file.

Reads are kept run-length coded, [n, SAM line]: n copies whose names get .0, .1, .. appended (n = 1: the line as it stands)."""
import gzip
import json
import os
import platform
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CLAIR = 'bin/Clair-ensemble/Clair.beta.ensemble.cpu'

STAND_IN = r'''#!/usr/bin/env python3
import re
import sys
a = sys.argv[1:]
if a[0] == 'view':
    flag = int(a[a.index('-F') + 1])
    region = a[4]
    name, lo, hi = region, None, None
    if ':' in region:
        name, span = region.rsplit(':', 1)
        lo, hi = (int(x) for x in span.split('-'))
    for line in open(a[3]):
        if line[0] == '@':
            continue
        f = line.split('\t')
        if int(f[1]) & flag or f[2] != name:
            continue
        if lo is not None:
            pos = int(f[3]) - 1
            n = sum(int(k) for k, op in re.findall(r'(\d+)([MIDNSHP=X])', f[5]) if op in 'MDN=X')
            if not (pos < hi and pos + (n or 1) > lo - 1):
                continue
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

DRIVER = ('import random, runpy, sys\n'
          'random.seed(int(sys.argv[1]))\n'
          'sys.argv = ["CreateTensor.py"] + sys.argv[2:]\n'
          'runpy.run_module("preprocess.CreateTensor", run_name="__main__")\n')

OTHER = {'A': 'C', 'C': 'G', 'G': 'T', 'T': 'A'}
CTG = 'ctgT'


def contig(seed, n):
    rng = random.Random(seed)
    return ''.join(rng.choice('ACGT') for _ in range(n))


def seq_for(ref, pos1, cigar, subs=None):
    """The bases of a read that follows ref along the CIGAR: soft clips are T, insertions cycle through ACGT, an X base differs from
    the reference, a reference byte that is not ACGT reads as A; subs: {0-based reference position: base} put in afterwards."""
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
            out.append(''.join('ACGT'[k & 3] for k in range(num)))
        elif ch == 'S':
            out.append('T' * num)
        elif ch == 'D':
            r += num
        num = 0
    return ''.join(out)


def rd(ref, name, pos1, cigar, flag=0, mapq=60, subs=None, qual=None, low=None):
    """A SAM line; qual: a character for every base (default I = 40); low: {0-based reference position: quality character} -- put on
    the base under an M, = or X there."""
    seq = seq_for(ref, pos1, cigar, subs)
    q = list((qual or 'I') * len(seq))
    if low:
        r, i, num = pos1 - 1, 0, 0
        for ch in cigar:
            if ch.isdigit():
                num = num * 10 + int(ch)
                continue
            if ch in 'M=X':
                for _ in range(num):
                    if r in low:
                        q[i] = low[r]
                    r += 1
                    i += 1
            elif ch in 'IS':
                i += num
            elif ch == 'D':
                r += num
            num = 0
    return '\t'.join([name, str(flag), CTG, str(pos1), str(mapq), cigar, '*', '0', '0', seq, ''.join(q)])


def expand(reads):
    out = []
    for n, line in reads:
        if n == 1:
            out.append(line)
        else:
            name, rest = line.split('\t', 1)
            out += [f'{name}.{k}\t{rest}' for k in range(n)]
    return out


def cases():
    out = []

    def case(name, ref, reads, positions, seed=1, search=None, **opts):
        reads = sorted(([1, r] if isinstance(r, str) else r for r in reads), key=lambda r: int(r[1].split('\t')[3]))     # (stable) by POS
        out.append(dict(name=name, contigs=[[CTG, ref]], reads=reads, positions=positions,
                        options=opts, seed=seed, search=search))

    # ---- every operation type around a window, both strands
    c = contig(11, 300)
    ops = [rd(c, 'a0', 61, '5S20M2I10M3D15M4N10M2H'), rd(c, 'a1', 71, '3H10=1X9=2P5=3D20=', flag=16), rd(c, 'a2', 81, '40M', subs={99: 'T', 104: 'N'}),
           rd(c, 'a3', 85, '10M1I10M1D30M', flag=16), rd(c, 'a4', 100, '2S30M', flag=16, qual='5'), rd(c, 'a5', 117, '30M'), rd(c, 'a6', 131, '20M')]
    case('ops', c, ops, [100, 130])
    case('ops_no_left_edge', c, ops, [100, 130], stop_consider_left_edge=True)
    # ---- windows at the left end of the contig, and at the right end short of the sequence
    c = contig(12, 120)
    ends = [rd(c, 'e0', 1, '50M'), rd(c, 'e1', 2, '50M', flag=16), rd(c, 'e2', 3, '45M'), rd(c, 'e3', 71, '50M'), rd(c, 'e4', 81, '40M', flag=16)]
    case('ends', c, ends, [5, 17, 18, 30, 100, 104, 110])
    # ---- IUPAC and lower-case reference bytes, IUPAC read bases
    c = list(contig(13, 200))
    for p, ch in zip(range(60, 76), 'ACGTURYSWKMBDHVN'):
        c[p] = ch
    c[80], c[82] = c[80].lower(), 'n'
    c = ''.join(c)
    iu = []
    for i in range(4):
        subs = {p: 'ACGTRYSWKMBDHVNA'[(p - 60 + 3 * i) % 16] for p in range(60, 76)}
        subs.update({84: 'RYKM'[i], 85: 'N'})
        iu.append(rd(c, f'i{i}', 41, '80M2D10M', flag=16 if i & 1 else 0, subs=subs))
    case('iupac', c, iu, [70, 85, 110])
    # ---- insertions: leading, at index 0, long (clamps at 32), and behind the last base
    c = contig(14, 300)
    ins = [rd(c, 'n0', 61, '100M'), rd(c, 'n1', 90, '3I30M'), rd(c, 'n2', 100, '2S4I30M', flag=16), rd(c, 'n3', 61, '23M2I60M'),
           rd(c, 'n4', 61, '30M45I40M', flag=16), rd(c, 'n5', 61, '45M6I'), rd(c, 'n6', 84, '1M2I40M')]
    case('insertions', c, ins, [100, 120])
    # ---- a deletion over the centre, a leading deletion, a deletion over the window's first position, a read that joins at c0 + 17 only
    dels = [rd(c, 'd0', 61, '100M'), rd(c, 'd1', 61, '35M8D40M', flag=16), rd(c, 'd2', 100, '3D30M'), rd(c, 'd3', 61, '20M6D50M'),
            rd(c, 'd4', 117, '20M'), rd(c, 'd5', 95, '2M40D10M'), rd(c, 'd6', 84, '4D30M', flag=16)]
    case('deletions', c, dels, [100])
    # ---- a region: a read that ends just before it but inside a window; minMQ
    reg = [rd(c, 'r0', 41, '58M'), rd(c, 'r1', 41, '60M'), rd(c, 'r2', 61, '80M', flag=16), rd(c, 'r7', 90, '5M60N5M', flag=16),
           rd(c, 'r3', 95, '50M', mapq=5), rd(c, 'r4', 96, '50M', mapq=10), rd(c, 'r5', 139, '30M'), rd(c, 'r6', 141, '30M')]
    case('region', c, reg, [90, 105, 130, 150], ctgStart=100, ctgEnd=140)
    case('no_region', c, reg, [90, 105, 130, 150])
    case('min_mq_0', c, reg, [105, 130], minMQ=0)
    case('min_mq_11', c, reg, [105, 130], minMQ=11)
    # ---- dcov 3 with five reads on one POS, and the quirk of POS 0
    c = contig(15, 200)
    dc = [[5, rd(c, 'q', 1, '60M')], [5, rd(c, 'p', 31, '60M', flag=16)], '\t'.join(['star', '0', CTG, '31', '60', '*', '*', '0', '0', 'ACGT', 'IIII']), [2, rd(c, 's', 41, '60M')]]
    case('dcov3', c, dc, [20, 50, 80], dcov=3)
    case('dcov1', c, dc, [20, 50, 80], dcov=1)
    # ---- minCoverage: a shallow centre, and a deep one cut at its first and at its second iteration
    c = contig(16, 300)
    cov = [[95, rd(c, 'x', 81, '60M')], [55, rd(c, 'y', 81, '15M', flag=16)], [3, rd(c, 'z', 181, '40M')]]
    case('min_coverage_first', c, cov, [100, 200], minCoverage=70)
    case('min_coverage_second', c, cov, [100, 200], minCoverage=63, search=1)
    case('min_coverage_none', c, cov, [100, 200], minCoverage=3)
    # ---- deep centres
    c = contig(17, 300)
    case('deep_101_100', c, [[60, rd(c, 'h', 81, '60M')], rd(c, 'l', 81, '60M', low={99: '#'}), [40, rd(c, 'g', 85, '60M', flag=16)]], [100], seed=3)
    case('deep_101_101', c, [[60, rd(c, 'h', 81, '60M')], rd(c, 'l', 81, '60M', low={99: '('}), [40, rd(c, 'g', 85, '60M', flag=16)]], [100], seed=4)
    case('deep_250', c, [[100, rd(c, 'h', 71, '60M', subs={99: 'A'})], [30, rd(c, 'k', 75, '20M3D30M')], [120, rd(c, 'g', 90, '60M', flag=16, subs={99: 'C'})]],
         [100], seed=5)
    rng = random.Random(18)
    high = set(rng.sample(range(1000), 120))
    runs, k = [], 0
    while k < 1000:
        j = k
        while j < 1000 and (j in high) == (k in high):
            j += 1
        runs.append([j - k, rd(c, f'u{k}', 81, '60M', flag=16 if len(runs) & 2 else 0, low=None if k in high else {99: '%'})])
        k = j
    case('deep_1000_scattered', c, runs, [100], seed=6)
    case('deep_cap', c, [[913 + (1 if s < 7 else 0), rd(c, f'w{s}', 80 + s, '35M', flag=16 if s & 1 else 0, subs={99: 'ACGT'[s & 3]})] for s in range(11)], [100],
         seed=7)
    assert sum(r[0] for r in out[-1]['reads']) == 10050
    return out


def run(tree, case, seed):
    clair = os.path.join(tree, CLAIR)
    ref = case['contigs'][0][1]
    with tempfile.TemporaryDirectory(prefix='tens') as d:
        tool = os.path.join(d, 'samtools')
        with open(tool, 'w') as f:
            f.write(STAND_IN)
        os.chmod(tool, 0o755)
        with open(os.path.join(d, 'in.sam'), 'w') as f:
            f.write(f'@SQ\tSN:{CTG}\tLN:{len(ref)}\n')
            f.write(''.join(r + '\n' for r in expand(case['reads'])))
        with open(os.path.join(d, 'ref.fa'), 'w') as f:
            f.write(f'>{CTG}\n{ref}\n')
        cmd = [sys.executable, '-c', DRIVER, str(seed), '--samtools', tool, '--bam_fn', os.path.join(d, 'in.sam'), '--ref_fn', os.path.join(d, 'ref.fa'),
               '--can_fn', 'PIPE', '--tensor_fn', 'PIPE', '--ctgName', CTG]
        for key, v in case['options'].items():
            cmd += ['--' + key] if v is True else ['--' + key, str(v)]
        env = dict(os.environ, PYTHONPATH=os.path.join(tree, 'bin/realignment'))
        stdin = ''.join(f'{CTG} {p} N 0\n' for p in case['positions'])
        p = subprocess.run(cmd, cwd=clair, env=env, input=stdin, capture_output=True, text=True, timeout=1200)
        assert p.returncode == 0, (case['name'], p.stderr[-2000:])
    return p.stdout


def main():
    tree = sys.argv[1]
    done = []
    for case in cases():
        search = case.pop('search')
        seed = case['seed']
        stdout = run(tree, case, seed)
        if search is not None:      # the first seed with which the first centre writes exactly `search` lines
            first = f'{CTG} {case["positions"][0]} '
            while sum(l.startswith(first) for l in stdout.splitlines()) != search:
                seed += 1
                assert seed < 200
                stdout = run(tree, case, seed)
            case['seed'] = seed
        case['stdout'] = stdout
        done.append(case)
        print(case['name'], case['options'], 'seed', case['seed'], len(stdout.splitlines()), 'lines', len(stdout), 'bytes')
    os.makedirs(os.path.join(HERE, 'tensors'), exist_ok=True)
    doc = dict(generator='tests/golden/make_tensor_golden.py', reference_module=CLAIR + '/preprocess/CreateTensor.py (OutputAlnTensor)',
               python=platform.python_version(), implementation=platform.python_implementation(), cases=done)
    # the recorded lines are 1056 numbers each, 100 of them for the deepest case: kept gzip-compressed (no name, no time: the same bytes
    # from the same cases); `zcat tests/golden/tensors/tensor_golden.json.gz | python -m json.tool` shows it
    with open(os.path.join(HERE, 'tensors', 'tensor_golden.json.gz'), 'wb') as f, gzip.GzipFile(fileobj=f, mode='wb', filename='', mtime=0) as z:
        z.write(json.dumps(doc, indent=0, separators=(',', ':')).encode())
    print(len(done), 'cases')


if __name__ == '__main__':
    main()
