"""Writes tests/golden/clair_ensemble/clair_ensemble_golden.json.gz: what the reference's own, unmodified
clair/post_processing/ensemble.py and clair/post_processing/overlap_variant.py print for constructed input (runpy, standard input and
output redirected).  Data only: the input text, the option and the output text of every case.

    python tests/golden/make_clair_ensemble_golden.py <reference tree>

Both scripts are pure Python without dependencies; the Python version is recorded."""
import contextlib
import gzip
import io
import json
import os
import random
import runpy
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CELLS, PROBS = 1056, 90


def run(script, argv, text):
    old = sys.stdin, sys.argv
    out = io.StringIO()
    try:
        sys.stdin, sys.argv = io.StringIO(text), [script] + argv
        with contextlib.redirect_stdout(out):
            runpy.run_path(script, run_name='__main__')
    finally:
        sys.stdin, sys.argv = old
    return out.getvalue()


# ---- ensemble.py ----------------------------------------------------------------------------------------------------------------------
def cells_of(rng, negative=False):
    """mostly zeros, as a tensor's rows beyond the depth are; a few cells below zero, as the difference channels have them"""
    x = [0] * CELLS
    for _ in range(60):
        x[rng.randrange(CELLS)] = rng.randint(-100 if negative else 0, 100)
    return x


def micro(v):
    return '%d.%06d' % (v // 1000000, v % 1000000)


def probs_of(rng):
    return [micro(rng.choice([0, 1, 999999, 1000000, rng.randrange(1000001), rng.randrange(2000)])) for _ in range(PROBS)]


def line(chrom, pos, seq, cells, probs):
    return '\t'.join([chrom, str(pos), seq] + [str(v) for v in cells] + list(probs)) + '\n'


def random_line(rng, chrom, pos, negative=False):
    return line(chrom, pos, ''.join(rng.choice('ACGT') for _ in range(33)), cells_of(rng, negative), probs_of(rng))


def ensemble_cases():
    rng = random.Random(2025)
    cases = []
    # one line per key; '10' before '9' (first appearance, not numeric or string order); '09' is another key than '9'; negative cells
    text = ''.join(random_line(rng, c, p, True) for c, p in (('ctgA', '10'), ('ctgA', '9'), ('ctgB', '9'), ('ctgA', '09'), ('ctgA', '100000')))
    cases.append(('one_line_per_key', 0, text))
    # 2, 3, 4, 7, 100 and 400 lines of one key each, a deep site's resamples
    text = ''.join(random_line(rng, 'ctgA', str(1000 + n), n == 3) for n in (2, 3, 4, 7, 100, 400) for _ in range(n))
    cases.append(('counts', 0, text))
    # three concatenated files with the keys interleaved; k4 has one line, k3 two, k1 and k2 three
    files = [['k1', 'k2', 'k3'], ['k2', 'k1', 'k4'], ['k3', 'k1', 'k2']]
    text = ''.join(random_line(rng, 'ctgA', {'k1': 51, 'k2': 40, 'k3': 77, 'k4': 12}[k], True) for f in files for k in f)
    for m in (0, 1, 2, 3, 4):
        cases.append(('interleaved_min%d' % m, m, text))
    # pairs whose sum is an odd number of micro-units, at counts 2 and 4: the mean lies one float64 rounding from a tie, or on it
    def odd_group(n):
        rows = [[rng.randrange(1000001) for _ in range(PROBS)] for _ in range(n)]
        for col in range(PROBS):
            total = sum(r[col] for r in rows)
            if n == 2 and total % 2 == 0 or n == 4 and total % 4 != 2:
                rows[0][col] += (2 - total % n) % n if n == 4 else 1
        return rows
    text = ''
    for i in range(40):
        n = 2 if i % 2 == 0 else 4
        cells = [cells_of(rng) for _ in range(n)]
        text += ''.join(line('ctgA', 5000 + i, 'A' * 33, c, [micro(v) for v in r]) for c, r in zip(cells, odd_group(n)))
    cases.append(('odd_sums', 2, text))
    # multiples of 1/128: exact ties of `{:.6f}`, alone, as means of 2 and 4 equal lines, and as a mean of two different lines
    ties = ['%.7f' % (j / 128) for j in range(1, 128, 2)] + ['0.0078125'] * (PROBS - 64)
    text = line('ctgA', 1, 'C' * 33, cells_of(rng), ties)
    text += ''.join(line('ctgA', 2, 'C' * 33, cells_of(rng), ties) for _ in range(2))
    text += ''.join(line('ctgA', 3, 'C' * 33, cells_of(rng), ties) for _ in range(4))
    lo = ['%.7f' % (j / 128 - 0.0000005) for j in range(1, 128, 2)] + ['0.007812'] * (PROBS - 64)
    hi = ['%.7f' % (j / 128 + 0.0000005) for j in range(1, 128, 2)] + ['0.007813'] * (PROBS - 64)
    text += line('ctgA', 4, 'C' * 33, cells_of(rng), lo) + line('ctgA', 4, 'C' * 33, cells_of(rng), hi)
    cases.append(('ties', 0, text))
    # counts 3 and 7 with a count of 3 asked for
    text = ''.join(random_line(rng, 'ctgA', 7000 + k, True) for n, k in ((3, 0), (7, 1), (2, 2), (3, 3), (7, 4)) for _ in range(n))
    cases.append(('thirds_and_sevenths', 3, text))
    # what the text tool may be given beyond probabilities: values of 8 and more (no float32 prints back to their text), values below
    # zero, a negative zero, exponents
    wide = ['12.3456785', '-0.0000004', '-0.0', '1e-7', '123456.7890125', '-2.5e-6', '8.0000005', '0.5e-6', '1.5e-6', '2.5e-6'] * 9
    text = line('ctgW', 1, 'G' * 33, cells_of(rng, True), wide)
    text += ''.join(line('ctgW', 2, 'G' * 33, cells_of(rng, True), wide) for _ in range(3))
    cases.append(('wide_values', 0, text))
    return cases


# ---- overlap_variant.py ---------------------------------------------------------------------------------------------------------------
HEADER = '##fileformat=VCFv4.1\n##FILTER=<ID=PASS,Description="All filters passed">\n##contig=<ID=chr1,length=100000>\n' \
         '#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tAmplicon\n'


def row(chrom, pos, ref, alt, qual, gt='0/1', dp=60, af='0.5000', filt='PASS', info='.'):
    q = str(qual)
    return '\t'.join([chrom, str(pos), '.', ref, alt, q, filt, info, 'GT:GQ:DP:AF', '%s:%s:%d:%s' % (gt, q, dp, af)]) + '\n'


def overlap_cases():
    cases = []
    # a deletion over a SNP: the SNP has the higher, the lower and the same QUAL
    rows = []
    for base, (qd, qs) in zip((100, 200, 300), ((50, 60), (60, 50), (55, 55))):
        rows += [row('chr1', base, 'ACGT', 'A', qd, '1/1'), row('chr1', base + 2, 'G', 'T', qs)]
    cases.append(('deletion_over_snp', HEADER + ''.join(rows)))
    # chains: a replacement changes what the next row is compared with
    rows = [row('chr1', 100, 'ACGTAC', 'A', 50), row('chr1', 102, 'G', 'T', 60), row('chr1', 104, 'A', 'C', 10),          # the SNP replaces; 104 is then free
            row('chr1', 200, 'ACGTAC', 'A', 70), row('chr1', 202, 'G', 'T', 60), row('chr1', 204, 'A', 'C', 10),          # the deletion stays; 204 falls too
            row('chr1', 300, 'ACGTAC', 'A', 20), row('chr1', 302, 'GTAC', 'G', 30), row('chr1', 305, 'C', 'G', 40),       # deletion, deletion, SNP: each replaces
            row('chr1', 400, 'ACG', 'A', 20), row('chr1', 400, 'ACGT', 'A', 20), row('chr1', 400, 'A', 'T', 19)]           # one position three times
    cases.append(('chains', HEADER + ''.join(rows)))
    # two ALTs, with and without a change of length; the 1024 that stands for a second ALT that is not there
    long_ref, long_alt = 'A' * 1028, 'A' * 1030
    rows = [row('chr1', 100, 'AT', 'A,ATT', 30, '1/2'), row('chr1', 101, 'T', 'C', 29),
            row('chr1', 200, 'A', 'C,G', 30, '1/2'), row('chr1', 200, 'A', 'T', 31),
            row('chr1', 300, 'ACG', 'ACGT,A', 30, '1/2'), row('chr1', 302, 'G', 'C,T', 30, '1/2'), row('chr1', 303, 'T', 'TA,TAA', 99, '1/2'),
            row('chr1', 400, 'AC', 'ACC,ACCC', 30, '1/2'), row('chr1', 401, 'C', 'T', 5),
            row('chr1', 500, long_ref, long_alt, 30), row('chr1', 503, 'A', 'T', 31), row('chr1', 504, 'A', 'T', 1), row('chr1', 505, 'A', 'G', 1)]
    cases.append(('two_alts', HEADER + ''.join(rows)))
    # insertions never overlap anything; rows just inside and just outside a deletion's interval
    rows = [row('chr1', 100, 'A', 'ATTT', 30), row('chr1', 100, 'A', 'C', 10), row('chr1', 101, 'C', 'CA', 10), row('chr1', 101, 'C', 'CAA', 90),
            row('chr1', 199, 'T', 'G', 5), row('chr1', 200, 'ACG', 'A', 50, '1/1'), row('chr1', 203, 'T', 'C', 5),
            row('chr1', 300, 'ACG', 'A', 50, '1/1'), row('chr1', 302, 'G', 'C', 5), row('chr1', 303, 'T', 'C', 5),
            row('chr1', 400, 'ACG', 'A', 50, '1/1'), row('chr1', 402, 'G', 'GT', 95)]
    cases.append(('insertions_and_edges', HEADER + ''.join(rows)))
    # two chromosomes; a fractional QUAL; FILTER, INFO and ID that are rewritten; rows out of order (the script swaps the pair)
    rows = [row('chr1', 100, 'ACGT', 'A', 50), row('chr2', 101, 'C', 'T', 60), row('chr2', 102, 'CTT', 'C', '12.97', filt='LowQual', info='SVTYPE=DEL'),
            row('chr2', 103, 'T', 'A', 12), row('chr2', 200, 'GA', 'G', '7.5'), row('chr2', 201, 'A', 'T', '7.9'),
            row('chr2', 301, 'A', 'T', 80), row('chr2', 300, 'GAC', 'G', 81), row('chr2', 299, 'TG', 'T', 81)]
    cases.append(('chromosomes_and_quals', HEADER + ''.join(rows)))
    cases.append(('header_only', HEADER))
    cases.append(('no_header', ''.join([row('chrM', 5, 'ACG', 'A', 3), row('chrM', 6, 'C', 'T', 3)])))
    return cases


def main():
    post = os.path.join(sys.argv[1], 'bin', 'Clair-ensemble', 'Clair.beta.ensemble.cpu', 'clair', 'post_processing')
    ens, ovl = os.path.join(post, 'ensemble.py'), os.path.join(post, 'overlap_variant.py')
    assert os.path.isfile(ens) and os.path.isfile(ovl), post
    ensemble = [dict(name=n, minimum_count=m, input=t, output=run(ens, ['--minimum_count_to_output', str(m)], t)) for n, m, t in ensemble_cases()]
    overlap = [dict(name=n, input=t, output=run(ovl, [], t)) for n, t in overlap_cases()]
    by = {c['name']: c for c in ensemble}
    assert by['interleaved_min3']['output'].count('\n') == 2 and by['interleaved_min0']['output'].count('\n') == 4 and by['interleaved_min4']['output'] == ''
    assert [l.split('\t')[1] for l in by['one_line_per_key']['output'].splitlines()] == ['10', '9', '9', '09', '100000']
    assert by['counts']['output'].count('\n') == 6 and '-' in by['wide_values']['output']
    for c in overlap:
        assert c['output'].count('\n') <= c['input'].count('\n')
    assert any(c['output'].count('\n') < c['input'].count('\n') for c in overlap)
    out = os.path.join(HERE, 'clair_ensemble', 'clair_ensemble_golden.json.gz')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, 'wb') as f, gzip.GzipFile(fileobj=f, mode='wb', filename='', mtime=0) as z:
        z.write(json.dumps(dict(python=sys.version.split()[0], ensemble=ensemble, overlap=overlap)).encode())
    print(out, os.path.getsize(out), 'bytes;', len(ensemble), 'ensemble cases,', len(overlap), 'overlap cases')


if __name__ == '__main__':
    main()
