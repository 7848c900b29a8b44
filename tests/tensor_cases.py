"""Inputs of the tensor tests (test infrastructure): the golden cases of tests/golden/tensors as BAM and FASTA files, and constructed
reads with qualities."""
import functools
import gzip
import json
import os

import pileup_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'tensors', 'tensor_golden.json.gz')


@functools.lru_cache(maxsize=None)
def golden():
    with gzip.open(GOLDEN, 'rt') as f:
        return json.load(f)


def golden_cases():
    return golden()['cases']


def case_named(name):
    return next(c for c in golden_cases() if c['name'] == name)


def expand(reads):
    """[n, SAM line] -> n lines whose names get .0, .1, .. appended (n = 1: the line as it stands)"""
    out = []
    for n, line in reads:
        if n == 1:
            out.append(line)
        else:
            name, rest = line.split('\t', 1)
            out += [f'{name}.{k}\t{rest}' for k in range(n)]
    return out


def sam_line(name, flag, ctg, pos1, mapq, cigar, seq, qual=None, tags=()):
    return '\t'.join([name, str(flag), ctg, str(pos1), str(mapq), cigar, '*', '0', '0', seq, qual if qual is not None else 'I' * len(seq)] + list(tags))


def write_case(tmp_path, case):
    """-> (bam path, fasta path) of a golden case"""
    d = os.path.join(str(tmp_path), case['name'])
    os.makedirs(d, exist_ok=True)
    bam_fn = pc.write_bam(os.path.join(d, 'in.bam'), [tuple(c) for c in case['contigs']], expand(case['reads']))
    return bam_fn, pc.write_fasta(os.path.join(d, 'ref.fa'), case['contigs'])


def candidate_text(case):
    ctg = case['contigs'][0][0]
    return ''.join(f'{ctg} {p} N 0\n' for p in case['positions'])


def keywords(case):
    """the options of a golden case as keyword arguments of clair_tensor.tensors / tensor_ref.tensors (without the random source)"""
    o = case['options']
    return dict(ctg_start=o.get('ctgStart'), ctg_end=o.get('ctgEnd'), min_mq=o.get('minMQ', 10), dcov=o.get('dcov', 1000),
                min_coverage=o.get('minCoverage', 0))


def argv(case):
    out = []
    for key, v in case['options'].items():
        out += ['--' + key] if v is True else ['--' + key, str(v)]
    return out
