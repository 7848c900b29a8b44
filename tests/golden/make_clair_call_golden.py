"""Writes tests/golden/clair_call/clair_call_golden.json.gz: what the reference's own, unmodified clair/call_var.py, run as a module
with --input_probabilities, prints for constructed cases.  Data only: SAM lines, FASTA, input lines, options and the VCF text.

    python tests/golden/make_clair_call_golden.py <reference tree>

The script runs in a child whose sys.modules holds stand-ins before the import: `clair.model` (an empty Clair; it would pull in
TensorFlow), `blosc` and `intervaltree` (absent here and unused on this path), and `pysam`.  The pysam stand-in is the literal,
sequential restatement of htslib's pile-up machine of tests/clair_call_ref.py (head and tail list, cnt, max_pos, the drop rule of
bam_plp_push, bam_plp64_next, resolve_cigar2, the spelling of pileup_seq) over SAM lines chosen by htslib's overlap rule in file
order -- deliberately not the closed form the product uses; FastaFile.fetch clips at the contig end.  What it does not model:
overlap detection of read pairs, BAQ, pysam's own version differences (its get_query_sequences is taken to spell what samtools'
pileup_seq spells).

The probabilities of the lines are capped at 0.999999: under NumPy 2 the script cannot print a row with p == 1.0.  The NumPy and
Python versions are recorded: under NumPy 2 the quality and the allele frequency are float32 (tests/clair_call_ref.py 'nep50')."""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))

DRIVER = r'''
import json, os, runpy, sys, types
sys.path.insert(0, os.environ['MPN_TESTS'])
sys.path.insert(0, os.environ['MPN_CLAIR'])
import clair_call_ref as ref

model = types.ModuleType('clair.model')
model.Clair = type('Clair', (), {})
blosc = types.ModuleType('blosc')
blosc.set_nthreads = lambda n: None
tree = types.ModuleType('intervaltree')
tree.IntervalTree = type('IntervalTree', (), {})


class Column:
    def __init__(self, at, members):
        self.reference_pos, self.members = at, members

    def get_query_sequences(self, mark_matches=False, mark_ends=False, add_indels=False):
        assert add_indels and not mark_matches and not mark_ends
        return [ref.spell(read, k, x, y, self.reference_pos) for read, k, x, y in self.members]


class AlignmentFile:
    def __init__(self, path, mode='rb'):
        with open(path) as f:
            self.reads = [ref.read_of(line) for line in json.load(f)]

    def pileup(self, contig, start, stop, flag_filter, min_base_quality, max_depth):
        assert stop == start + 1 and flag_filter == ref.FILTER_FLAG and max_depth == ref.MAX_DEPTH
        machine = ref.Pileup(ref.overlapping(self.reads, start), max_depth)
        while True:
            got = machine.auto()
            if got is None:
                return
            yield Column(*got)

    def close(self):
        pass


class FastaFile:
    def __init__(self, filename):
        self.seq, name = {}, None
        for line in open(filename):
            if line.startswith('>'):
                name = line[1:].split()[0]
                self.seq[name] = ''
            else:
                self.seq[name] += line.strip()

    def fetch(self, reference, start, end):
        return self.seq[reference][max(start, 0):max(end, 0)]

    def close(self):
        pass


pysam = types.ModuleType('pysam')
pysam.AlignmentFile, pysam.FastaFile = AlignmentFile, FastaFile
sys.modules.update({'clair.model': model, 'blosc': blosc, 'intervaltree': tree, 'pysam': pysam})
sys.argv = ['call_var'] + sys.argv[1:]
runpy.run_module('clair.call_var', run_name='__main__')
'''


def input_lines(case, ctg):
    return ''.join('\t'.join([ctg, str(s), r] + [str(v) for v in x.reshape(-1).tolist()] + ['%.6f' % v for v in p.tolist()]) + '\n'
                   for s, r, x, p in zip(case['sites'], case['refs'], case['x'], case['probs']))


def deep_case(cc):
    """600 reads in three start groups over the sites: the machine and the closed form take other reads than all that overlap"""
    import random
    rng = random.Random(77)
    lines = []
    for start, n in ((70, 230), (75, 200), (82, 170)):
        for i in range(n):
            body = [('M', 100 - start), ('I', 2), ('M', 40)] if i % 3 else [('M', 100 - start), ('D', 3), ('M', 40)]
            lines.append(cc.line_of(rng, f's{start}.{i}', 16 if i % 2 else 0, start, body))
    base = cc.decode_case(15, n_sites=12, reads=10)
    sites = [100, 101, 140]
    probs = np.zeros((3, 90), dtype=np.float32)
    probs[:, 15] = probs[:, 22] = probs[:, 24 + 18] = probs[:, 57 + 18] = 1
    return dict(base, lines=lines, sites=sites, x=base['x'][:3], probs=probs, refs=[cc.window(base['seq'], s) for s in sites])


def main():
    clair = os.path.join(sys.argv[1], 'bin', 'Clair-ensemble', 'Clair.beta.ensemble.cpu')
    assert os.path.isfile(os.path.join(clair, 'clair', 'call_var.py')), clair
    import clair_call_cases as cc
    import clair_call_ref as ref
    plan = [('all_bases', cc.cached_case(11), ['--pysam_for_all_indel_bases', '--showRef', '--qual', '100']),
            ('tensor_bases', cc.cached_case(12), []),
            ('haploid', cc.cached_case(13, long_events=True), ['--pysam_for_all_indel_bases', '--haploid', '--showRef', '--qual', '300']),
            ('tensor_bases_long', cc.cached_case(14, long_events=True), ['--showRef']),
            ('reset', cc.reset_case(), ['--pysam_for_all_indel_bases', '--showRef']),
            ('insdel', (lambda c: dict(c, sites=c['sites'][:1], x=c['x'][:1], probs=c['probs'][:1], refs=c['refs'][:1]))(cc.insdel_case()),
             ['--pysam_for_all_indel_bases']),
            ('deep', deep_case(cc), ['--pysam_for_all_indel_bases', '--showRef'])]
    cases, classes, trace = [], set(), set()
    with tempfile.TemporaryDirectory() as d:
        driver = os.path.join(d, 'driver.py')
        with open(driver, 'w') as f:
            f.write(DRIVER)
        for name, case, options in plan:
            case = dict(case, probs=np.minimum(np.asarray(case['probs'], dtype=np.float32), np.float32(0.999999)))
            sam_fn, fa_fn, out_fn = (os.path.join(d, name + e) for e in ('.sam.json', '.fa', '.vcf'))
            with open(sam_fn, 'w') as f:
                json.dump(case['lines'], f)
            with open(fa_fn, 'w') as f:
                f.write('>%s\n%s\n' % (cc.CTG, case['seq']))
            with open(fa_fn + '.fai', 'w') as f:
                f.write('%s\t%d\t%d\t%d\t%d\n' % (cc.CTG, len(case['seq']), len(cc.CTG) + 2, len(case['seq']), len(case['seq']) + 1))
            text = input_lines(case, cc.CTG)
            env = dict(os.environ, MPN_TESTS=TESTS, MPN_CLAIR=clair)
            p = subprocess.run([sys.executable, driver, '--input_probabilities', '--bam_fn', sam_fn, '--ref_fn', fa_fn, '--call_fn', out_fn] + options,
                               input=text.encode(), capture_output=True, env=env, cwd=d, timeout=3600)
            assert p.returncode == 0, p.stderr.decode()[-3000:]
            vcf = open(out_fn).read()
            # ---- what the fixture must hold: checked on the restatement's trace of the same lines
            kw = dict(pysam_all='--pysam_for_all_indel_bases' in options, haploid='--haploid' in options, show_ref='--showRef' in options)
            quantized = dict(case, probs=ref.quantize(case['probs']))
            for got in cc.expected_rows(quantized, trace=trace, **kw):
                if got is not None:
                    classes.add(got[1]['flags'].index(True))
                    assert float(got[1]['p']) != 1.0
            cases.append(dict(name=name, contig=cc.CTG, seq=case['seq'], lines=case['lines'], options=options, input=text, vcf=vcf))
        deep = cases[-1]
        reads = [ref.read_of(l) for l in deep['lines']]
        taken = ref.closed_members(reads, 100)
        everyone = [r for r in ref.overlapping(reads, 100) if r[1] <= 99 < r[1] + ref.rlen(r[2])]
        assert len(ref.overlapping(reads, 100)) > 250 and len(taken) < len(everyone) and len({r[1] for r in taken}) == 3
        assert ref.literal_sequences(reads, 100) == ref.closed_sequences(reads, 100)
    assert classes == set(range(10)), classes
    assert trace == {'nothing', 'ins_ins reset', 'del_del reset'}, trace
    used = {o for c in cases for o in c['options']}
    assert {'--pysam_for_all_indel_bases', '--haploid', '--showRef', '--qual'} <= used and any('--pysam_for_all_indel_bases' not in c['options'] for c in cases)
    out = os.path.join(HERE, 'clair_call', 'clair_call_golden.json.gz')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, 'wb') as f, gzip.GzipFile(fileobj=f, mode='wb', filename='', mtime=0) as z:
        z.write(json.dumps(dict(numpy=np.__version__, python=sys.version.split()[0], cases=cases)).encode())
    print(out, os.path.getsize(out), 'bytes;', sum(len(c['vcf'].splitlines()) for c in cases), 'lines of VCF')


if __name__ == '__main__':
    main()
