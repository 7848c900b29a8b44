"""Records tests/golden/read_realign/*.json.gz with the reference's own realign_illumina_reads.py.

    python tests/golden/make_read_realign_golden.py <reference tree> --samtools PATH

<reference tree> is a checkout of the project this one follows (its bin/realignment holds realign_illumina_reads.py, the vendored
intervaltree and realign/realigner.cpp, ssw_cpp.cpp and ssw.c).  PATH is samtools 1.13 built from that tree's bin/samtools-1.13,
outside this repository:

    ./configure --without-curses --disable-bz2 --disable-lzma --disable-libcurl && make

The UNMODIFIED script and the intervaltree are copied to a temporary directory outside the repository.  realign/realigner beside
them is the reference's own library (the recipe of oracle/Makefile).  realign/debruijn_graph is a STAND-IN: tests/golden/
dbg_standin.cpp, this project's csrc/dbg_core.h behind the script's get_consensus (the reference's graph library needs Boost and
does not compile without it).  The goldens therefore pin everything in the script except the consensus, which is the project's
own rule, pinned by tests/test_dbg_ref.py.  For every case of tests/read_realign_cases.py listed below the BAM, its .bai and the
FASTA's .fai are made with that samtools, and the script runs under CPython with `--read_fn PIPE`.

Only data is stored: how the case is generated (its function and arguments in tests/read_realign_cases.py), for the small cases
also the SAM lines and the contig, the arguments, the records the script printed and the header it printed without the @PG lines
that `samtools view -h` adds.

The maker fails unless at least three cases have a read whose CIGAR or POS changes, one has a read that is realigned in two
windows of overlapping splits, and one spans at least three chunks (both judged with tests/read_realign_ref.py's trace)."""
import argparse
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import read_realign_cases as rc      # noqa: E402
import read_realign_ref as ref       # noqa: E402

# (function in read_realign_cases, keyword arguments, index into its list or None)
CASES = [('long_cigars', {}, None), ('long_insertions', {}, None), ('chunk_edges', {}, 0), ('lagging_chunks', {}, None),
         ('qualities_and_letters', {}, None), ('windows', {}, None), ('plain_variants', {}, None), ('deep_window', {}, None),
         ('plain_variants', dict(seed=33, n=9000, depth=25), None), ('plain_variants', dict(seed=45, n=16000, depth=8), None)]
SMALL = 48 << 10


def generate(spec):
    fn, kw, index = spec
    got = getattr(rc, fn)(**kw)
    return got if index is None else got[index]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('reference')
    ap.add_argument('--samtools', required=True)
    a = ap.parse_args()
    samtools = os.path.abspath(a.samtools)
    src = os.path.join(a.reference, 'bin', 'realignment')
    out_dir = os.path.join(HERE, 'read_realign')
    os.makedirs(out_dir, exist_ok=True)
    changed_cases = two_windows = three_chunks = 0
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(os.path.join(src, 'realign_illumina_reads.py'), d)
        shutil.copytree(os.path.join(src, 'intervaltree'), os.path.join(d, 'intervaltree'))
        os.makedirs(os.path.join(d, 'realign'))
        r = os.path.join(src, 'realign')
        subprocess.check_call(['gcc', '-O2', '-fPIC', '-w', '-c', '-o', os.path.join(d, 'ssw_c.o'), os.path.join(r, 'ssw.c')])
        subprocess.check_call(['g++', '-std=c++14', '-O1', '-fPIC', '-w', '-shared', '-o', os.path.join(d, 'realign', 'realigner'),
                               os.path.join(r, 'realigner.cpp'), os.path.join(r, 'ssw_cpp.cpp'), os.path.join(d, 'ssw_c.o')])
        subprocess.check_call(['g++', '-std=c++17', '-O2', '-fPIC', '-shared', '-o', os.path.join(d, 'realign', 'debruijn_graph'),
                               os.path.join(HERE, 'dbg_standin.cpp')])
        for n, spec in enumerate(CASES):
            case = generate(spec)
            w = os.path.join(d, f'case{n}')
            os.makedirs(w)
            lines = rc.sam_lines(case)
            with open(os.path.join(w, 'in.sam'), 'w') as f:
                f.write(rc.header_text(case) + ''.join(lines))
            with open(os.path.join(w, 'ref.fa'), 'w') as f:
                f.write(f'>{rc.CTG}\n' + ''.join(case['contig'][i:i + 60] + '\n' for i in range(0, len(case['contig']), 60)))
            subprocess.check_call([samtools, 'view', '-b', '-o', os.path.join(w, 'in.bam'), os.path.join(w, 'in.sam')])
            subprocess.check_call([samtools, 'index', os.path.join(w, 'in.bam')])
            subprocess.check_call([samtools, 'faidx', os.path.join(w, 'ref.fa')])
            args = ['--bam_fn', os.path.join(w, 'in.bam'), '--ref_fn', os.path.join(w, 'ref.fa'), '--ctgName', rc.CTG, '--minMQ', str(case['min_mq']),
                    '--minCoverage', str(case['min_coverage']), '--read_fn', 'PIPE']
            text = subprocess.run([sys.executable, os.path.join(d, 'realign_illumina_reads.py'), '--samtools', samtools] + args, check=True,
                                  stdout=subprocess.PIPE, cwd=w).stdout.decode()
            got = text.splitlines(keepends=True)
            header = [l for l in got if l.startswith('@') and not l.startswith('@PG')]
            records = [l for l in got if not l.startswith('@')]
            # what the case reaches
            trace = []
            ref.realign(lines, case['contig'], rc.CTG, case['min_mq'], case['min_coverage'], consensus=lambda *x: [], trace=trace)
            by_name = {ref.name_of(k): r for k, r in enumerate(case['records'])}
            changed = sum((l.split('\t')[5], int(l.split('\t')[3]) - 1) != (by_name[l.split('\t')[0]]['cigar'], by_name[l.split('\t')[0]]['pos'])
                          for l in records)
            twice = any(set(a_) & set(b_) for t in trace if t['members'] for s1, s2 in zip(t['members'], t['members'][1:]) for a_ in s1 for b_ in s2)
            changed_cases += changed > 0
            two_windows += twice
            three_chunks += len(trace) >= 3
            stored = dict(name=case['name'], generator=list(spec), args=dict(ctgName=rc.CTG, minMQ=case['min_mq'], minCoverage=case['min_coverage']),
                          header=header, records=records, changed=changed)
            if sum(map(len, lines)) <= SMALL:
                stored['sam_lines'], stored['contig'] = lines, case['contig']
            path = os.path.join(out_dir, case['name'] + '.json.gz')
            with open(path, 'wb') as f:
                f.write(gzip.compress(json.dumps(stored, indent=0).encode(), mtime=0))
            print(f'{case["name"]}: {len(records)} records, {changed} changed, {len(trace)} yields, two windows: {twice}, {os.path.getsize(path)} bytes')
    if changed_cases < 3 or not two_windows or not three_chunks:
        sys.exit(f'the cases do not reach what they are for: {changed_cases} with a changed read, {two_windows} with a read in two windows, '
                 f'{three_chunks} over three chunks')


if __name__ == '__main__':
    main()
