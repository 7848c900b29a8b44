"""Records tests/golden/local_realign/local_realign_golden.json.gz with the reference's own programs.

    python tests/golden/make_local_realign_golden.py <reference tree> --samtools PATH

<reference tree> is a checkout of the project this one follows (its bin/realignment holds local_realignment.py,
extract_vcf_position.py, fast_align_reads2ref.py, pyssw.py and realign/ssw.c).  PATH is samtools 1.13 built from that tree's
bin/samtools-1.13, outside this repository:

    ./configure --without-curses --disable-bz2 --disable-lzma --disable-libcurl && make

The scripts are copied to a temporary directory, ssw.c is compiled to realign/libssw.so beside them, and for every case of
tests/local_realign_cases.constructed_cases() the BAM, its .bai and the FASTA's .fai are made with that samtools.  Then the
UNMODIFIED local_realignment.py runs once per site (as realignment.sh starts it) and the unmodified extract_vcf_position.py once per
case.  Only data is stored: the SAM lines, the contig, the positions, the VCF text, the lines the scripts wrote, the VCF and the
standard output of extract_vcf_position.py.  A site at which the script raises has no line (`raised` lists those).  The deep case
(more than 8000 reads, so that mpileup's -d 8000 acts) is stored as its seed and the expected lines in local_realign_deep.json."""
import argparse
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import local_realign_cases as lc      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('reference')
    ap.add_argument('--samtools', required=True)
    a = ap.parse_args()
    samtools = os.path.abspath(a.samtools)
    src = os.path.join(a.reference, 'bin', 'realignment')
    out_dir = os.path.join(HERE, 'local_realign')
    os.makedirs(out_dir, exist_ok=True)
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        tool = os.path.join(tmp, 'realignment')
        os.makedirs(os.path.join(tool, 'realign'))
        for fn in ('local_realignment.py', 'extract_vcf_position.py', 'fast_align_reads2ref.py', 'pyssw.py'):
            shutil.copy(os.path.join(src, fn), tool)
        subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', os.path.join(tool, 'realign', 'libssw.so'), os.path.join(src, 'realign', 'ssw.c'), '-lm'])
        deep = None
        for case in lc.constructed_cases() + [lc.deep_case(2404)]:
            d = os.path.join(tmp, case['name'])
            os.makedirs(os.path.join(d, 'tmp'))
            with open(os.path.join(d, 'in.sam'), 'w') as f:
                f.write('@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:%s\tLN:%d\n' % (lc.CTG, len(case['seq'])) + ''.join(l + '\n' for l in case['lines']))
            with open(os.path.join(d, 'ref.fa'), 'w') as f:
                f.write('>%s\n' % lc.CTG + ''.join(case['seq'][i:i + 60] + '\n' for i in range(0, len(case['seq']), 60)))
            with open(os.path.join(d, 'in.vcf'), 'w') as f:
                f.write(case['vcf'])
            subprocess.check_call([samtools, 'view', '-b', '-o', os.path.join(d, 'in.bam'), os.path.join(d, 'in.sam')])
            subprocess.check_call([samtools, 'index', os.path.join(d, 'in.bam')])
            subprocess.check_call([samtools, 'faidx', os.path.join(d, 'ref.fa')])
            lines, raised = '', []
            for k, pos in enumerate(case['positions']):
                fn = os.path.join(d, 'tmp', '0_output_%d' % (k + 1))
                p = subprocess.run([sys.executable, os.path.join(tool, 'local_realignment.py'), '--bam_fn', os.path.join(d, 'in.bam'), '--ref_fn',
                                    os.path.join(d, 'ref.fa'), '--pos', str(pos), '--platform', 'ont', '--samtools', samtools, '--ctgName', lc.CTG,
                                    '--output_fn', fn], capture_output=True, text=True)
                if p.returncode != 0:
                    raised.append(pos)
                    print(case['name'], pos, 'raised:', p.stderr.strip().splitlines()[-1:], file=sys.stderr)
                    continue
                with open(fn) as f:
                    lines += f.read()
            alt_fn = os.path.join(d, 'tmp', '0_all_alt_info')
            with open(alt_fn, 'w') as f:
                f.write(lines)
            p = subprocess.run([sys.executable, os.path.join(tool, 'extract_vcf_position.py'), '--vcf_fn', os.path.join(d, 'in.vcf'), '--alt_fn', alt_fn,
                                '--output_fn', os.path.join(d, '0_realign.vcf')], capture_output=True, text=True, check=True)
            with open(os.path.join(d, '0_realign.vcf')) as f:
                vcf = f.read()
            if case['name'] == 'deep':              # stored by its seed: the reads are made again by local_realign_cases.deep_case
                deep = dict(seed=case['seed'], reads=len(case['lines']), positions=case['positions'], expected_lines=lines, expected_vcf=vcf,
                            expected_stdout=p.stdout)
            else:
                cases.append(dict(case, expected_lines=lines, raised=raised, expected_vcf=vcf, expected_stdout=p.stdout))
            print(case['name'], len(case['lines']), 'reads', len(lines.splitlines()), 'lines', file=sys.stderr)
    with open(os.path.join(out_dir, 'local_realign_golden.json.gz'), 'wb') as f, gzip.GzipFile(fileobj=f, mode='wb', filename='', mtime=0) as z:
        z.write(json.dumps(dict(cases=cases), separators=(',', ':')).encode())
    with open(os.path.join(out_dir, 'local_realign_deep.json'), 'w') as f:
        json.dump(deep, f, indent=0)
        f.write('\n')


if __name__ == '__main__':
    main()
