"""Regenerates tests/golden/nanosplit_golden.json: (read list, input files) -> output files of the REFERENCE's own prebuilt read
splitter, /root/reference/bin/tools/nanosplit (an x86-64 ELF shipped in the reference tree).  Run in the build container only:
/root/reference does not exist on the GPU box.  The fixture is data (inputs and expected outputs as text), not source.

In the list text `{dir}/` stands for the directory the call ran in.  No case has a malformed list line: the reference tool's
behaviour on one (it reuses the previous pair) is outside the contract."""
import gzip
import json
import os
import subprocess
import tempfile

REF = '/root/reference/bin/tools/nanosplit'
HERE = os.path.dirname(os.path.abspath(__file__))

FQ_A = ('@r1 runid=ab12 ch=7\nACGTACGTAC\n+\n!!!!!#####\n'          # with a comment; listed for two files
        '@r2\nTTTTGGGGCCCCAAAAN\n+\nIIIIIIIIIIIIIIII5\n'             # without a comment; its pair is listed twice
        '@r3 empty\n\n+\n\n'                                         # an empty sequence
        '@r4\tcomment after a tab\nGATTACA\n+\n7654321\n'
        '@shared in_fastq\nCCCC\n+\n&&&&\n'                          # the name also occurs in the FASTA
        '@unlisted\nAAAA\n+\n))))\n')
FA_B = ('>f1 multi line\nACGTACGTACGTACGTACGT\nTTTTTTTTTTTTTTTTTTTT\nGG\n'
        '>shared in_fasta\nGGGGGGGG\nAAAA\n'
        '>f2\nN\n'
        '>unlisted2 x\nACGT\n')
FQ_C = ''.join(f'@z{i} n={i}\n{"ACGGT" * (i + 1)}\n+\n{"FGHIJ" * (i + 1)}\n' for i in range(6))

CALLS = [
    # a FASTQ and a FASTA in one call; list lines out of read order; a read in two files; a pair twice; a file listed only for
    # a name that does not occur (created empty); a name present in both inputs; the last line without a newline
    dict(name='fastq_and_fasta', files={'a.fq': FQ_A, 'b.fa': FA_B}, inputs=['a.fq', 'b.fa'],
         list='f2\t{dir}/out_x\nr4\t{dir}/out_y\nr1\t{dir}/out_x\nr2 {dir}/out_y\nr1\t{dir}/out_y\nr2 {dir}/out_y\nghost\t{dir}/out_empty\n'
              'shared\t{dir}/out_x\nr3\t{dir}/out_x\nf1\t{dir}/out_z\nshared\t{dir}/out_z'),
    # the same inputs in the other order: the order of the input files decides
    dict(name='fasta_then_fastq', files={'a.fq': FQ_A, 'b.fa': FA_B}, inputs=['b.fa', 'a.fq'],
         list='shared\t{dir}/s\nr1\t{dir}/s\nf2\t{dir}/s\n'),
    # gzip input beside a plain one, and a file given twice: its records are written twice
    dict(name='gzip_and_repeat', files={'c.fq.gz': FQ_C, 'a.fq': FQ_A}, gz=['c.fq.gz'], inputs=['c.fq.gz', 'a.fq', 'c.fq.gz'],
         list='z5\t{dir}/odd\nz0\t{dir}/even\nz3\t{dir}/odd\nz2\t{dir}/even\nz1\t{dir}/odd\nz4\t{dir}/even\nr2\t{dir}/odd\nz3\t{dir}/even\n'),
]


def main():
    cases = []
    for call in CALLS:
        with tempfile.TemporaryDirectory(prefix='ns') as d:
            for fn, text in call['files'].items():
                data = text.encode()
                with open(os.path.join(d, fn), 'wb') as f:
                    f.write(gzip.compress(data, mtime=0) if fn in call.get('gz', ()) else data)
            with open(os.path.join(d, 'list.tsv'), 'w') as f:
                f.write(call['list'].replace('{dir}', d))
            before = set(os.listdir(d))
            p = subprocess.run([REF, os.path.join(d, 'list.tsv')] + [os.path.join(d, x) for x in call['inputs']], capture_output=True, timeout=60)
            assert p.returncode == 0, (call['name'], p.stderr[-200:])
            outputs = {fn: open(os.path.join(d, fn), 'rb').read().decode('latin-1') for fn in sorted(set(os.listdir(d)) - before)}
        cases.append(dict(name=call['name'], files=call['files'], gz=call.get('gz', []), inputs=call['inputs'], list=call['list'], outputs=outputs))
        print(call['name'], {k: len(v) for k, v in outputs.items()})
    json.dump(dict(generator='tests/golden/make_nanosplit_golden.py', reference_binary='bin/tools/nanosplit (prebuilt, reference tree)', cases=cases),
              open(os.path.join(HERE, 'nanosplit_golden.json'), 'w'), indent=1)
    print(len(cases), 'calls')


if __name__ == '__main__':
    main()
