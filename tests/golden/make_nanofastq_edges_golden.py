"""Regenerates tests/golden/nanofastq_edges_golden.json: stdin -> (stdout, stderr) of the REFERENCE's own prebuilt read filter
(/root/reference/bin/tools/nanofastq, as tests/golden/make_nanofastq_golden.py runs it) on header and line-end edge cases: what the
read filter on the device (MPN_READ_INGEST=device) has to parse and write itself.  Run in the build container only; the fixture
is data (inputs and expected outputs), not source.

Left out on purpose: a header that holds VT or FF.  kseq ends the name at any isspace(), fastq_filter.parse_fastx only at a blank or
a TAB, so the host mirror does not reproduce the binary there."""
import json
import os
import subprocess

REF = '/root/reference/bin/tools/nanofastq'
HERE = os.path.dirname(os.path.abspath(__file__))


def rec(head, seq, qual, plus='+', eol='\n'):
    return f'@{head}{eol}{seq}{eol}{plus}{eol}{qual}{eol}'


def main():
    seq, good, poor = 'ACGTTGCAAC', 'IIIIHHHHGG', '#$#$#$#$#$'
    inputs = {
        'crlf': ''.join(rec(h, seq[:n], good[:n], eol='\r\n') for h, n in (('c1', 10), ('c2 with comment', 7), ('c3\ttab', 4))),
        'headers': ''.join(rec(h, seq, good) for h in ('a ', 'a\tx y', 'a  x', ' a x', '', 'plain', 'b \t', 'c\t')),
        'qual_at': rec('q1', 'ACGT', '@III') + rec('q2 c', 'ACGTA', '+@>II', plus='+anything') + rec('q3', 'ACG', '@@@', plus='+q3 c') +
                   rec('q4', 'ACGTAC', '>IIII@'),
        'no_last_lf': rec('n1 x', seq, good) + rec('n2', 'ACGTA', 'IIII@')[:-1],
        'serials': ''.join(rec(f'r{i} ch={i}', seq[:4 + i % 7], (poor if i % 3 == 2 else good)[:4 + i % 7]) for i in range(12)),
    }
    argsets = [[], ['-h', '1', '-t', '1'], ['-q', '7', '-r', 'p_']]
    cases = []
    for name, text in inputs.items():
        for args in argsets:
            p = subprocess.run([REF] + args, input=text.encode(), capture_output=True, timeout=60)
            assert p.returncode == 0, (name, args, p.stderr[-200:])
            cases.append(dict(input=name, args=args, stdout=p.stdout.decode('latin-1'), stderr=p.stderr.decode('latin-1')))
    json.dump(dict(generator='tests/golden/make_nanofastq_edges_golden.py', reference_binary='bin/tools/nanofastq (prebuilt, reference tree)',
                   inputs=inputs, cases=cases), open(os.path.join(HERE, 'nanofastq_edges_golden.json'), 'w'))
    print(len(cases), 'cases')


if __name__ == '__main__':
    main()
