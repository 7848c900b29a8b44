"""CPU test: the events and the decoding through the arithmetic and the index maps the kernels use (csrc/clair_call_core.h), built for
the host with g++ (scripts/clair_call_host_check.cpp, under AddressSanitizer and UBSan where the toolchain has their runtimes),
equal the restatement (tests/clair_call_ref.py, 'legacy') exactly -- before any of it meets a GPU -- and malformed input ends in a
message, not in an access outside the text."""
import os
import struct
import subprocess

import numpy as np
import pytest

import clair_call_cases as cc
import clair_call_ref as ref
from megapath_nano_amd import clair_call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp('clair_call_host') / 'clair_call_host_check'
    src = os.path.join(ROOT, 'scripts', 'clair_call_host_check.cpp')
    base = ['g++', '-std=c++17', '-Wall', '-Werror', '-o', str(out), src]
    subprocess.run(base + ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], check=True)
    return out


def run(exe, tmp_path, blob, check=True):
    path = tmp_path / 'case.bin'
    path.write_bytes(blob)
    p = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600)
    if check:
        assert p.returncode == 0, p.stderr[-2000:]
    return p


def case_blob(tmp_path, case, options, lines=None):
    bam_fn = pc_write(tmp_path, case, lines)
    text, reads = cc.bam_text_reads(bam_fn)
    pos, rlen = np.array([r[2] for r in reads], dtype=np.int64), np.array([r[1] for r in reads], dtype=np.int64)
    begin, end = clair_call.site_ranges(pos, rlen, case['sites'])
    return cc.host_case_bytes(text, reads, case['seq'].encode(), case['sites'], list(zip(begin.tolist(), end.tolist())), case['refs'], case['x'],
                              case['probs'], options), reads


def pc_write(tmp_path, case, lines=None):
    import pileup_cases as pc
    return pc.write_bam(os.path.join(str(tmp_path), 'in.bam'), [(cc.CTG, case['seq'])], lines if lines is not None else case['lines'])


def parse(stdout):
    events, rows = {}, {}
    for line in stdout.splitlines():
        f = line.split(' ')
        if f[0] == 'E':
            events.setdefault(int(f[1]), []).append((int(f[2]), int(f[3]), int(f[4]), int(f[5]), int(f[6]), {'-': '', '!': None}.get(f[7], f[7])))
        elif f[0] == 'R':
            rows[int(f[1])] = f[2:]
        else:
            raise AssertionError(line)
    return events, rows


@pytest.mark.parametrize('seed,all_bases,haploid,show', [(11, True, False, True), (12, False, False, False), (13, True, True, True), (14, False, False, True)])
def test_host_build_equals_the_restatement(exe, tmp_path, seed, all_bases, haploid, show):
    case = cc.cached_case(seed, long_events=seed > 12)
    blob, _ = case_blob(tmp_path, case, (1 if all_bases else 0) | (2 if haploid else 0) | (4 if show else 0))
    events, rows = parse(run(exe, tmp_path, blob).stdout)
    want_events = cc.expected_events(case)
    want_rows = cc.expected_rows(case, all_bases, haploid, show)
    emitted = 0
    for s, we, wr in zip(case['sites'], want_events, want_rows):
        assert events.get(s, []) == we, s
        got = rows[s]
        if wr is None:
            assert got[0] != '0', (s, got)
            continue
        parts = wr[1]
        alts = parts['alt'].split(',')
        flags = sum(1 << i for i, f in enumerate(parts['flags']) if f)
        bits, = struct.unpack('<I', np.float32(parts['p']).tobytes())
        assert got == ['0', str(flags), str(ref.GENOTYPES.index(parts['gt'])), str(parts['gt21']), str(parts['task']), str(bits), str(parts['support']),
                       str(parts['depth']), parts['ref'], alts[0], alts[1] if len(alts) > 1 else '-'], (s, got, parts)
        emitted += 1
    assert emitted > 40


@pytest.mark.parametrize('name', cc.GOLDEN_NAMES)
def test_host_build_on_the_goldens(exe, tmp_path, name):
    """REF, ALT, GT and DP of every record the reference's own call_var.py printed"""
    case = cc.golden_case(name)
    kw = case['kw']
    blob, _ = case_blob(tmp_path, case, (1 if kw['pysam_all'] else 0) | (2 if kw['haploid'] else 0) | (4 if kw['show_ref'] else 0))
    path = tmp_path / 'case.bin'
    path.write_bytes(blob)
    out = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    got = []
    for line in out.stdout.splitlines():          # (a position can repeat: the rows in the order of the lines)
        f = line.split(' ')
        if f[0] == 'R' and f[2] == '0':
            got.append([f[1], f[-3], f[-2] if f[-1] == '-' else f[-2] + ',' + f[-1], ref.GENOTYPES[int(f[4])], f[9]])
    want = [l.split('\t') for l in cc.records(case['vcf'])]
    assert got == [[w[1], w[3], w[4], w[9].split(':')[0], w[9].split(':')[2]] for w in want] and len(want) > 0


def test_the_two_deletion_reset_at_the_end_of_the_contig(exe, tmp_path):
    case = cc.reset_case()
    blob, _ = case_blob(tmp_path, case, 1 | 4)
    events, rows = parse(run(exe, tmp_path, blob).stdout)
    site = case['sites'][0]
    assert events[site] == [(1, 5, 1, 0, 2, '')] and rows[site][:2] == ['0', '1'] and rows[site][-3] == rows[site][-2]


def test_an_insertion_directly_followed_by_a_deletion(exe, tmp_path):
    """the deletion is spelled into the inserted bases, as the script takes them from the pile-up's text"""
    case = cc.insdel_case()
    one = dict(case, sites=case['sites'][:1])
    blob, _ = case_blob(tmp_path, one, 1)
    events, rows = parse(run(exe, tmp_path, blob).stdout)
    want = cc.expected_events(one)[0]
    assert events[100] == want and want[0][:5] == (0, 2, 2, 0, 2) and want[0][5].endswith('-2NN') and want[2] == (0, 3, 1, 3, 46, None)
    line, parts = cc.expected_rows(one, True)[0]
    assert rows[100][-3:] == [parts['ref'], parts['alt'], '-'] and parts['alt'].endswith('-2NN')
    two = dict(case, sites=case['sites'][1:], probs=case['probs'][1:])
    blob, _ = case_blob(tmp_path, two, 1)
    assert parse(run(exe, tmp_path, blob).stdout)[1][100] == [str(clair_call.LONG_KEY)]


def test_malformed_input(exe, tmp_path):
    case = cc.cached_case(11)
    seq = case['seq']
    import random
    rng = random.Random(1)
    site = 100
    one = dict(case, sites=[site], refs=[cc.window(seq, site)], x=case['x'][:1], probs=case['probs'][:1])
    # an insertion past the bases, and a read without bases, at the column of the site: a bad read, no access outside
    for line in (cc.sam('short', 0, 80, '20M5I20M', 'A' * 22), cc.sam('nobases', 0, 80, '20M5I20M', '*')):
        blob, _ = case_blob(tmp_path, one, 1, [line])
        assert run(exe, tmp_path, blob).stdout.startswith('B 100 0')
    # a CIGAR past the record: n_cigar raised behind the writer's back
    blob, reads = case_blob(tmp_path, one, 1, [cc.line_of(rng, 'past', 0, 80, [('M', 20), ('I', 2), ('M', 20)])])
    blob = bytearray(blob)
    at = 40 + reads[0][0] + 16
    blob[at:at + 2] = struct.pack('<H', 60000)
    assert run(exe, tmp_path, bytes(blob)).stdout.startswith('B 100 0')
    # a site past the contig: a deletion there has the empty key, and the look-up returns nothing
    far = dict(case, sites=[len(seq) + 4], refs=['A' * 17], x=case['x'][:1], probs=case['probs'][:1])
    blob, _ = case_blob(tmp_path, far, 1, [cc.line_of(rng, 'far', 0, len(seq) - 16, [('M', 20), ('D', 3), ('M', 5)])])
    events, rows = parse(run(exe, tmp_path, blob).stdout)
    assert events[len(seq) + 4] == [(1, 3, 1, 0, 0, '')]
    # NaN probabilities are refused
    nan = dict(one, probs=np.full((1, 90), np.nan, dtype=np.float32))
    blob, _ = case_blob(tmp_path, nan, 1, [])
    assert parse(run(exe, tmp_path, blob).stdout)[1][100] == [str(clair_call.BAD_PROB)]
    # a case file that ends early
    assert run(exe, tmp_path, blob[:100], check=False).returncode == 2
