"""GPU tests (-m gpu) of fastx.nanosplit on the resident text (MPN_READ_INGEST=device) against the host path
(fastx.nanosplit(..., device=False) with the knob unset), byte for byte and count for count: the reference binary's goldens, generated
reads in the plain, gzip and BGZF forms at two text sizes, many outputs, the hand-overs to the host in the middle of a call, a damaged
BGZF block and bin/mpn-nanosplit.  Where the input is plain four-line FASTQ the host's parser and mapper.split_reads are replaced by
functions that raise: the files can then only come from the lookup and the emit kernels."""
import gzip
import json
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import fastq_scan_ref as scan_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'nanosplit_golden.json')))


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', '65536')
    monkeypatch.delenv('MPN_READ_INGEST', raising=False)


def bgzf_block(payload):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    data = c.compress(payload) + c.flush()
    return (b'\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0' + struct.pack('<H', len(data) + 25) + data +
            struct.pack('<II', zlib.crc32(payload) & 0xffffffff, len(payload)))


def bgzf(text, block=3000):
    return b''.join(bgzf_block(text[a:a + block]) for a in range(0, len(text), block)) + bgzf_block(b'')


def lay_out(d, files, pairs, inputs):
    """files: {name: bytes}; pairs: [(read id, output name)], or the text of a list with {dir} in front of its output names
    -> (list path, input paths), everything under d"""
    os.makedirs(d)
    for name, data in files.items():
        with open(os.path.join(d, name), 'wb') as f:
            f.write(data)
    with open(os.path.join(d, 'list.tsv'), 'wb') as f:
        if isinstance(pairs, str):
            f.write(pairs.replace('{dir}', d).encode())
        else:
            f.write(b''.join(rid + b'\t' + os.fsencode(d) + b'/' + out + b'\n' for rid, out in pairs))
    return os.path.join(d, 'list.tsv'), [os.path.join(d, x) for x in inputs]


def outputs_of(d, files, written):
    made = sorted(set(os.listdir(d)) - set(files) - {'list.tsv'})
    assert sorted(os.path.basename(p) for p, _ in written) == made              # every listed file is created, and no other
    return {fn: open(os.path.join(d, fn), 'rb').read() for fn in made}, [(os.path.basename(p), k) for p, k in written]


def guard(monkeypatch):
    from megapath_nano_amd import fastx, mapper

    def refuse(*a, **k):
        raise AssertionError('the host path was taken')
    monkeypatch.setattr(fastx, 'iter_fastx_full', refuse)
    monkeypatch.setattr(mapper, 'split_reads', refuse)


def both(tmp_path, monkeypatch, files, pairs, inputs, guarded=False, timings=None):
    """-> ({output name: bytes} of the device path, its (name, count) list) after both paths agreed"""
    from megapath_nano_amd import fastx
    tag = str(len(os.listdir(tmp_path)))
    monkeypatch.delenv('MPN_READ_INGEST', raising=False)
    d = os.path.join(str(tmp_path), 'host' + tag)
    lst, paths = lay_out(d, files, pairs, inputs)
    want = outputs_of(d, files, fastx.nanosplit(lst, paths, device=False))
    d = os.path.join(str(tmp_path), 'dev' + tag)
    lst, paths = lay_out(d, files, pairs, inputs)
    with monkeypatch.context() as m:
        m.setenv('MPN_READ_INGEST', 'device')
        if guarded:
            guard(m)
        got = outputs_of(d, files, fastx.nanosplit(lst, paths, timings=timings))
    assert got[1] == want[1]
    assert sorted(got[0]) == sorted(want[0])
    for fn in want[0]:
        assert got[0][fn] == want[0][fn], fn
    return got


@pytest.mark.parametrize('case', GOLD['cases'], ids=[c['name'] for c in GOLD['cases']])
def test_goldens_of_the_reference_binary(libmpn, monkeypatch, tmp_path, case):
    """the FASTA, mixed and gzip inputs of the goldens: the device path hands over to the host where it has to"""
    files = {fn: (gzip.compress(text.encode()) if fn in case['gz'] else text.encode()) for fn, text in case['files'].items()}
    for size in ('64', '65536'):
        monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', size)
        got, counts = both(tmp_path, monkeypatch, files, case['list'], case['inputs'])
        assert {fn: data.decode('latin-1') for fn, data in got.items()} == case['outputs']


@pytest.fixture(scope='module')
def generated():
    """about 300 reads of 0 .. 3000 bases in two files that share a name; 12 outputs, one of them listed for an absent name only"""
    rng = np.random.default_rng(190)
    recs, pairs = [], []
    for i in range(300):
        n = int(rng.integers(0, 3001)) if i % 50 else 0
        head = b'read_%d' % i + (b'', b' comment %d' % i, b' ', b'\tx y')[i % 4]
        recs.append(scan_ref.rec(head, scan_ref._bases(n, i), scan_ref._quals(n, i)))
        if i % 7 != 3:                                                         # a seventh of the reads is not listed
            pairs.append((b'read_%d' % i, b'out_%d' % (i % 10)))
        if i % 10 == 4:
            pairs.append((b'read_%d' % i, b'out_%d' % ((i + 3) % 10)))         # a tenth of them for a second output
    shared = scan_ref.rec(b'shared first', b'ACGTACGTAC'), scan_ref.rec(b'shared second', b'TTTT')
    every = scan_ref.rec(b'every where', scan_ref._bases(2500, 1), scan_ref._quals(2500, 1))
    a = b''.join(recs[:100]) + shared[0] + every + b''.join(recs[100:180])
    b = b''.join(recs[180:250]) + shared[1] + b''.join(recs[250:])
    pairs += [(b'shared', b'out_2'), (b'shared', b'out_10'), (b'nowhere', b'out_11')] + [(b'every', b'out_%d' % g) for g in range(11)]
    return a, b, pairs


@pytest.mark.parametrize('form', ['plain', 'gzip', 'bgzf'])
def test_generated_reads_in_every_form_and_text_size(libmpn, monkeypatch, tmp_path, generated, form):
    a, b, pairs = generated
    pack = {'plain': lambda t: t, 'gzip': lambda t: gzip.compress(t, 6), 'bgzf': bgzf}[form]
    files = {'a.fq': pack(a), 'b.fq': pack(b)}
    for size in ('5000', '65536'):                          # records straddle the texts; `every` needs a round per output at 5000
        monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', size)
        t = {}
        got, counts = both(tmp_path, monkeypatch, files, pairs, ['a.fq', 'b.fq'], guarded=True, timings=t)
        assert dict(counts)['out_11'] == 0 and got['out_11'] == b'' and dict(counts)['out_10'] == 3
        assert got['out_2'].index(b'@shared first\n') < got['out_2'].index(b'@shared second\n')
        assert got['out_10'].count(b'@every where\n') == 1 and b'@read_2 \n' not in got['out_2'] and b'@read_2\n' in got['out_2']
        assert t['records'] == 303 and 'host' not in t and min(t['lookup_device_ms'], t['emit_device_ms']) > 0


def test_1100_outputs(libmpn, monkeypatch, tmp_path):
    recs = [scan_ref.rec(b'r%d c' % i, scan_ref._bases(20 + i, i), scan_ref._quals(20 + i, i)) for i in range(40)]
    pairs = [(b'r%d' % i, b'o%d' % g) for i in range(40) for g in range(i, 1100, 40)] + [(b'r7', b'o%d' % g) for g in range(1100)]
    got, counts = both(tmp_path, monkeypatch, {'in.fq': b''.join(recs)}, pairs, ['in.fq'], guarded=True)
    assert len(got) == 1100 and all(k in (1, 2) for _, k in counts) and sum(k for _, k in counts) == 2200 - len(range(7, 1100, 40))


def test_the_host_finishes_a_file_and_a_device_file_follows(libmpn, monkeypatch, tmp_path):
    recs = [scan_ref.rec(b'm%d' % i, scan_ref._bases(200 + i, i), scan_ref._quals(200 + i, i)) for i in range(30)]
    multi = b'@multi line\nACGT\nACGT\n+\nIIII\nIIII\n'
    files = {'a.fq': b''.join(recs[:10]) + multi + b''.join(recs[10:20]), 'b.fq': b''.join(recs[20:]),
             'c.fa': b'>m3 in fasta\nACGT\nAC\n>other\nA\n', 'empty.fq': b''}
    pairs = [(b'm%d' % i, b'out_%d' % (i % 3)) for i in range(30)] + [(b'multi', b'out_0'), (b'multi', b'out_2')]
    for size in ('1500', '65536'):
        monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', size)
        t = {}
        got, counts = both(tmp_path, monkeypatch, files, pairs, ['a.fq', 'b.fq'], timings=t)
        assert t['records'] == 20 and 'host' in t                                   # ten before the multi-line record, ten of b.fq
        assert got['out_0'].index(b'@m9\n') < got['out_0'].index(b'@multi line\nACGTACGT\n') < got['out_0'].index(b'@m12\n') < got['out_0'].index(b'@m21\n')
        # a FASTA file (and an empty one) between two FASTQ files
        t = {}
        got, counts = both(tmp_path, monkeypatch, files, pairs, ['b.fq', 'c.fa', 'empty.fq', 'a.fq'], timings=t)
        assert t['records'] == 20
        assert got['out_0'].index(b'@m27\n') < got['out_0'].index(b'>m3 in fasta\nACGTAC\n') < got['out_0'].index(b'@m0\n')


def test_a_damaged_bgzf_block_raises_and_earlier_texts_stay_written(libmpn, monkeypatch, tmp_path):
    from megapath_nano_amd import fastx
    recs = [scan_ref.rec(b'd%d' % i, scan_ref._bases(900, i), scan_ref._quals(900, i)) for i in range(12)]
    text = b''.join(recs)
    blocks = [bgzf_block(text[a:a + 3000]) for a in range(0, len(text), 3000)]
    k = len(blocks) - 2
    blocks[k] = blocks[k][:-8] + struct.pack('<I', (zlib.crc32(text[3000 * k:3000 * k + 3000]) ^ 1) & 0xffffffff) + blocks[k][-4:]
    lst, paths = lay_out(os.path.join(str(tmp_path), 'd'), {'in.fq.gz': b''.join(blocks) + bgzf_block(b'')},
                         [(b'd%d' % i, b'out') for i in range(12)], ['in.fq.gz'])
    monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', '4000')
    monkeypatch.setenv('MPN_READ_INGEST', 'device')
    with pytest.raises(ValueError, match='BGZF block'):
        fastx.nanosplit(lst, paths)
    out = open(os.path.join(str(tmp_path), 'd', 'out'), 'rb').read()
    assert out.startswith(recs[0] + recs[1]) and out == text[:len(out)] and len(out) < len(text) and out.endswith(b'\n')
    # a BAM file and a saved index raise what they raise on the host path
    bam = bgzf_block(b'BAM\x01' + b'\0' * 8)
    for name, data, what in (('x.bam', bam, 'a BAM file is taken as read input only'), ('x.idx', fastx.INDEX_MAGIC + b'\0' * 8, 'a saved index')):
        lst, paths = lay_out(os.path.join(str(tmp_path), name + '_d'), {name: data}, [(b'a', b'out')], [name])
        with pytest.raises(ValueError, match=what):
            fastx.nanosplit(lst, paths)
        monkeypatch.delenv('MPN_READ_INGEST')
        with pytest.raises(ValueError, match=what):
            fastx.nanosplit(lst, paths, device=False)
        monkeypatch.setenv('MPN_READ_INGEST', 'device')


def test_executable_takes_the_knob_and_refuses_a_bogus_one(libmpn, monkeypatch, tmp_path, generated):
    from megapath_nano_amd import fastx
    a, b, pairs = generated
    files = {'a.fq': a, 'b.fq.gz': bgzf(b)}
    want, _ = both(tmp_path, monkeypatch, files, pairs, ['a.fq', 'b.fq.gz'], guarded=True)
    d = os.path.join(str(tmp_path), 'exe')
    lst, paths = lay_out(d, files, pairs, ['a.fq', 'b.fq.gz'])
    exe = [sys.executable, os.path.join(ROOT, 'bin', 'mpn-nanosplit'), lst] + paths
    p = subprocess.run(exe, capture_output=True, timeout=300, env=dict(os.environ, MPN_READ_INGEST='device', MPN_INGEST_BATCH_BYTES='20000'))
    assert p.returncode == 0, p.stderr[-500:]
    assert {fn: open(os.path.join(d, fn), 'rb').read() for fn in want} == want
    p = subprocess.run(exe, capture_output=True, timeout=300, env=dict(os.environ, MPN_READ_INGEST='bogus'))
    assert p.returncode != 0 and b'MPN_READ_INGEST=bogus' in p.stderr
    monkeypatch.setenv('MPN_READ_INGEST', 'bogus')
    with pytest.raises(ValueError, match='MPN_READ_INGEST=bogus'):
        fastx.nanosplit(lst, paths)
