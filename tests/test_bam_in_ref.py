"""CPU tests of BAM read input: the restatement (tests/bam_in_ref.py) is pinned to what samtools itself gives for its own test input
(tests/golden/bam_reads), the framing and the sniffing of fastx.open_once run without a GPU, and the walk the GPU kernel runs
(csrc/bam_walk_core.h) is built for the host with plain g++ (scripts/bam_walk_host_check.cpp) and takes every case, the malformed ones
included, to the status and the rows the restatement gives."""
import collections
import json
import os
import re
import struct
import subprocess

import pytest

import bam_in_cases as bc
import bam_in_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='module')
def golden():
    return json.load(open(os.path.join(GOLDEN, 'bam_reads', 'bam_reads_golden.json')))


def as_text(reads):
    return [(n, s.decode(), q.decode() if q is not None else None) for n, s, q in reads]


def multiset(records):
    return collections.Counter((re.sub(r'/[12]$', '', n), s, q) for n, s, q in records)


def test_restatement_gives_what_samtools_fastq_gives(golden):
    g = golden['bam2fq.001.bam']
    text = ref.inflate(open(os.path.join(GOLDEN, 'bam_reads', 'bam2fq.001.bam'), 'rb').read())
    rows = ref.walk(text)
    got = as_text(ref.reads(text))
    assert len(rows) == g['records'] == 37 and sum(1 for r in rows if r['flag'] & 0x10) == g['reverse'] == 17 and len(got) == 36
    assert multiset(got) == multiset(g['split']) == multiset(g['one_file'])


@pytest.mark.parametrize('name,n,n_rev', [('range.bam', 112, 56), ('colons.bam', 6, 0)])
def test_restatement_on_files_htslib_wrote(golden, name, n, n_rev):
    text = ref.inflate(open(os.path.join(GOLDEN, 'htslib', name), 'rb').read())
    assert sum(1 for r in ref.walk(text) if r['flag'] & 0x10 and not r['flag'] & 0x900) == n_rev
    got = as_text(ref.reads(text))
    assert len(got) == n and got == [tuple(r) for r in golden[name]['reads']]


def test_the_case_writer_writes_what_gzip_reads():
    for name, f in bc.files().items():
        assert ref.inflate(f['blob']) == f['text'], name
    main = bc.files()['main']
    rows = ref.walk(main['text'])
    assert {r['l_seq'] for r in rows} >= set(bc.LENGTHS) and {r['l_read_name'] for r in rows} >= {2, 255}
    assert any(r['flag'] & 0x100 for r in rows) and any(r['flag'] & 0x800 for r in rows) and any(not r['has_qual'] and r['l_seq'] for r in rows)


def test_malformed_texts_end_in_their_status():
    for name, text, status, offset, n in bc.malformed_texts():
        rows = []
        with pytest.raises(ref.BamError) as e:
            ref.walk(text, rows)
        assert (e.value.status, e.value.offset, len(rows)) == (status, offset, n), name


def test_open_once_tells_a_bam_from_other_gzip(tmp_path):
    import gzip
    from megapath_nano_amd import fastx
    files = bc.files()
    for name in ('main', 'no_quals', 'header_only'):
        p = tmp_path / f'{name}.bam'
        p.write_bytes(files[name]['blob'])
        kind, stream = fastx.open_once(str(p))
        assert kind == 'bam' and stream.read(4) == b'\x1f\x8b\x08\x04'        # nothing was consumed
        stream.close()
    for name, data in (('fq.gz', gzip.compress(b'@r\nACGT\n+\nIIII\n')), ('bgzf_fastq.gz', bc.bgzf(b'@r\nACGT\n+\nIIII\n')),
                       ('bam_text_in_plain_gzip.gz', gzip.compress(files['no_quals']['text'])), ('cut.gz', files['main']['blob'][:20])):
        p = tmp_path / name
        p.write_bytes(data)
        kind, stream = fastx.open_once(str(p))
        stream.close()
        assert kind == 'gzip', name


def test_a_bam_is_no_target(tmp_path):
    from megapath_nano_amd import aligner
    p = tmp_path / 'reads.bam'
    p.write_bytes(bc.files()['no_quals']['blob'])
    with pytest.raises(ValueError, match='read input only'):
        list(aligner.iter_target_records([str(p)]))
    with pytest.raises(ValueError, match='read input only'):
        aligner.load_target(str(p), 15, 10)


def test_block_framing_refuses_what_is_not_bgzf():
    from megapath_nano_amd import ingest
    blob = bc.files()['no_quals']['blob']
    assert ingest.bgzf_block_size(blob[:18]) + len(bc.EOF_BLOCK) == len(blob)
    with pytest.raises(ValueError, match='offset 77'):
        ingest.bgzf_block_size(b'\x1f\x8b\x08\x00' + blob[4:18], 77)
    with pytest.raises(ValueError, match='BC'):
        ingest.bgzf_block_size(blob[:12] + b'XY' + blob[14:18])
    with pytest.raises(ValueError, match='BSIZE'):
        ingest.bgzf_block_size(blob[:16] + struct.pack('<H', 20))


# ---- the walk of the kernel, built for the host ----------------------------------------------------------------------------------
def run_host_check(exe, tmp_path, cases):
    """cases: [(text, cut, max_records)] -> [(status, calls, next, rows as (off, l_seq, flag, l_read_name, has_qual, seq))]"""
    src, dst = tmp_path / 'cases.bin', tmp_path / 'results.bin'
    with open(src, 'wb') as f:
        f.write(struct.pack('<I', len(cases)))
        for text, cut, max_records in cases:
            f.write(struct.pack('<QQI', len(text), cut, max_records) + text)
    subprocess.run([str(exe), str(src), str(dst)], check=True, timeout=300)
    blob, out, p = dst.read_bytes(), [], 0
    for _ in cases:
        status, calls, n, nxt = struct.unpack_from('<iIQq', blob, p)
        p += 24
        out.append((status, calls, nxt, [struct.unpack_from('<qiHBBq', blob, p + 24 * r) for r in range(n)]))
        p += 24 * n
    assert p == len(blob)
    return out


def host_check_cases():
    """(name, text, cut, max_records, expected status, expected next, expected rows): every well-formed and malformed text, whole
    and cut in two at places inside the header, inside fixed fields and at record ends, walked 1, 3 and 65 536 records per call"""
    cases = []
    texts = [(n, f['text'], ref.OK, len(f['text']), None) for n, f in bc.files().items() if n in ('main', 'no_quals', 'header_only', 'only_empty_reads')]
    texts += [(n, t, s, o, k) for n, t, s, o, k in bc.malformed_texts()]
    for name, text, status, nxt, n_rows in texts:
        rows = []
        try:
            ref.walk(text, rows)
        except ref.BamError:
            pass
        want = [(r['off'], r['l_seq'], r['flag'], r['l_read_name'], r['has_qual'], r['seq']) for r in rows]
        assert n_rows is None or len(want) == n_rows
        marks = sorted({1, 5, 9, len(text) // 3, len(text) - 2} | {r[0] + d for r in want[:6] for d in (0, 2, 21, 37)})
        for cut in [0] + [c for c in marks if 0 < c < len(text)]:
            for max_records in ((1, 3, 1 << 16) if len(want) < 10 or cut == 0 else (3,)):
                cases.append((f'{name} cut {cut} by {max_records}', text, cut, max_records, status, nxt, want))
    return cases


def test_host_build_of_the_walk_agrees(tmp_path):
    exe = tmp_path / 'bam_walk_host_check'
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-o', str(exe), os.path.join(ROOT, 'scripts', 'bam_walk_host_check.cpp')], check=True)
    cases = host_check_cases()
    assert len(cases) > 100
    got = run_host_check(exe, tmp_path, [(c[1], c[2], c[3]) for c in cases])
    for (name, text, cut, max_records, status, nxt, want), (g_status, g_calls, g_next, g_rows) in zip(cases, got):
        assert (g_status, g_next) == (status, nxt), name
        assert g_rows == want, name
        if status == ref.OK and not cut:
            assert g_calls == len(want) // max_records + 1, name
