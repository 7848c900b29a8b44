"""GPU tests (-m gpu) of BAM read input (include/mpn_ingest.h: mpn_bam_flatten, mpn_bam_walk, mpn_bam_decode; ingest.iter_bam_read_batches):
the device against the restatement tests/bam_in_ref.py, field for field, on the cases of tests/bam_in_cases.py and the golden files;
then end to end, a BAM query against the same reads as FASTQ.  Every malformed text here has been through the host build of the walk
under the address and undefined-behaviour sanitizers (scripts/bam_walk_host_check.cpp, tests/test_bam_in_ref.py)."""
import gzip
import json
import os
import threading

import numpy as np
import pandas as pd
import pytest

import bam_in_cases as bc
import bam_in_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
GOLDEN_FILES = {'bam2fq.001.bam': os.path.join(GOLDEN, 'bam_reads', 'bam2fq.001.bam'), 'range.bam': os.path.join(GOLDEN, 'htslib', 'range.bam'),
                'colons.bam': os.path.join(GOLDEN, 'htslib', 'colons.bam')}


@pytest.fixture(scope='module')
def cases(libmpn, tmp_path_factory):
    """name -> dict(path, text, rows, reads): the files of bam_in_cases and the golden files, restated once"""
    d = tmp_path_factory.mktemp('bam_in')
    out = {}
    for name, f in bc.files().items():
        p = d / f'{name}.bam'
        p.write_bytes(f['blob'])
        out[name] = dict(path=str(p), text=f['text'])
    for name, path in GOLDEN_FILES.items():
        out[name] = dict(path=path, text=ref.inflate(open(path, 'rb').read()))
    for c in out.values():
        c['rows'] = ref.walk(c['text'])
        c['reads'] = [ref.read_of(c['text'], r) for r in c['rows'] if not r['flag'] & 0x900]
    return out


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    monkeypatch.delenv('MPN_INGEST_BATCH_BYTES', raising=False)
    monkeypatch.delenv('MPN_BAM_WALK_RECORDS', raising=False)


def upload(data):
    import torch
    buf = np.zeros(max((len(data) + 15) & ~15, 16), dtype=np.uint8)
    buf[:len(data)] = np.frombuffer(data, dtype=np.uint8)
    return torch.from_numpy(buf).cuda()


def row_tuples(rows):
    return [(int(r['off']), int(r['l_seq']), int(r['flag']), int(r['l_read_name']), int(r['has_qual'])) for r in rows]


def want_tuples(rows):
    return [(r['off'], r['l_seq'], r['flag'], r['l_read_name'], r['has_qual']) for r in rows]


def walk_all(text, text_len, max_records, final=True, start=0, at_header=True):
    from megapath_nano_amd import ingest
    rows, calls = [], 0
    while True:
        got, nxt, status = ingest.bam_walk(text, text_len, start, at_header, final, max_records)
        calls += 1
        at_header = at_header and nxt == start
        rows += row_tuples(got)
        start = nxt
        if status != ref.OK or len(got) < max_records:
            return rows, nxt, status, calls


# ---- the kernels on their own -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_records', [1, 3, 64, 65, 1 << 16])
def test_walk_rows_equal_the_restatement(cases, max_records):
    for name in ('main', 'no_quals', 'header_only', 'only_empty_reads', 'bam2fq.001.bam', 'range.bam', 'colons.bam'):
        c = cases[name]
        rows, nxt, status, calls = walk_all(upload(c['text']), len(c['text']), max_records)
        assert (status, nxt) == (ref.OK, len(c['text'])), name
        assert rows == want_tuples(c['rows']), name
        assert calls == len(rows) // max_records + 1, name


def test_walk_stops_at_what_passes_the_end_and_resumes(cases):
    """final = 0: a header or a record that passes the end is where the walk stops, without a status; the tail goes in front of the
    next text.  Cuts inside the magic, l_text, the header text, a reference entry, block_size, the fixed fields, the bases."""
    import torch
    c = cases['main']
    text, want = c['text'], want_tuples(c['rows'])
    first = want[0][0]
    for cut in (0, 2, 6, 3000, first - 9, first, first + 2, first + 21, want[1][0], want[12][0] + 50, len(text) - 1, len(text)):
        rows, nxt, status, _ = walk_all(upload(text[:cut]), cut, 3, final=False)
        assert status == ref.OK and nxt <= cut
        if cut < first:
            assert (rows, nxt) == ([], 0)
        else:
            assert rows == [w for w in want if w[0] + 4 <= cut and w[0] + 4 + int.from_bytes(text[w[0]:w[0] + 4], 'little') <= cut]
        more, nxt2, status, _ = walk_all(upload(text[nxt:]), len(text) - nxt, 1 << 16, at_header=cut < first)
        assert status == ref.OK and nxt + nxt2 == len(text)
        assert rows + [(w[0] + nxt,) + w[1:] for w in more] == want
    del torch


def test_walk_gives_malformed_text_its_status():
    for name, text, status, offset, n in bc.malformed_texts():
        rows = []
        with pytest.raises(ref.BamError):
            ref.walk(text, rows)
        for max_records in (1, 1 << 16):
            got, nxt, st, _ = walk_all(upload(text), len(text), max_records)
            assert (st, nxt) == (status, offset), name
            assert got == want_tuples(rows) and len(got) == n, name
        if status == ref.TRUNCATED:      # without final this is a tail to carry, not an error
            got, nxt, st, _ = walk_all(upload(text), len(text), 1 << 16, final=False)
            assert (st, nxt, len(got)) == (ref.OK, offset, n), name


@pytest.mark.parametrize('with_qual', [True, False])
def test_decode_equals_the_restatement(cases, with_qual):
    from megapath_nano_amd import ingest
    for name in ('main', 'no_quals', 'only_empty_reads', 'range.bam'):
        c = cases[name]
        kept = [r for r in c['rows'] if not r['flag'] & 0x900]
        rows = np.array([(r['off'], r['l_seq'], r['flag'], r['l_read_name'], r['has_qual']) for r in kept], dtype=ingest.BAM_ROW)
        seq, qual, names = ingest.bam_decode(upload(c['text']), len(c['text']), rows, with_qual)
        want = ref.Batch([(n, s, q if with_qual else None) for n, s, q in c['reads']])
        total = int(want.lens.sum())
        assert names == want.names, name
        assert seq.numel() == (total + 16 + 15) // 16 * 16
        got = seq.cpu().numpy()
        assert np.array_equal(got[:total + 16], want.buf) and not got[total:].any(), name
        if with_qual:
            got = qual.cpu().numpy()
            if want.qbuf is None:        # no read has qualities: the caller would not have asked; every read gets '!'
                assert (got[:total] == ord('!')).all() and not got[total:].any(), name
            else:
                assert np.array_equal(got[:total + 16], want.qbuf) and not got[total:].any(), name
        else:
            assert qual is None


def test_decode_refuses_rows_that_do_not_fit_the_text(cases):
    from megapath_nano_amd import _ffi, ingest
    c = cases['no_quals']
    text = upload(c['text'])
    rows = np.array([(r['off'], r['l_seq'], r['flag'], r['l_read_name'], r['has_qual']) for r in c['rows']], dtype=ingest.BAM_ROW)
    for field, value in (('off', len(c['text']) - 10), ('off', -1), ('l_seq', 100000), ('l_seq', -1), ('l_read_name', 0)):
        bad = rows.copy()
        bad[field][1] = value
        with pytest.raises(_ffi.MpnError, match='rc=-2'):
            ingest.bam_decode(text, len(c['text']), bad, True)
    assert ingest.bam_decode(text, len(c['text']), rows, False)[2] == [r[0] for r in c['reads']]


def test_flatten_joins_carry_and_slots():
    """slots at 16-byte aligned offsets with gaps, of lengths around the 16-byte vectors and the 1 KiB chunks, empty ones among them,
    behind a carry at every alignment"""
    import torch
    from megapath_nano_amd import ingest
    rng = np.random.default_rng(3)
    lens = np.array([0, 1, 15, 16, 17, 0, 1023, 1024, 1025, 65280, 3, 0, 40000, 31], dtype=np.int64)
    so = np.zeros(len(lens) + 1, dtype=np.int64)
    so[1:] = np.cumsum((lens + 15) & ~15)
    host = rng.integers(1, 256, size=int(so[-1]), dtype=np.uint8)
    slots = torch.from_numpy(host).cuda()
    prev = rng.integers(1, 256, size=5000, dtype=np.uint8)
    d_prev = torch.from_numpy(prev).cuda()
    for a, n in ((0, 0), (0, 16), (1, 1), (3, 37), (16, 2048), (4, 2049), (15, 4985), (7, 0)):
        carry = d_prev[a:a + n] if n else None
        text, total = ingest.bam_flatten(slots, so[:-1], lens, carry, 'cuda')
        want = np.concatenate([prev[a:a + n]] + [host[o:o + l] for o, l in zip(so[:-1], lens)])
        got = text.cpu().numpy()
        assert total == len(want) and len(got) == max((total + 15) // 16 * 16, 16)
        assert np.array_equal(got[:total], want) and not got[total:(total + 15) // 16 * 16].any(), (a, n)
    text, total = ingest.bam_flatten(slots, so[:0], lens[:0], d_prev[5:105], 'cuda')
    assert total == 100 and np.array_equal(text.cpu().numpy()[:100], prev[5:105])
    text, total = ingest.bam_flatten(slots, so[:0], lens[:0], None, 'cuda')
    assert total == 0


# ---- files ------------------------------------------------------------------------------------------------------------------------
def assert_batches(got, want, name):
    assert len(got) == len(want), (name, len(got), len(want))
    for g, w in zip(got, want):
        assert g.names == w.names, name
        assert g.n == len(w.names) and np.array_equal(g.lens, w.lens) and np.array_equal(g.off, w.off), name
        assert g.buf.dtype == np.uint8 and np.array_equal(g.buf, w.buf), name
        assert (g.qbuf is None) == (w.qbuf is None), name
        if w.qbuf is not None:
            assert np.array_equal(g.qbuf, w.qbuf), name
        d_buf, d_off, d_lens = g.dev
        assert np.array_equal(d_buf.cpu().numpy(), w.buf) and np.array_equal(d_off.cpu().numpy(), w.off) and np.array_equal(d_lens.cpu().numpy(), w.lens)
        assert d_buf.is_cuda and d_off.dtype.is_floating_point is False and str(d_lens.dtype) == 'torch.int32' and str(d_off.dtype) == 'torch.int64'


@pytest.mark.parametrize('name,group,walk,batch_bases', [
    ('main', None, None, 200_000_000),         # one group, one walk launch, one batch
    ('main', 1 << 17, 3, 5000),                # groups of 128 KiB: header and records span groups; the walk resumes; batches inside the file
    ('cuts', 1 << 17, 1, 200_000_000),         # block ends inside block_size, fixed fields, bases, at a record end; empty blocks
    ('cuts', None, None, 70_001),
    ('cuts', 1, 64, 1024),                     # a group per block
    ('no_eof', 1 << 17, 3, 4096),
    ('stored', 1 << 16, None, 64),
    ('no_quals', None, None, 200_000_000),     # no record has qualities: qbuf is None
    ('no_quals', None, 1, 21),
    ('header_only', None, None, 100),
    ('only_empty_reads', None, None, 100),
    ('bam2fq.001.bam', None, None, 200_000_000), ('range.bam', None, 3, 1000), ('colons.bam', None, None, 200_000_000),
])
def test_file_batches_equal_the_restatement(cases, monkeypatch, name, group, walk, batch_bases):
    from megapath_nano_amd import ingest
    if group is not None:
        monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', str(group))
    c = cases[name]
    timings = {}
    got = list(ingest.iter_bam_read_batches(c['path'], batch_bases, walk_records=walk, timings=timings))
    want = ref.batches(c['reads'], batch_bases)
    assert_batches(got, want, name)
    assert timings['records'] == len(c['rows'])
    if walk is not None and group is None:
        assert timings['walk_launches'] == len(c['rows']) // walk + 1
    if name == 'no_quals':
        assert all(b.qbuf is None for b in got)


def test_golden_files_give_the_golden_reads(cases):
    from megapath_nano_amd import fastx
    import test_bam_in_ref as cpu
    golden = json.load(open(os.path.join(GOLDEN, 'bam_reads', 'bam_reads_golden.json')))
    got = cpu.as_text(fastx.read_fastx(GOLDEN_FILES['bam2fq.001.bam'], with_qual=True))
    assert len(got) == 36 and cpu.multiset(got) == cpu.multiset(golden['bam2fq.001.bam']['split']) == cpu.multiset(golden['bam2fq.001.bam']['one_file'])
    for name in ('range.bam', 'colons.bam'):
        assert cpu.as_text(fastx.read_fastx(GOLDEN_FILES[name], with_qual=True)) == [tuple(r) for r in golden[name]['reads']]
    assert fastx.read_fastx(GOLDEN_FILES['colons.bam']) == [(n, s.encode()) for n, s, _ in golden['colons.bam']['reads']]


def test_a_fifo_is_read_once(cases, tmp_path):
    from megapath_nano_amd import aligner, fastx
    pipe = str(tmp_path / 'reads_pipe')
    os.mkfifo(pipe)
    blob = open(cases['no_eof']['path'], 'rb').read()

    def feed():
        with open(pipe, 'wb') as f:
            f.write(blob)
    writer = threading.Thread(target=feed, daemon=True)
    writer.start()
    got = list(aligner.iter_read_batches([pipe], 100_000))
    writer.join(30)
    assert fastx.is_fifo(pipe) and not writer.is_alive()
    assert_batches(got, ref.batches(cases['no_eof']['reads'], 100_000), 'fifo')


def test_malformed_files_are_refused(cases, tmp_path, monkeypatch):
    from megapath_nano_amd import ingest
    good = open(cases['stored']['path'], 'rb').read()
    main = open(cases['main']['path'], 'rb').read()
    second = ingest.bgzf_block_size(good[:18])
    seen = []

    def refused(name, blob, match):
        p = tmp_path / name
        p.write_bytes(blob)
        with pytest.raises(ValueError, match=match) as e:
            list(ingest.iter_bam_read_batches(str(p), 10_000))
        seen.append(str(e.value))
    # a stored block: the flipped payload bit inflates, and the CRC-32 the device computes tells
    refused('crc.bam', good[:second + 3000] + bytes([good[second + 3000] ^ 4]) + good[second + 3001:], f'block 1 at file offset {second}: BAD_CRC')
    refused('flipped.bam', main[:5000] + bytes([main[5000] ^ 0x20]) + main[5001:], 'BGZF block 0 at file offset 0: ')
    refused('cut_mid_block.bam', main[:len(main) // 2], 'ends inside the BGZF block at file offset')
    refused('cut_in_block_header.bam', good[:second + 7], f'ends inside the BGZF block at file offset {second}')
    refused('garbage_behind.bam', good[:second] + b'garbage that is no block', f'not a BGZF block at file offset {second}')
    refused('gzip_behind.bam', good[:second] + gzip.compress(b'plain gzip'), f'not a BGZF block at file offset {second}')
    refused('isize.bam', good[:second - 4] + (70000).to_bytes(4, 'little') + good[second:], 'ISIZE 70000')
    refused('isize_short.bam', good[:second - 4] + (100).to_bytes(4, 'little') + good[second:], 'block 0 at file offset 0: (OVERFLOW|BAD_SIZE)')
    refused('cut_at_block_end.bam', good[:second], 'BAM_TRUNCATED')      # whole blocks, but the text ends inside the header
    refused('no_blocks.bam', bc.EOF_BLOCK, 'offset 0 of the inflated stream: BAM_TRUNCATED')
    names = ('OK', 'TRUNCATED', 'BAD_MAGIC', 'BAD_BLOCK', 'BAD_CODE', 'BAD_DISTANCE', 'BAD_CRC', 'BAD_SIZE', 'OVERFLOW', 'UNSUPPORTED',
             'BAM_TRUNCATED', 'BAM_BAD_MAGIC', 'BAM_BAD_HEADER', 'BAM_BAD_RECORD')
    assert ingest.STATUS_NAMES == names
    for group in (None, 64):
        if group:
            monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', str(group))
        for name, text, status, offset, _ in bc.malformed_texts():
            refused(f'{name}.bam', bc.bgzf(text, cuts=range(0, len(text), 50) if group else ()), f'offset {offset} of the inflated stream: {names[status]}$')


# ---- end to end -------------------------------------------------------------------------------------------------------------------
class FakeMetadata:
    """The joins Align() uses, over an in-memory table (as in test_align_mirror_gpu.py)."""

    def __init__(self, table):
        self.t = table

    def get_assembly_path(self, *, assembly_list, how='inner'):
        return assembly_list.merge(self.t[['assembly_id', 'path']].drop_duplicates(), on='assembly_id', how=how)

    def get_assembly_length(self, *, assembly_list, how='inner'):
        return assembly_list.merge(self.t[['assembly_id', 'assembly_length']].drop_duplicates(), on='assembly_id', how=how)

    def get_sequence_tax_id(self, *, assembly_list, how='inner'):
        return assembly_list.merge(self.t[['assembly_id', 'tax_id', 'species_tax_id', 'genus_tax_id', 'sequence_id']], on='assembly_id', how=how)


def bam_of(reads, rng):
    """reads: [(name, bases, Phred+33)] -> BAM file bytes; every other read is stored as its reverse complement with flag 0x10, and
    a secondary and a supplementary record stand between them"""
    recs = []
    for k, (name, seq, qual) in enumerate(reads):
        phred = bytes(q - 33 for q in qual)
        if k % 2:
            recs.append(bc.record(name, seq[::-1].translate(ref.COMPLEMENT).decode(), phred[::-1], flag=0x10 | 0x4))
        else:
            recs.append(bc.record(name, seq.decode(), phred, flag=0x4, tags=b'qsf\0\0\0\x41'))
        if k % 7 == 3:
            recs.append(bc.record(name, 'ACGTACGT', bytes(8), flag=0x100 if k % 2 else 0x800))
    text = bc.header(b'@HD\tVN:1.6\tSO:unknown\n', ()) + b''.join(recs)
    return bc.bgzf(text, cuts=sorted(int(x) for x in rng.integers(1, len(text), size=6)), max_block=20000)


@pytest.fixture(scope='module')
def world(tmp_path_factory, libmpn):
    """Three genomes as assemblies; 24 reads as FASTQ in one directory and as BAM in another, under the same basename (Align() seeds
    its tie-breaker with the md5 of the basenames); the same reads again as two halves."""
    from megapath_nano_amd import synth
    d = tmp_path_factory.mktemp('bam_e2e')
    rng = np.random.default_rng(8)
    gen = synth.make_genomes(31, 3, 40000, strain_pairs=1)
    reads = [(r['name'], bytes(r['seq']), bytes(rng.integers(33, 127, size=len(r['seq'])).astype(np.uint8)))
             for r in synth.make_reads(32, gen, 24, mean_len=2000)]
    rows = []
    for i, (name, seq) in enumerate(gen):
        p = d / f'asm{i}.fna.gz'
        p.write_bytes(gzip.compress(b'>' + name.encode() + b'\n' + bytes(seq) + b'\n', 6))
        rows.append(dict(assembly_id=f'GCF_{i:09d}.1', path=p.name, assembly_length=len(seq), tax_id=1000 + i, species_tax_id=500 + i,
                         genus_tax_id=50, sequence_id=name))
    (d / 'fq').mkdir()
    (d / 'bam').mkdir()
    for base, part in (('reads', reads), ('half1', reads[:11]), ('half2', reads[11:])):
        (d / 'fq' / base).write_bytes(ref.fastq_text(part))
        (d / 'bam' / base).write_bytes(bam_of(part, rng))
    return dict(dir=d, table=pd.DataFrame(rows), targets=[str(d / f'asm{i}.fna.gz') for i in range(3)], reads=reads)


def test_read_fastx_gives_the_tuples_of_the_fastq(world):
    from megapath_nano_amd import fastx
    want = fastx.read_fastx(str(world['dir'] / 'fq' / 'reads'), with_qual=True)
    assert want == world['reads'] and len(want) == 24
    assert fastx.read_fastx(str(world['dir'] / 'bam' / 'reads'), with_qual=True) == want
    assert fastx.read_fastx(str(world['dir'] / 'bam' / 'reads')) == [(n, s) for n, s, _ in want]


def map_text(world, queries, **kw):
    from megapath_nano_amd import aligner
    options = aligner.AlignerOptions(['-x', 'map-ont'], False)
    got, header = aligner.map_files(world['targets'], [str(world['dir'] / q) for q in queries], options, want_paf=True, want_sam=True, **kw)
    return ''.join(b.paf for b in got), header + ''.join(b.sam for b in got)


def test_map_files_gives_the_same_paf_and_sam(world):
    paf, sam = map_text(world, ['fq/reads'])
    assert paf.count('\n') >= 20 and sam.count('\n') >= 24
    assert map_text(world, ['bam/reads']) == (paf, sam)
    assert map_text(world, ['bam/reads'], read_batch_bases=9000) == map_text(world, ['fq/reads'], read_batch_bases=9000)


def test_a_mixed_query_list_equals_the_concatenated_fastq(world):
    want = map_text(world, ['fq/half1', 'fq/half2'])
    assert want == map_text(world, ['fq/reads'])
    assert map_text(world, ['fq/half1', 'bam/half2']) == want
    assert map_text(world, ['bam/half1', 'fq/half2']) == want
    assert map_text(world, ['bam/half1', 'bam/half2']) == want


def run_align(world, kind, prefix):
    from megapath_nano_amd import aligner
    return aligner.Align(assembly_metadata=FakeMetadata(world['table']),
                         global_options=dict(assembly_folder=str(world['dir']), min_alignment_score=0, debug=False),
                         temp_dir_name=str(world['dir']), log_file=None, query_filename_list=pd.DataFrame({'path': [str(world['dir'] / kind / 'reads')]}),
                         target_assembly_list=world['table'][['assembly_id']].drop_duplicates().copy(),
                         aligner_options=['-t', '4', '-N', '50', '-p', '1', '-x', 'map-ont'], paf_path_and_prefix=str(world['dir'] / prefix))


def test_align_gives_the_same_table(world):
    a = run_align(world, 'fq', 'from_fq')
    b = run_align(world, 'bam', 'from_bam')
    assert len(a) > 0 and a.equals(b)
    assert (world['dir'] / 'from_fq.paf').read_bytes() == (world['dir'] / 'from_bam.paf').read_bytes() != b''


def test_a_bam_target_is_refused(world):
    from megapath_nano_amd import aligner
    options = aligner.AlignerOptions(['-x', 'map-ont'], True)
    with pytest.raises(ValueError, match='read input only'):
        aligner.map_files([str(world['dir'] / 'bam' / 'reads')], [str(world['dir'] / 'fq' / 'reads')], options)
