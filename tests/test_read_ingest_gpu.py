"""GPU tests (-m gpu) of FASTQ read input on the device (MPN_READ_INGEST=device; ingest.iter_fastq_read_batches behind
aligner.iter_read_batches): the batches against those of the host loop, batch for batch, for plain, gzip and BGZF files, from a
regular file and from a FIFO, with chunks and groups small enough that records straddle them; then one mapping end to end."""
import gzip
import os
import threading

import numpy as np
import pytest

import fastq_scan_ref as ref
from megapath_nano_amd import bam

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_BAM = os.path.join(ROOT, 'tests', 'golden', 'bam_reads', 'bam2fq.001.bam')
BATCH_BASES = 20000
FORMS = ('plain', 'gzip', 'bgzf')


def bgzf(text, block=5000):
    """blocks of `block` bytes of text (cut wherever that falls in a record) and the empty block htslib ends a file with"""
    return b''.join(bam._bgzf_block(text[a:a + block], 6) for a in range(0, len(text), block)) + bam._bgzf_block(b'', 6)


def in_form(text, form):
    return {'plain': text, 'gzip': gzip.compress(text, 6), 'bgzf': bgzf(text)}[form]


def _reads(seed, n, lo, hi):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        k = int(rng.integers(lo, hi))
        out.append((b'r%d_%d comment %d' % (seed, i, k), ref._bases(k, seed + i), ref._quals(k, seed + i)))
    return out


def four_line(reads):
    return b''.join(ref.rec(n, s, q) for n, s, q in reads)


def multi_line(reads, width=61):
    out = []
    for n, s, q in reads:
        out.append(b'@' + n + b'\n' + b''.join(s[a:a + width] + b'\n' for a in range(0, len(s), width)) + b'+\n' +
                   b''.join(q[a:a + width] + b'\n' for a in range(0, len(q), width)))
    return b''.join(out)


@pytest.fixture(scope='module')
def files(tmp_path_factory, libmpn):
    """The texts of the query list: a four-line FASTQ, a multi-line FASTQ, a FASTA whose first read is longer than a batch (the host
    loop then starts a batch at it, where the device mode flushes before a file that goes to the host from its first byte), a BAM,
    and a FASTQ that turns multi-line halfway."""
    d = tmp_path_factory.mktemp('read_ingest')
    texts = {
        'four': four_line(_reads(1, 40, 50, 3000)),
        'multi': multi_line(_reads(2, 12, 100, 2500)),
        'fasta': b'>long one\n' + ref._bases(BATCH_BASES + 5000) + b'\n' + b''.join(b'>f%d\n' % i + ref._bases(700 + i) + b'\n' for i in range(6)),
        'halfway': four_line(_reads(3, 14, 50, 2500)) + multi_line(_reads(4, 5, 200, 900)) + four_line(_reads(5, 6, 50, 2000)),
    }
    for name, text in texts.items():
        for form in FORMS:
            (d / f'{name}.{form}').write_bytes(in_form(text, form))
    return dict(dir=d, texts=texts)


@pytest.fixture(autouse=True)
def small_chunks(monkeypatch):
    monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', '8192')
    monkeypatch.delenv('MPN_READ_INGEST', raising=False)


class Fifos:
    """FIFOs that a thread each fills with a file's bytes"""

    def __init__(self, d):
        self.dir, self.threads, self.n = d, [], 0

    def of(self, path):
        self.n += 1
        fifo = str(self.dir / f'fifo{self.n}')
        os.mkfifo(fifo)
        data = open(path, 'rb').read()

        def fill():
            with open(fifo, 'wb') as f:
                f.write(data)
        t = threading.Thread(target=fill, daemon=True)
        t.start()
        self.threads.append(t)
        return fifo

    def join(self):
        for t in self.threads:
            t.join(30)
            assert not t.is_alive()


def batches(paths, mode, monkeypatch, batch_bases=BATCH_BASES):
    from megapath_nano_amd import aligner
    monkeypatch.setenv('MPN_READ_INGEST', mode)
    out = []
    for b in aligner.iter_read_batches(paths, batch_bases, device='cuda'):
        dev = tuple(t.cpu().numpy() for t in b.dev)
        out.append(dict(names=list(b.names), lens=b.lens, off=b.off, buf=b.buf, qbuf=b.qbuf, dev=dev))
    return out


def assert_same_batches(got, want):
    assert [len(b['names']) for b in got] == [len(b['names']) for b in want]
    for g, w in zip(got, want):
        assert g['names'] == w['names']
        for key in ('lens', 'off', 'buf', 'qbuf'):
            assert (g[key] is None) == (w[key] is None), key
            if w[key] is not None:
                assert g[key].dtype == w[key].dtype and np.array_equal(g[key], w[key]), key
        # the device copy of either mode is the host copy
        for b in (g, w):
            assert np.array_equal(b['dev'][0], b['buf']) and np.array_equal(b['dev'][1], b['off']) and np.array_equal(b['dev'][2], b['lens'])


@pytest.mark.parametrize('source', ['file', 'fifo'])
@pytest.mark.parametrize('form', FORMS)
def test_batches_equal_the_host_loop(files, tmp_path, monkeypatch, form, source):
    d = files['dir']
    fifos = Fifos(tmp_path)

    def query_list():
        src = (lambda p: fifos.of(p)) if source == 'fifo' else (lambda p: p)
        return [src(str(d / f'four.{form}')), str(d / 'multi.plain'), str(d / 'fasta.plain'), GOLDEN_BAM, src(str(d / f'halfway.{form}'))]
    want = batches(query_list(), 'host', monkeypatch)
    got = batches(query_list(), 'device', monkeypatch)
    fifos.join()
    assert_same_batches(got, want)
    n_fq = len(ref.host_records(files['texts']['four'])) + len(ref.host_records(files['texts']['multi']))
    assert len(want) >= 7 and sum(len(b['names']) for b in want) > n_fq + 7 + len(ref.host_records(files['texts']['halfway']))
    # batches span files: one holds the last reads of the first file and the reads of the second
    assert any('r1_39' in b['names'] and 'r2_0' in b['names'] for b in got)


def test_the_device_took_the_plain_records(files, monkeypatch):
    """the same batches could come from a path that hands everything to the host: the timings say which records the scan took"""
    from megapath_nano_amd import fastx, ingest
    for name, on_device, on_host in (('four', 40, 0), ('multi', 0, 12), ('halfway', 14, 11)):
        for form in FORMS:
            t = {}
            kind, stream, first = fastx.open_query(str(files['dir'] / f'{name}.{form}'))
            assert (kind, first) == (form, b'@')
            with stream:
                got = list(ingest.iter_fastq_read_batches(stream, BATCH_BASES, 'cuda', t, form=kind))
            assert (t.get('records', 0), t.get('host_records', 0)) == (on_device, on_host), (name, form)
            recs = [(b.names[i], b.buf[b.off[i]:b.off[i] + b.lens[i]].tobytes(), b.qbuf[b.off[i]:b.off[i] + b.lens[i]].tobytes())
                    for b in got for i in range(b.n)]
            assert recs == ref.host_records(files['texts'][name])


def test_fasta_and_empty_files_take_the_host_path(files, tmp_path, monkeypatch):
    (tmp_path / 'empty').write_bytes(b'')
    (tmp_path / 'empty.gz').write_bytes(gzip.compress(b''))
    paths = [str(tmp_path / 'empty'), str(files['dir'] / 'fasta.gzip'), str(tmp_path / 'empty.gz'), str(files['dir'] / 'fasta.bgzf')]
    want = batches(paths, 'host', monkeypatch, batch_bases=1 << 30)
    got = batches(paths, 'device', monkeypatch, batch_bases=1 << 30)
    # a flush before every file that goes to the host: one batch per file that has reads, the same reads as the host's one batch
    assert [len(b['names']) for b in got] == [7, 7] and [len(b['names']) for b in want] == [14]
    assert [n for b in got for n in b['names']] == want[0]['names'] and all(b['qbuf'] is None for b in got + want)


def test_a_damaged_bgzf_block_names_the_block_and_its_offset(files, tmp_path, monkeypatch):
    blob = bytearray((files['dir'] / 'four.bgzf').read_bytes())
    sizes, p = [], 0
    while p < len(blob):
        sizes.append(int.from_bytes(blob[p + 16:p + 18], 'little') + 1)
        p += sizes[-1]
    where = sum(sizes[:3])
    blob[where + 18 + 40] ^= 0x10                 # inside the deflate data of block 3
    (tmp_path / 'damaged.fq.gz').write_bytes(bytes(blob))
    monkeypatch.setenv('MPN_READ_INGEST', 'device')
    from megapath_nano_amd import aligner
    with pytest.raises(ValueError, match=rf'BGZF block 3 at file offset {where}: \w+'):
        list(aligner.iter_read_batches([str(tmp_path / 'damaged.fq.gz')], BATCH_BASES, device='cuda'))


def test_map_files_gives_the_same_paf(tmp_path, monkeypatch, libmpn):
    from megapath_nano_amd import aligner, synth
    monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', '65536')
    rng = np.random.default_rng(5)
    gen = synth.make_genomes(41, 3, 40000, strain_pairs=1)
    reads = [(r['name'].encode(), bytes(r['seq']), bytes(rng.integers(33, 127, size=len(r['seq'])).astype(np.uint8)))
             for r in synth.make_reads(42, gen, 24, mean_len=2000)]
    targets = []
    for i, (name, seq) in enumerate(gen):
        targets.append(str(tmp_path / f'asm{i}.fna.gz'))
        open(targets[-1], 'wb').write(gzip.compress(b'>' + name.encode() + b'\n' + bytes(seq) + b'\n', 6))
    queries = []
    for form, part in zip(FORMS, (reads[:9], reads[9:17], reads[17:])):
        queries.append(str(tmp_path / f'reads.{form}'))
        open(queries[-1], 'wb').write(in_form(four_line(part), form))
    options = aligner.AlignerOptions(['-x', 'map-ont'], False)

    def paf(mode):
        monkeypatch.setenv('MPN_READ_INGEST', mode)
        got, _ = aligner.map_files(targets, queries, options, want_paf=True, read_batch_bases=15000)
        return ''.join(b.paf for b in got)
    want = paf('host')
    assert want.count('\n') >= 20
    assert paf('device') == want
