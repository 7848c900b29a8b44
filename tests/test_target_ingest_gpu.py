"""GPU tests (-m gpu) of MPN_TARGET_INGEST=device (megapath_nano_amd/ingest.py): target files go from compressed bytes to index parts
on the GPU.  The host path (fastx + aligner.iter_target_parts + mapper.Index) is the reference: same parts, same indexes, same
Align() output; the fallbacks (corrupted file, FIFO, oversized stream, FASTQ-like file) end where the host path ends."""
import gzip
import os
import threading
import zlib

import numpy as np
import pandas as pd
import pytest

from megapath_nano_amd import aligner, fastx

pytestmark = pytest.mark.gpu
MINI, BATCH = 30_000, 70_000          # a mini-batch per 40-kb genome, a part closes after two of them: three parts


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


def fasta(records, eol=b'\n', width=80):
    out = b''
    for name, seq in records:
        seq = bytes(seq)
        out += b'>' + name.encode() + b' a description' + eol + b''.join(seq[a:a + width] + eol for a in range(0, len(seq), width))
    return out


@pytest.fixture(scope='module')
def world(tmp_path_factory, libmpn):
    """Six genomes of 40 kb, two contigs each: four single-member .fna.gz (one with CRLF), one .fna.gz of two members (a contig
    each) and one plain .fna."""
    from megapath_nano_amd import synth
    d = tmp_path_factory.mktemp('ingest')
    gen = synth.make_genomes(21, 6, 40000, strain_pairs=1)
    reads = synth.make_reads(22, gen, 24, mean_len=2000)
    rows, paths = [], []
    for i, (name, seq) in enumerate(gen):
        contigs = [(f'{name}.c1', seq[:25000]), (f'{name}.c2', seq[25000:])]
        if i == 2:
            p, data = d / f'asm{i}.fna.gz', gzip.compress(fasta(contigs[:1])) + gzip.compress(fasta(contigs[1:]))
        elif i == 3:
            p, data = d / f'asm{i}.fna', fasta(contigs)
        elif i == 4:
            p, data = d / f'asm{i}.fna.gz', gzip.compress(fasta(contigs, eol=b'\r\n'), 6)
        else:
            p, data = d / f'asm{i}.fna.gz', gzip.compress(fasta(contigs), 6)
        p.write_bytes(data)
        paths.append(str(p))
        for cname, cseq in contigs:
            rows.append(dict(assembly_id=f'GCF_{i:09d}.1', path=p.name, assembly_length=len(seq), tax_id=1000 + i, species_tax_id=500 + i,
                             genus_tax_id=50, sequence_id=cname))
    fq = d / 'reads.fq'
    with open(fq, 'wb') as f:
        for r in reads:
            f.write(b'@' + r['name'].encode() + b'\n' + bytes(r['seq']) + b'\n+\n' + b'I' * len(r['seq']) + b'\n')
    return dict(dir=d, paths=paths, table=pd.DataFrame(rows), fq=str(fq), read_genome={r['name']: int(r['genome']) for r in reads})


@pytest.fixture(autouse=True)
def small_parts(monkeypatch):
    monkeypatch.setattr(aligner, 'IDX_MINI_BATCH', MINI)       # what MPN_IDX_MINI_BATCH sets when the module is imported
    monkeypatch.delenv('MPN_TARGET_INGEST', raising=False)
    monkeypatch.delenv('MPN_INGEST_MAX_STREAM', raising=False)
    monkeypatch.delenv('MPN_INGEST_BATCH_BYTES', raising=False)


def host_parts(paths):
    from megapath_nano_amd import mapper
    out = []
    for part in aligner.iter_target_parts(aligner.iter_target_records(paths), BATCH):
        idx = mapper.Index(part, k=15, w=10)
        out.append((list(idx.names), idx.lens.tolist(), idx.export()))
        idx.close()
    return out


def device_parts(paths):
    from megapath_nano_amd import ingest
    out = []
    for idx in ingest.iter_target_parts_device(paths, BATCH, k=15, w=10):
        out.append((list(idx.names), idx.lens.tolist(), idx.export()))
        idx.close()
    return out


def assert_same_parts(got, want):
    assert [(n, l) for n, l, _ in got] == [(n, l) for n, l, _ in want]
    for (_, _, a), (_, _, b) in zip(got, want):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_device_parts_equal_host_parts(world):
    want = host_parts(world['paths'])
    assert [len(n) for n, _, _ in want] == [4, 4, 4]
    assert_same_parts(device_parts(world['paths']), want)


def test_groups_of_one_file_give_the_same_parts(world, monkeypatch):
    """MPN_INGEST_BATCH_BYTES below every file: each is a group of its own, a part's bases arrive from two groups"""
    monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', '1000')
    assert_same_parts(device_parts(world['paths']), host_parts(world['paths']))


def test_oversized_streams_go_through_zlib(world, monkeypatch):
    from megapath_nano_amd import ingest
    monkeypatch.setenv('MPN_INGEST_MAX_STREAM', '1000')
    seen = []
    monkeypatch.setattr(ingest, 'inflate_files', lambda *a, _f=ingest.inflate_files, **k: (lambda r: (seen.append(r.on_host), r)[1])(_f(*a, **k)))
    assert_same_parts(device_parts(world['paths']), host_parts(world['paths']))
    assert seen and all(len(s) > 0 for s in seen)


def test_files_the_scan_cannot_take_fall_back(world, tmp_path):
    """a FASTQ file and a file with blanks inside its sequence lines among the targets: read through the host path, in place"""
    fq_like = tmp_path / 'reads_as_target.fq.gz'
    fq_like.write_bytes(gzip.compress(b'@r1\nACGTACGTACGTACGTAAAACCCCGGGGTTTT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n'))
    spaced = tmp_path / 'spaced.fna'
    spaced.write_bytes(b'>spaced\nACGT ACGT\n  GGGGCCCCAAAATTTTACGTACGTACGT  \n')
    paths = world['paths'][:2] + [str(fq_like)] + world['paths'][2:4] + [str(spaced)] + world['paths'][4:]
    want = host_parts(paths)
    assert any('r1' in n for n, _, _ in want) and any('spaced' in n for n, _, _ in want)
    assert_same_parts(device_parts(paths), want)


def run_align(world, prefix):
    return aligner.Align(assembly_metadata=FakeMetadata(world['table']),
                         global_options=dict(assembly_folder=str(world['dir']), min_alignment_score=0, debug=False),
                         temp_dir_name=str(world['dir']), log_file=None, query_filename_list=pd.DataFrame({'path': [world['fq']]}),
                         target_assembly_list=world['table'][['assembly_id']].drop_duplicates().copy(),
                         aligner_options=['-t', '4', '-N', '50', '-p', '1', '-x', 'map-ont', '-I', str(BATCH), '--split-prefix', 'tmp'],
                         paf_path_and_prefix=str(world['dir'] / prefix))


def test_align_gives_the_same_table_and_paf(world, monkeypatch):
    from megapath_nano_amd import ingest
    a = run_align(world, 'host')
    calls = []
    monkeypatch.setattr(ingest, 'iter_target_parts_device',
                        lambda *x, _f=ingest.iter_target_parts_device, **k: (calls.append(1), _f(*x, **k))[1])
    monkeypatch.setenv('MPN_TARGET_INGEST', 'device')
    b = run_align(world, 'device')
    assert calls and len(a) > 0 and a.equals(b)
    assert (world['dir'] / 'host.paf').read_bytes() == (world['dir'] / 'device.paf').read_bytes()
    monkeypatch.setenv('MPN_TARGET_INGEST', 'host')
    calls.clear()
    assert run_align(world, 'host2').equals(a) and not calls


def test_unknown_knob_value_raises(world, monkeypatch):
    monkeypatch.setenv('MPN_TARGET_INGEST', 'gpu')
    with pytest.raises(ValueError):
        run_align(world, 'bad')


def test_corrupted_file_raises_what_the_host_path_raises(world, tmp_path, monkeypatch):
    """The device path must have run, the decoder must have given the damaged stream a status of its own, and the re-read through
    fastx that follows from it must be what raises: the same exception the host path raises."""
    from megapath_nano_amd import ingest
    TRUNCATED, BAD_BLOCK, BAD_CODE, BAD_DISTANCE, BAD_CRC, BAD_SIZE = 1, 3, 4, 5, 6, 7
    good = open(world['paths'][0], 'rb').read()
    options = aligner.AlignerOptions(['-x', 'map-ont', '-I', str(BATCH)], True)
    part_calls, statuses, rereads = [], [], []
    monkeypatch.setattr(ingest, 'iter_target_parts_device',
                        lambda *x, _f=ingest.iter_target_parts_device, **k: (part_calls.append(list(x[0])), _f(*x, **k))[1])
    monkeypatch.setattr(ingest, 'inflate_files',
                        lambda *x, _f=ingest.inflate_files, **k: (lambda r: (statuses.append(r.status.tolist()), r)[1])(_f(*x, **k)))
    monkeypatch.setattr(ingest, '_host_records', lambda path, _f=ingest._host_records: (rereads.append(path), _f(path))[1])
    mid = len(good) // 2
    for name, data, allowed in (('flipped.fna.gz', good[:mid] + bytes([good[mid] ^ 0x10]) + good[mid + 1:],
                                 {BAD_CRC, BAD_CODE, BAD_DISTANCE, BAD_BLOCK, BAD_SIZE, TRUNCATED}),
                                ('cut.fna.gz', good[:mid], {TRUNCATED}),
                                ('crc.fna.gz', good[:-5] + bytes([good[-5] ^ 1]) + good[-4:], {BAD_CRC})):
        p = tmp_path / name
        p.write_bytes(data)
        paths = [world['paths'][1], str(p)]
        monkeypatch.delenv('MPN_TARGET_INGEST', raising=False)
        del part_calls[:], statuses[:], rereads[:]
        with pytest.raises((zlib.error, gzip.BadGzipFile, EOFError)) as host:
            aligner.map_files(paths, [world['fq']], options)
        assert not part_calls and not statuses
        monkeypatch.setenv('MPN_TARGET_INGEST', 'device')
        with pytest.raises(host.type):
            aligner.map_files(paths, [world['fq']], options)
        assert part_calls == [paths] and len(statuses) == 1
        assert statuses[0][0] == 0 and statuses[0][1] in allowed, (name, statuses)
        assert rereads == [str(p)]


def test_fifo_target_stays_on_the_host_path(world, tmp_path, monkeypatch):
    from megapath_nano_amd import ingest
    options = aligner.AlignerOptions(['-x', 'map-ont', '-I', str(BATCH), '--split-prefix', 'tmp'], True)
    gz_files = [p for p in world['paths'] if p.endswith('.gz')]
    want, _ = aligner.map_files(gz_files, [world['fq']], options, want_paf=True)
    pipe = str(tmp_path / 'temp_pipe_target_fasta')
    os.mkfifo(pipe)

    def feed():
        with open(pipe, 'wb') as f:
            for p in gz_files:
                f.write(open(p, 'rb').read())
    writer = threading.Thread(target=feed, daemon=True)
    writer.start()
    monkeypatch.setenv('MPN_TARGET_INGEST', 'device')
    monkeypatch.setattr(ingest, 'iter_target_parts_device', lambda *a, **k: pytest.fail('a FIFO went to the device path'))
    assert not aligner.target_ingest_on_device([pipe]) and fastx.is_fifo(pipe)
    got, _ = aligner.map_files([pipe], [world['fq']], options, want_paf=True)
    writer.join(30)
    assert ''.join(b.paf for b in got) == ''.join(b.paf for b in want) != ''


def test_placement_to_assembly_gives_the_same_table(world, monkeypatch):
    """two species of three assemblies each: the first was aligned against already, the other two are the candidates whose files
    placement_to_assembly ingests per species"""
    from megapath_nano_amd import ingest, placement
    table = world['table'].copy()
    table['species_tax_id'] = 500 + table['assembly_id'].str.slice(4, 13).astype(int) // 3

    class Metadata(FakeMetadata):
        def get_tax_id(self, *, assembly_list, how='inner'):
            return assembly_list[['assembly_id']].merge(self.t[['assembly_id', 'tax_id', 'species_tax_id', 'genus_tax_id']].drop_duplicates(),
                                                        on='assembly_id', how=how)

        def get_sequence_tax_id(self, *, assembly_list, how='inner'):     # (the candidates arrive with their taxonomy columns)
            return super().get_sequence_tax_id(assembly_list=assembly_list[['assembly_id']], how=how)

        def get_assembly_path(self, *, assembly_list, how='inner'):
            return super().get_assembly_path(assembly_list=assembly_list[['assembly_id']], how=how)

        def get_assembly_length(self, *, assembly_list, how='inner'):
            return super().get_assembly_length(assembly_list=assembly_list[['assembly_id']], how=how)
    # every read goes to the species of the genome it was drawn from
    placed = pd.DataFrame({'read_id': list(world['read_genome']), 'species_tax_id': [500 + g // 3 for g in world['read_genome'].values()]})
    ids = table[['assembly_id']].drop_duplicates().reset_index(drop=True)
    kw = dict(assembly_metadata=Metadata(table), target_assembly_list=ids, species_id_assembly_id=ids.iloc[[0, 3]].reset_index(drop=True),
              species_list=pd.DataFrame({'species_tax_id': [501, 500]}), read_id_species_id=placed,
              query_filename_list=pd.DataFrame({'path': [world['fq']]}),
              global_options=dict(assembly_folder=str(world['dir']), min_alignment_score=0, debug=False, alignerThreadOption='-t 4', mapping_only=False))
    want, n_want = placement.placement_to_assembly(**kw)
    calls = []
    monkeypatch.setattr(ingest, 'iter_target_parts_device',
                        lambda *x, _f=ingest.iter_target_parts_device, **k: (calls.append(list(x[0])), _f(*x, **k))[1])
    monkeypatch.setenv('MPN_TARGET_INGEST', 'device')
    got, n_got = placement.placement_to_assembly(**kw)
    assert len(calls) == 2 and all(len(paths) == 2 for paths in calls)
    assert n_got == n_want == 4 and len(want) > 0
    pd.testing.assert_frame_equal(got, want, check_exact=True)
