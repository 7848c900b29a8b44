"""GPU tests (-m gpu) of Align() under MPN_BAM_WRITER=device: every batch's SAM text goes to bam.DeviceBamBuilder, the table is the
default's, <prefix>.bam and .bam.bai are those of an MPN_BGZF=device run byte for byte, and the mapper's own SAM -- with
--cs --MD --eqx and SA:Z as well -- is never refused."""
import gzip

import pandas as pd
import pytest

from megapath_nano_amd import bam

pytestmark = pytest.mark.gpu


class FakeMetadata:
    """The joins Align() uses, over an in-memory table (as in test_bam_device_gpu.py)."""

    def __init__(self, table):
        self.t = table

    def get_assembly_path(self, *, assembly_list, how='inner'):
        return assembly_list.merge(self.t[['assembly_id', 'path']].drop_duplicates(), on='assembly_id', how=how)

    def get_assembly_length(self, *, assembly_list, how='inner'):
        return assembly_list.merge(self.t[['assembly_id', 'assembly_length']].drop_duplicates(), on='assembly_id', how=how)

    def get_sequence_tax_id(self, *, assembly_list, how='inner'):
        return assembly_list.merge(self.t[['assembly_id', 'tax_id', 'species_tax_id', 'genus_tax_id', 'sequence_id']],
                                   on='assembly_id', how=how)


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    from map_cases import small_world
    d = tmp_path_factory.mktemp('align_bam_writer')
    gen, reads = small_world(seed=11, n_genomes=3, glen=60000, n_reads=15, mean_len=2000)
    rows = []
    for i, (name, seq) in enumerate(gen):
        p = d / f'asm{i}.fna.gz'
        with gzip.open(p, 'wb') as f:
            f.write(b'>' + name.encode() + b'\n' + bytes(seq) + b'\n')
        rows.append(dict(assembly_id=f'GCF_{i:09d}.1', path=p.name, assembly_length=len(seq), tax_id=1000 + i,
                         species_tax_id=500 + i, genus_tax_id=50, sequence_id=name))
    fq = d / 'reads.fq'
    with open(fq, 'wb') as f:
        for r in reads:
            f.write(b'@' + r['name'].encode() + b'\n' + bytes(r['seq']) + b'\n+\n' + b'I' * len(r['seq']) + b'\n')
    return d, pd.DataFrame(rows), fq


def run(world, prefix, extra=()):
    from megapath_nano_amd.aligner import Align
    d, table, fq = world
    return Align(assembly_metadata=FakeMetadata(table), global_options=dict(assembly_folder=str(d), min_alignment_score=0, debug=False),
                 temp_dir_name=str(d), log_file=None, query_filename_list=pd.DataFrame({'path': [str(fq)]}),
                 target_assembly_list=table[['assembly_id']].copy(), aligner_options=['-t', '4', '-N', '50', '-p', '1', '-x', 'map-ont', *extra],
                 paf_path_and_prefix=str(d / prefix))


@pytest.mark.parametrize('extra', [(), ('--cs', '--MD', '--eqx')], ids=['plain', 'cs_md_eqx'])
def test_device_writer_writes_the_files_of_the_device_bgzf_run(world, libmpn, oracle_built, monkeypatch, extra):
    d = world[0]
    tag = 'tags' if extra else 'plain'
    monkeypatch.delenv('MPN_BGZF', raising=False)
    monkeypatch.delenv('MPN_BAM_WRITER', raising=False)
    a = run(world, f'default_{tag}', extra)
    monkeypatch.setenv('MPN_BGZF', 'device')
    b = run(world, f'bgzf_{tag}', extra)
    monkeypatch.delenv('MPN_BGZF', raising=False)
    finished, refused = [], []
    monkeypatch.setattr(bam.DeviceBamBuilder, 'finish', lambda self, path, index=True, _f=bam.DeviceBamBuilder.finish: (finished.append(path), _f(self, path, index))[1])
    monkeypatch.setattr(bam.DeviceRefused, '__init__', lambda self, *args, _f=bam.DeviceRefused.__init__: (refused.append(args), _f(self, *args))[1])
    monkeypatch.setenv('MPN_BAM_WRITER', 'device')
    c = run(world, f'writer_{tag}', extra)
    assert a.equals(b) and a.equals(c)
    assert finished == [str(d / f'writer_{tag}.bam')] and refused == []
    sam = open(d / f'writer_{tag}.sam').read()
    assert sam == open(d / f'default_{tag}.sam').read() and sam.count('\n') > 10
    if extra:
        assert 'cs:Z:' in sam and 'MD:Z:' in sam
    for ext in ('.bam', '.bam.bai'):
        got, want = open(d / f'writer_{tag}{ext}', 'rb').read(), open(d / f'bgzf_{tag}{ext}', 'rb').read()
        assert len(want) > 100 and got == want, ext


def test_refusal_falls_back_to_the_host_writer(world, libmpn, oracle_built, monkeypatch, capsys):
    d = world[0]
    monkeypatch.delenv('MPN_BGZF', raising=False)
    monkeypatch.setenv('MPN_BAM_WRITER', 'device')

    def refuse(self, data):
        raise bam.DeviceRefused(7, 14, 'unknown tag type')
    monkeypatch.setattr(bam.DeviceBamBuilder, 'add_text', refuse)
    run(world, 'fallback')
    assert 'the host writer takes over' in capsys.readouterr().err
    monkeypatch.undo()
    monkeypatch.setenv('MPN_BGZF', 'device')
    monkeypatch.delenv('MPN_BAM_WRITER', raising=False)
    run(world, 'fallback_ref')
    for ext in ('.bam', '.bam.bai'):
        assert open(d / f'fallback{ext}', 'rb').read() == open(d / f'fallback_ref{ext}', 'rb').read()


def test_unknown_writer_raises(world, libmpn, oracle_built, monkeypatch):
    monkeypatch.setenv('MPN_BAM_WRITER', 'gpu')
    with pytest.raises(ValueError):
        run(world, 'bad')
