"""GPU tests (-m gpu) of BAM files whose BGZF blocks were deflated on the GPU (bam.device_bgzf_blocks over mpn_bgzf_compress):
the records are those of the zlib file, the index points at record starts, and Align() takes the path under MPN_BGZF=device."""
import pandas as pd
import pytest

from bam_reader import read_bai, read_bam
from megapath_nano_amd import bam
from bgzf_cases import big_sam

pytestmark = pytest.mark.gpu


class FakeMetadata:
    """The joins Align() uses, over an in-memory table (as in test_align_mirror_gpu.py)."""

    def __init__(self, table):
        self.t = table

    def get_assembly_path(self, *, assembly_list, how='inner'):
        return assembly_list.merge(self.t[['assembly_id', 'path']].drop_duplicates(), on='assembly_id', how=how)

    def get_assembly_length(self, *, assembly_list, how='inner'):
        return assembly_list.merge(self.t[['assembly_id', 'assembly_length']].drop_duplicates(), on='assembly_id', how=how)

    def get_sequence_tax_id(self, *, assembly_list, how='inner'):
        return assembly_list.merge(self.t[['assembly_id', 'tax_id', 'species_tax_id', 'genus_tax_id', 'sequence_id']],
                                   on='assembly_id', how=how)


def test_device_compressed_bam_has_the_same_records_and_a_sound_index(tmp_path, libmpn):
    sam = str(tmp_path / 'big.sam')
    n = big_sam(sam)
    ref_out, out = str(tmp_path / 'zlib.bam'), str(tmp_path / 'device.bam')
    assert bam.sam_to_sorted_bam(sam, ref_out, exclude_flags=1796) == n
    assert bam.sam_to_sorted_bam(sam, out, exclude_flags=1796, compress_blocks=bam.device_bgzf_blocks) == n
    b, want = read_bam(out), read_bam(ref_out)
    assert len(b['blocks']) > bam.BgzfWriter.PENDING + 10
    assert b['text'] == want['text'] and b['refs'] == want['refs']
    assert [r['raw'] for r in b['records']] == [r['raw'] for r in want['records']]
    # the checks of test_bam.py's test_threaded_bgzf_index_points_at_record_starts...: the two .bai files need not be equal
    # (htslib folds bins by their compressed span), but each must be sound
    ublock = {c: u for c, u in b['blocks']}
    upos = lambda v: ublock[v >> 16] + (v & 0xffff)  # noqa: E731
    starts = {upos(v) for v, _ in b['offsets']}
    refs, nc = read_bai(out + '.bai')
    n_chunks = 0
    for tid, (bins, lin) in enumerate(refs):
        for bn, chunks in bins.items():
            if bn == bam.META_BIN:
                continue
            for beg, end in chunks:
                assert upos(beg) in starts and beg < end, (tid, bn)
                n_chunks += 1
        assert all(upos(v) in starts for v in lin), tid
    assert n_chunks > 20 and nc == 0
    for r, (v, _) in zip(b['records'], b['offsets']):
        ref_len = sum(c >> 4 for c in r['cigar'] if (c & 15) in (0, 2, 3, 7, 8))
        bn = bam.reg2bin(r['pos'], r['pos'] + max(ref_len, 1))
        bins = refs[r['tid']][0]
        while bn not in bins:
            bn = (bn - 1) >> 3
        assert any(upos(beg) <= upos(v) < upos(end) for beg, end in bins[bn]), r['name']


def test_align_with_mpn_bgzf_device_writes_the_same_records(tmp_path, libmpn, oracle_built, monkeypatch):
    import gzip
    from map_cases import small_world
    from megapath_nano_amd.aligner import Align
    d = tmp_path
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
    table = pd.DataFrame(rows)

    def run(prefix):
        return Align(assembly_metadata=FakeMetadata(table), global_options=dict(assembly_folder=str(d), min_alignment_score=0, debug=False),
                     temp_dir_name=str(d), log_file=None, query_filename_list=pd.DataFrame({'path': [str(fq)]}),
                     target_assembly_list=table[['assembly_id']].copy(), aligner_options=['-t', '4', '-N', '50', '-p', '1', '-x', 'map-ont'],
                     paf_path_and_prefix=str(d / prefix))

    monkeypatch.delenv('MPN_BGZF', raising=False)
    a = run('plain')
    calls = []
    monkeypatch.setattr(bam, 'device_bgzf_blocks', lambda p, _f=bam.device_bgzf_blocks: (calls.append(len(p)), _f(p))[1])
    monkeypatch.setenv('MPN_BGZF', 'device')
    b = run('device')
    assert calls and a.equals(b)
    x, y = read_bam(str(d / 'plain.bam')), read_bam(str(d / 'device.bam'))
    assert len(x['records']) > 0 and [r['raw'] for r in x['records']] == [r['raw'] for r in y['records']] and x['text'] == y['text']
    assert open(d / 'plain.bam', 'rb').read() != open(d / 'device.bam', 'rb').read()      # another compressor wrote it
    monkeypatch.setenv('MPN_BGZF', 'gpu')
    with pytest.raises(ValueError):
        run('bad')
