"""CPU tests of the compress_blocks hook of the BAM writer (megapath_nano_amd/bam.py): a hook that compresses exactly as the writer
does itself must leave the files byte for byte what they are without it."""
import numpy as np
import pytest

from bgzf_cases import big_sam
from megapath_nano_amd import bam


@pytest.fixture(scope='module')
def written(tmp_path_factory):
    d = tmp_path_factory.mktemp('hook')
    sam = str(d / 'big.sam')
    n = big_sam(sam)
    calls = []

    def hook(payloads):
        calls.append([bytes(p) for p in payloads])
        return [bam._bgzf_block(p, 6) for p in payloads]

    assert bam.sam_to_sorted_bam(sam, str(d / 'plain.bam'), exclude_flags=1796, level=6) == n
    assert bam.sam_to_sorted_bam(sam, str(d / 'hook.bam'), exclude_flags=1796, level=6, compress_blocks=hook) == n
    return d, calls


def test_a_hook_that_compresses_like_the_writer_gives_the_same_files(written):
    d, _ = written
    assert open(d / 'hook.bam', 'rb').read() == open(d / 'plain.bam', 'rb').read()
    assert open(d / 'hook.bam.bai', 'rb').read() == open(d / 'plain.bam.bai', 'rb').read()


def test_the_hook_gets_the_payloads_in_file_order_a_batch_at_a_time(written):
    from bam_reader import read_bgzf
    d, calls = written
    assert len(calls) > 1 and all(0 < len(c) <= bam.BgzfWriter.PENDING for c in calls)
    payloads = [p for c in calls for p in c]
    assert len(payloads) > bam.BgzfWriter.PENDING + 10
    assert all(0 < len(p) <= bam.BGZF_BLOCK for p in payloads)
    data, blocks = read_bgzf(str(d / 'plain.bam'))
    assert b''.join(payloads) == data and len(blocks) == len(payloads) + 1      # + the empty end-of-file block
    assert [u for _, u in blocks[:-1]] == np.cumsum([0] + [len(p) for p in payloads[:-1]]).tolist()


def test_level_0_does_not_go_through_the_hook(tmp_path):
    def hook(payloads):
        raise AssertionError('level 0 is written as stored blocks by the writer itself')
    recs = [(0, 5, 8, 0, b'x' * 100)] * 3
    bam.write_bam(str(tmp_path / 'a.bam'), '@SQ\tSN:t\tLN:100\n', ['t'], [100], recs, level=0, compress_blocks=hook)
    bam.write_bam(str(tmp_path / 'b.bam'), '@SQ\tSN:t\tLN:100\n', ['t'], [100], recs, level=0)
    assert open(tmp_path / 'a.bam', 'rb').read() == open(tmp_path / 'b.bam', 'rb').read()
    assert bam.BgzfWriter.PENDING == 256


def test_a_hook_that_loses_a_block_is_an_error(tmp_path):
    with pytest.raises(ValueError):
        bam.write_bam(str(tmp_path / 'c.bam'), '@SQ\tSN:t\tLN:100\n', ['t'], [100], [(0, 5, 8, 0, b'x' * 100)], compress_blocks=lambda p: [])
