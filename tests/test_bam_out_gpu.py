"""GPU tests (-m gpu) of the device BAM writer (csrc/bam_out_kernels.hip): the scan and encode kernels on the lines of
bam_out_cases.py against bam.encode_record byte for byte, with the statuses of the serial host check; whole files -- .bam and
.bam.bai -- against bam.sam_to_sorted_bam with the device sort and the device deflate, byte for byte; refusals that leave no file;
bin/mpn-sam2bam."""
import os
import subprocess
import sys

import pytest

import bam_out_cases as bc
from bgzf_cases import big_sam
from megapath_nano_amd import abundance, bam

pytestmark = pytest.mark.gpu
ROOT = bc.ROOT


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return bc.build_host_check(tmp_path_factory.mktemp('bam_out_host'))


def check_equal(got, lines):
    assert len(got) == len(lines)
    for g, l in zip(got, lines):
        tid, pos0, end0, flag, rec = bc.expected(l)
        assert g[0] == bc.OK, (l[:80], g[0])
        assert g[1:5] == (tid, pos0, end0, flag), l[:80]
        assert g[5] == rec, l[:80]


def test_records_equal_encode_record(libmpn):
    lines = bc.good_lines()
    check_equal(bam.device_encode_lines(bc.REFS, lines), lines)


@pytest.mark.parametrize('pad', range(16))
def test_records_at_every_line_start_mod_16(libmpn, pad):
    lines = bc.basic_lines()
    check_equal(bam.device_encode_lines(bc.REFS, lines, pad=pad), lines)
    bare = [l.rstrip(b'\n') for l in lines]                       # and without their line feeds: other starts again
    check_equal(bam.device_encode_lines(bc.REFS, bare, pad=pad), bare)


def test_every_four_digit_fraction_is_the_float_strtod_gives(libmpn):
    lines = bc.float_lines()
    check_equal(bam.device_encode_lines(bc.REFS, lines), lines)


def test_statuses_equal_the_host_checks(libmpn, exe, tmp_path):
    cases = bc.refused_lines() + [(l, bc.OK) for l in bc.basic_lines()]
    lines = [l for l, _ in cases]
    got, host = bam.device_encode_lines(bc.REFS, lines), bc.host_encode(exe, tmp_path, lines)
    assert [g[0] for g in got] == [h[0] for h in host] == [st for _, st in cases]
    assert [g[5] for g in got] == [h[5] for h in host]
    cases = bc.skipped_lines()
    lines = [l for l, _ in cases]
    got, host = bam.device_encode_lines(bc.REFS, lines, exclude_flags=1028), bc.host_encode(exe, tmp_path, lines, exclude_flags=1028)
    assert [g[0] for g in got] == [h[0] for h in host] == [st for _, st in cases]
    assert all(g[5] == b'' for g in got)


def test_no_reference_at_all(libmpn):
    lines = [bc.line(rname='t1', rnext='t2'), bc.line(rname='*')]
    got = bam.device_encode_lines([], lines)
    assert [g[5] for g in got] == [bam.encode_record(l.decode().rstrip('\n').split('\t'), {})[4] for l in lines]


def test_native_bai_equals_bai_builder(libmpn, tmp_path):
    import numpy as np
    case = bc.cut_cases()[-1]                                       # 'spread'
    _, text, names, lens, recs = case
    path = str(tmp_path / 'spread.bam')
    bai = bam.BaiBuilder(len(names), 1 << 16)
    voff, v = [], 1 << 16
    for k, (t, p, e, f, s) in enumerate(recs):                      # offsets that ascend as a file's do
        v += (s << 12) + 7
        voff.append(v)
        bai.push(t, p, e, v, not f & 4)
    bai.finish(v + (1 << 16))
    bai.write(path + '.bai')
    t, p, e, f, s = (np.array(x) for x in zip(*recs))
    got = bam.native_bai(len(names), t, p, e, voff, (f & 4) == 0, 1 << 16, v + (1 << 16))
    assert got == open(path + '.bai', 'rb').read()


# ---- whole files -----------------------------------------------------------------------------------------------------------------------
def reference_files(sam, out, exclude):
    n = bam.sam_to_sorted_bam(sam, out, exclude_flags=exclude, sort_keys=abundance.device_sort_order, compress_blocks=bam.device_bgzf_blocks)
    return n, open(out, 'rb').read(), open(out + '.bai', 'rb').read()


def device_files(sam, out, exclude, **kw):
    n = bam.sam_to_sorted_bam_device(sam, out, exclude_flags=exclude, **kw)
    return n, open(out, 'rb').read(), open(out + '.bai', 'rb').read()


@pytest.fixture(scope='module')
def big(tmp_path_factory, libmpn):
    d = tmp_path_factory.mktemp('bam_out_big')
    sam = str(d / 'big.sam')
    n = big_sam(sam)
    return sam, n, reference_files(sam, str(d / 'ref.bam'), 1796)


@pytest.fixture(scope='module')
def tricky(tmp_path_factory, libmpn):
    d = tmp_path_factory.mktemp('bam_out_tricky')
    sam = str(d / 'tricky.sam')
    bc.tricky_sam(sam)
    return sam, {x: reference_files(sam, str(d / f'ref{x}.bam'), x) for x in (0, 4, 1796)}


def test_big_sam_files_are_identical(big, tmp_path):
    sam, n, want = big
    got = device_files(sam, str(tmp_path / 'dev.bam'), 1796)
    assert want[0] == n and len(want[1]) > 266 * 1000
    assert got[0] == want[0] and got[2] == want[2] and got[1] == want[1]


@pytest.mark.parametrize('exclude', [0, 4, 1796])
def test_tricky_sam_files_are_identical(tricky, tmp_path, exclude):
    sam, refs = tricky
    want = refs[exclude]
    got = device_files(sam, str(tmp_path / 'dev.bam'), exclude)
    assert 0 < want[0] and (exclude == 0 or want[0] < refs[0][0])
    assert got[0] == want[0] and got[2] == want[2] and got[1] == want[1]


@pytest.mark.parametrize('chunk', [4096, 65536])
def test_chunk_edges_change_nothing(tricky, tmp_path, chunk):
    sam, refs = tricky
    size = os.path.getsize(sam)
    assert size > 5 * 65536 and open(sam, 'rb').read()[4095:4096] == b'\n'           # a line ends exactly on the first edge
    got = device_files(sam, str(tmp_path / 'dev.bam'), 0, chunk_bytes=chunk)
    assert got == refs[0]


def test_index_sam_files_are_identical(libmpn, tmp_path):
    sam = os.path.join(ROOT, 'tests', 'golden', 'htslib', 'index.sam')
    want = reference_files(sam, str(tmp_path / 'ref.bam'), 0)
    assert device_files(sam, str(tmp_path / 'dev.bam'), 0) == want


def test_no_records_and_all_filtered(libmpn, tmp_path):
    head = '@SQ\tSN:t1\tLN:3000000\n'
    for name, body, exclude in (('empty', b'', 0), ('filtered', bc.line(flag=4) + bc.line(flag=260), 4)):
        sam = str(tmp_path / f'{name}.sam')
        open(sam, 'wb').write(head.encode() + body)
        want = reference_files(sam, str(tmp_path / f'{name}_ref.bam'), exclude)
        assert want[0] == 0 and device_files(sam, str(tmp_path / f'{name}_dev.bam'), exclude) == want


def test_a_refused_line_is_named_and_nothing_is_written(tricky, tmp_path):
    sam, _ = tricky
    lines = open(sam, 'rb').read().split(b'\n')
    at = 250
    assert lines[at][:1] != b'@' and lines[at].strip()
    lines[at] += b'\tXX:Q:1'
    bad, out = str(tmp_path / 'bad.sam'), str(tmp_path / 'bad.bam')
    open(bad, 'wb').write(b'\n'.join(lines))
    for chunk in (None, 4096):
        with pytest.raises(bam.DeviceRefused) as e:
            bam.sam_to_sorted_bam_device(bad, out, chunk_bytes=chunk)
        assert (e.value.line, e.value.status) == (at + 1, bc.TAG_TYPE) and 'tag type' in str(e.value)
        assert not os.path.exists(out) and not os.path.exists(out + '.bai')


def test_a_full_pool_refuses(tricky, tmp_path):
    sam, _ = tricky
    out = str(tmp_path / 'pool.bam')
    with pytest.raises(bam.DeviceRefused) as e:
        bam.sam_to_sorted_bam_device(sam, out, pool_bytes=1)
    assert e.value.status == bc.POOL and e.value.line == 5                      # the first record line behind four header lines
    assert not os.path.exists(out) and not os.path.exists(out + '.bai')


def test_a_header_line_behind_a_record_refuses(libmpn, tmp_path):
    sam, out = str(tmp_path / 'late.sam'), str(tmp_path / 'late.bam')
    open(sam, 'wb').write(b'@SQ\tSN:t1\tLN:3000000\n' + bc.line() + b'@CO\tlate\n' + bc.line())
    with pytest.raises(bam.DeviceRefused) as e:
        bam.sam_to_sorted_bam_device(sam, out)
    assert (e.value.line, e.value.status) == (3, bc.LATE_HEADER) and not os.path.exists(out)


def test_builder_fed_in_pieces_writes_the_same_files(tricky, tmp_path):
    sam, refs = tricky
    data = open(sam, 'rb').read()
    header = [l.decode() + '\n' for l in data.split(b'\n') if l[:1] == b'@']
    names, lens = bam.parse_header(header)
    b = bam.DeviceBamBuilder(names, lens, bam.sorted_header_text(header), 1796)
    for k in range(0, len(data), 77777):
        b.add_text(data[k:k + 77777])
    out = str(tmp_path / 'pieces.bam')
    n = b.finish(out)
    ms = b.stage_ms()
    b.close()
    assert (n, open(out, 'rb').read(), open(out + '.bai', 'rb').read()) == refs[1796]
    assert set(ms) == set(bam.STAGES) and ms['encode'] > 0 and ms['deflate'] > 0


def test_sam2bam_tool_writes_the_same_files(big, tmp_path):
    sam, n, want = big
    out = str(tmp_path / 'tool.bam')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'mpn-sam2bam'), '-F', '1796', sam, out], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert f'{n} records'.encode() in p.stderr
    assert open(out, 'rb').read() == want[1] and open(out + '.bai', 'rb').read() == want[2]
    bad = str(tmp_path / 'bad.sam')
    open(bad, 'wb').write(b'@SQ\tSN:t1\tLN:3000000\n' + bc.line() + bc.line(tags=('XB:B:c,1',)))
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'mpn-sam2bam'), bad, str(tmp_path / 'bad.bam')], capture_output=True, timeout=300)
    assert p.returncode != 0 and b'line 3' in p.stderr and b'array tag' in p.stderr and not os.path.exists(str(tmp_path / 'bad.bam'))
