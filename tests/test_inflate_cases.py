"""CPU tests: the inflate cases against zlib / gzip (the oracle), and against the serial decoder the GPU kernel runs, built for the
host with plain g++ (scripts/inflate_host_check.cpp)."""
import gzip
import io
import os
import struct
import subprocess
import zlib

import pytest

import inflate_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def cases():
    return ic.make_cases()


def host_inflate(stream):
    return gzip.GzipFile(fileobj=io.BytesIO(stream), mode='rb').read()


def test_case_list_covers_what_it_should(cases):
    names = {c['name'] for c in cases}
    assert len(names) == len(cases)
    assert {c['status'] for c in cases} == {ic.OK, ic.TRUNCATED, ic.BAD_MAGIC, ic.BAD_BLOCK, ic.BAD_CODE, ic.BAD_DISTANCE, ic.BAD_CRC, ic.BAD_SIZE}
    assert sum(c['status'] == ic.TRUNCATED for c in cases) >= 3


def test_zlib_accepts_every_valid_case(cases):
    for c in cases:
        if c['status'] == ic.OK:
            assert host_inflate(c['gz']) == c['data'], c['name']


def test_zlib_rejects_every_malformed_case(cases):
    for c in cases:
        if c['status'] != ic.OK:
            with pytest.raises((gzip.BadGzipFile, EOFError, zlib.error)):
                host_inflate(c['gz'])
                pytest.fail(c['name'] + ' was accepted')


def run_host_check(exe, tmp_path, streams_and_caps):
    src, dst = tmp_path / 'cases.bin', tmp_path / 'results.bin'
    with open(src, 'wb') as f:
        f.write(struct.pack('<I', len(streams_and_caps)))
        for stream, cap in streams_and_caps:
            f.write(struct.pack('<QQ', len(stream), cap) + stream)
    subprocess.run([str(exe), str(src), str(dst)], check=True, timeout=300)
    blob, out, p = dst.read_bytes(), [], 0
    for _ in streams_and_caps:
        status, members, length, stored = struct.unpack_from('<iiQQ', blob, p)
        p += 24
        out.append((status, members, length, blob[p:p + stored]))
        p += stored
    assert p == len(blob)
    return out


def test_host_build_of_the_decoder_agrees(cases, tmp_path):
    exe = tmp_path / 'inflate_host_check'
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-o', str(exe), os.path.join(ROOT, 'scripts', 'inflate_host_check.cpp')], check=True)
    got = run_host_check(exe, tmp_path, [(c['gz'], len(c['data']) if c['data'] is not None else 1 << 16) for c in cases])
    for c, (status, members, length, data) in zip(cases, got):
        assert status == c['status'], (c['name'], status)
        if c['status'] == ic.OK:
            assert (members, length) == (c['members'], len(c['data'])) and data == c['data'], c['name']
    # slots that are too small: the exact length, the first bytes, and nothing past the slot
    small = [c for c in cases if c['status'] == ic.OK and len(c['data']) > 1]
    got = run_host_check(exe, tmp_path, [(c['gz'], len(c['data']) // 2) for c in small])
    for c, (status, members, length, data) in zip(small, got):
        assert (status, members, length) == (ic.OVERFLOW, c['members'], len(c['data'])) and data == c['data'][:len(c['data']) // 2], c['name']
