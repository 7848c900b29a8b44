"""CPU tests: the CRC-32 arithmetic the BGZF and inflate kernels share (csrc/crc32_poly.h), built for the host with plain g++
(scripts/crc32_host_check.cpp) and run the way the kernels use it -- slices from a zero register, weighted by the bytes behind
them, joined into a running register over one or two flushes -- against zlib.crc32."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'scripts', 'crc32_host_check.cpp')

# around the slice counts (a slice of 0, 1 or 2 bytes; lanes without bytes), the largest inflate flush, the largest BGZF payload
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 16384 + 257, 65280)
SLICES = (64, 256)


@pytest.fixture(scope='module')
def cases():
    """(data, split, slices): every length as one flush (split = length) and as two, cut at an odd offset."""
    rng = np.random.default_rng(32)
    out = []
    for n in LENGTHS:
        data = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        for slices in SLICES:
            out.append((data, n, slices))
            out.append((data, min(n, (n // 2) | 1), slices))
    return out


def run_cases(exe, tmp_path, cases):
    src, dst = tmp_path / 'cases.bin', tmp_path / 'results.bin'
    with open(src, 'wb') as f:
        f.write(struct.pack('<I', len(cases)))
        for data, split, slices in cases:
            f.write(struct.pack('<QQI', len(data), split, slices) + data)
    subprocess.run([str(exe), str(src), str(dst)], check=True, timeout=60)
    blob = dst.read_bytes()
    assert len(blob) == 4 * len(cases)
    return struct.unpack(f'<{len(cases)}I', blob)


def check(exe, tmp_path, cases):
    assert any(split % 2 == 1 and 0 < split < len(data) for data, split, _ in cases)
    got = run_cases(exe, tmp_path, cases)
    for (data, split, slices), crc in zip(cases, got):
        assert crc == zlib.crc32(data), (len(data), split, slices)


def test_sliced_crc_equals_zlib(cases, tmp_path):
    exe = tmp_path / 'crc32_host_check'
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-o', str(exe), SRC], check=True)
    check(exe, tmp_path, cases)


def test_sliced_crc_under_the_sanitizers(cases, tmp_path):
    exe = tmp_path / 'crc32_host_check_san'
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-o', str(exe), SRC], check=True)
    check(exe, tmp_path, cases)
