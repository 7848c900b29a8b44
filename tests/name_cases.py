"""The name cases that the name set meets on the host (tests/test_name_set_host.py, scripts/name_set_host_check.cpp) and on the GPU
(tests/test_name_lookup_gpu.py), and the dict that says what a lookup has to answer."""
import numpy as np

LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 255, 5000)


def _bytes(rng, n):
    """n bytes an id can hold in a FASTQ header: no blank, TAB, LF or CR"""
    b = rng.integers(0x21, 0x100, size=n, dtype=np.int64).astype(np.uint8)
    return bytes(b)


def ids():
    """distinct ids: every length of LENGTHS, pairs that differ in one byte at either end, a prefix of another, VT / FF / high bytes"""
    rng = np.random.default_rng(19)
    out = [_bytes(rng, n) for n in LENGTHS]
    base = _bytes(rng, 40)
    out += [base, base[:-1] + bytes([base[-1] ^ 1]), bytes([base[0] ^ 1]) + base[1:]]
    out += [base[:16], base[:17], base + b'x']                       # prefixes that end at and behind a word, and an extension
    out += [b'v\x0bt', b'f\x0cf', bytes(range(0x80, 0x100)), b'\xff', b'\x80' * 16, b'a\x0b\x0c\xfe' * 9]
    out += [b'0f3c9a52-7d1e-4b8a-9c55-e1f2a3b4c5d6', b'0f3c9a52-7d1e-4b8a-9c55-e1f2a3b4c5d7']      # ONT UUIDs, 36 bytes
    assert len(set(out)) == len(out) and not any(set(x) & set(b' \t\n\r') for x in out)
    return out


def want_found(names, queries):
    """the smallest index of names whose bytes are the query's, or -1"""
    first = {}
    for i, x in enumerate(names):
        first.setdefault(x, i)
    return [first.get(q, -1) for q in queries]


def default_slots(distinct):
    s = 16
    while s < 2 * distinct:
        s *= 2
    return s
