"""GPU tests (-m gpu) of mpn_bgzf_compress (csrc/bgzf_kernels.hip): BGZF blocks deflated on the GPU, one workgroup per block.
zlib's inflate and CRC32 are the judges.  Every payload of bgzf_cases.py goes through the entry point in all three modes, in one
batch, in a second batch in reverse order and alone; the size conditions are derived in the tests that state them."""
import ctypes as ct
import zlib

import numpy as np
import pytest

import bgzf_cases as bc

pytestmark = pytest.mark.gpu
AUTO, STORED, NO_MATCH = 0, 1, 2
MODES = {'auto': AUTO, 'stored': STORED, 'no_match': NO_MATCH}


def compress(lib, payloads, mode, cap=None):
    """-> (return value, out bytes up to the return value, out_off list)"""
    lib.mpn_bgzf_compress.argtypes = [ct.c_int64, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_int64, ct.c_void_p, ct.c_int32]
    lib.mpn_bgzf_compress.restype = ct.c_int64
    n = len(payloads)
    pay_off = np.zeros(n + 1, dtype=np.int64)
    pay_off[1:] = np.cumsum([len(p) for p in payloads])
    data = np.frombuffer(b''.join(payloads) + b'\0', dtype=np.uint8)
    if cap is None:
        cap = int(pay_off[n]) + 31 * n
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    out_off = np.full(n + 1, -7, dtype=np.int64)
    r = lib.mpn_bgzf_compress(n, data.ctypes.data, pay_off.ctypes.data, out.ctypes.data, cap, out_off.ctypes.data, mode)
    return r, out[:max(r, 0)].tobytes(), out_off.tolist()


def split(r, out, off):
    assert r >= 0 and off[0] == 0 and off[-1] == r == len(out)
    assert all(a < b for a, b in zip(off, off[1:])), 'out_off must ascend: the blocks lie one after another'
    return [out[a:b] for a, b in zip(off, off[1:])]


@pytest.fixture(scope='module')
def cases():
    return bc.make_cases()


@pytest.fixture(scope='module')
def results(libmpn, cases):
    """mode -> dict(batch, reversed, alone): lists of blocks in the order of `cases`"""
    payloads = [p for _, p in cases]
    res = {}
    for mode in MODES.values():
        batch = split(*compress(libmpn, payloads, mode))
        rev = split(*compress(libmpn, payloads[::-1], mode))[::-1]
        alone = [split(*compress(libmpn, [p], mode))[0] for p in payloads]
        res[mode] = dict(batch=batch, reversed=rev, alone=alone)
    return res


@pytest.mark.parametrize('mode', sorted(MODES))
def test_every_block_inflates_to_its_payload_wherever_it_stood(results, cases, mode):
    r = results[MODES[mode]]
    for k, (name, payload) in enumerate(cases):
        btype, _, _ = bc.check_block(r['batch'][k], payload)
        assert r['batch'][k] == r['reversed'][k] == r['alone'][k], name
        if mode == 'stored':
            assert btype == 0, name


def test_stored_fallback_for_random_bytes_and_tiny_payloads(results, cases):
    for mode in (AUTO, NO_MATCH):
        for k, (name, payload) in enumerate(cases):
            blk = results[mode]['batch'][k]
            if name == 'random' or len(payload) == 0:
                assert bc.check_block(blk, payload)[0] == 0, name
                assert blk == results[STORED]['batch'][k]


def test_one_repeated_byte_is_a_handful_of_matches(results, cases):
    """65 280 equal bytes: one literal and 254 matches of at most 258 at the longest legal codes (15 + 15 bits) stay below 1 KiB;
    zlib needs 80-303 bytes; literals alone need a bit per byte, 8 160 bytes.  Bound: 2 048."""
    k = [n for n, _ in cases].index('one_byte_65280')
    assert len(results[AUTO]['batch'][k]) <= 2048
    assert len(results[NO_MATCH]['batch'][k]) > 8160
    assert bc.check_block(results[AUTO]['batch'][k], cases[k][1])[0] == 2


def test_four_symbols_under_no_match_reach_the_entropy_of_five(results, cases):
    """Four equally likely symbols and the end-of-block symbol: 2.25 bits a byte at most, 18 360 bytes; zlib Z_HUFFMAN_ONLY gives
    18 372; a fixed-Huffman coder more than 65 000.  Bound: 19 000.  With matches the block inflates too: its 4-byte matches lie
    at every distance up to and beyond 32 768, and a distance beyond the window would make inflate fail."""
    k = [n for n, _ in cases].index('four_symbols')
    payload = cases[k][1]
    assert len(bc.zlib_raw(payload, 6, zlib.Z_HUFFMAN_ONLY)) < 19000
    assert len(results[NO_MATCH]['batch'][k]) <= 19000
    assert bc.check_block(results[AUTO]['batch'][k], payload)[0] == 2


def test_all_symbols_reach_the_ends_of_both_alphabets(results, cases):
    k = [n for n, _ in cases].index('all_symbols')
    btype, hlit, hdist = bc.check_block(results[AUTO]['batch'][k], cases[k][1])
    assert btype == 2 and hlit == 286 and hdist >= 29


@pytest.mark.parametrize('name,counts', [('fibonacci', bc.FIB_COUNTS), ('skewed', bc.SKEWED_COUNTS)])
def test_skewed_counts_exercise_length_limiting(results, cases, name, counts):
    """22 symbols with Fibonacci counts: their unrestricted Huffman code is deeper than 15 bits.  With the end-of-block symbol
    beside them some merges tie, and a tree that breaks the ties towards the shallow side is only 12 deep, so the second payload
    has counts without any tie: its code is 19 deep for every implementation, and the literal code of its NO_MATCH block went
    through the length limiting -- and inflate accepted it as complete."""
    k = [n for n, _ in cases].index(name)
    payload = cases[k][1]
    got = np.bincount(np.frombuffer(payload, dtype=np.uint8), minlength=256)
    assert sorted(got[got > 0].tolist()) == sorted(counts) and len(payload) == sum(counts)
    assert bc.huffman_depth(list(counts)) > 15
    if name == 'fibonacci':
        assert len(payload) == 46367
    else:
        assert bc.huffman_depth(list(counts) + [1]) > 15      # the end-of-block symbol included
    assert bc.check_block(results[NO_MATCH]['batch'][k], payload)[0] == 2
    # zlib's own limited code is the yardstick, with the margin of a header without run-length symbols (at most about 280 bytes)
    assert len(results[NO_MATCH]['batch'][k]) <= len(bc.zlib_raw(payload, 6, zlib.Z_HUFFMAN_ONLY)) + 26 + 280


def test_bam_like_blocks_against_zlib(results, cases):
    """Total size of the BAM-like full blocks: NO_MATCH at most 1.05 x zlib Z_HUFFMAN_ONLY (a header without run-length symbols
    costs at most about 280 bytes, 0.7 %; the rest is for another length-limiting heuristic), AUTO at most 1.05 x zlib level 1
    (a greedy matcher corresponds to level 1)."""
    ks = [k for k, (n, _) in enumerate(cases) if n.startswith('bam')]
    assert len(ks) >= 3 and all(len(cases[k][1]) == bc.BGZF_BLOCK for k in ks)
    huff = sum(len(bc.zlib_raw(cases[k][1], 6, zlib.Z_HUFFMAN_ONLY)) + 26 for k in ks)
    lvl1 = sum(len(bc.zlib_raw(cases[k][1], 1)) + 26 for k in ks)
    got_nm = sum(len(results[NO_MATCH]['batch'][k]) for k in ks)
    got_auto = sum(len(results[AUTO]['batch'][k]) for k in ks)
    print(f'bam-like blocks: huffman-only {huff}, level 1 {lvl1}, device NO_MATCH {got_nm}, device AUTO {got_auto}')
    assert got_nm <= 1.05 * huff
    assert got_auto <= 1.05 * lvl1


def test_refusals(libmpn):
    from megapath_nano_amd import _ffi
    r, _, _ = compress(libmpn, [b'x' * 10, b'y' * 65281], AUTO)
    assert r == -1 and '65280' in _ffi.last_error()
    payloads = [b'abc' * 1000, b'', b'z' * 70]
    want, out, off = compress(libmpn, payloads, AUTO)
    assert want > 0
    r, _, short_off = compress(libmpn, payloads, AUTO, cap=want - 1)
    assert r == -3 and short_off[-1] == want
    r, out2, off2 = compress(libmpn, payloads, AUTO, cap=want)
    assert r == want and out2 == out and off2 == off
    assert compress(libmpn, [], AUTO)[0] == 0


def test_device_bgzf_blocks_is_the_python_face_of_it(results, cases):
    from megapath_nano_amd import bam
    payloads = [p for _, p in cases[:20]]
    assert bam.device_bgzf_blocks(payloads) == results[AUTO]['batch'][:20]
    assert bam.device_bgzf_blocks(payloads, mode=bam.BGZF_NO_MATCH) == results[NO_MATCH]['batch'][:20]
    assert bam.device_bgzf_blocks([]) == []
