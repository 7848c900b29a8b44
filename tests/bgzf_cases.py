"""Payloads for the tests of the GPU BGZF compressor (mpn_bgzf_compress) and what judges its output: zlib's inflate and CRC32."""
import struct
import zlib

import numpy as np

BGZF_BLOCK = 0xff00
HEADER = b'\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00'
EDGE_LENGTHS = (0, 1, 2, 3, 4, 5, 255, 256, 257, 258, 259, 260, 65279, 65280)
FIB_COUNTS = (1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765, 10946, 17711)   # sum 46367
# c[k] = c[k-1] + c[k-2] + 1: with the end-of-block symbol (count 1) no two weights of the Huffman merge are ever equal, so the
# tree is the one chain, 19 deep, whichever way an implementation breaks ties (sum 46344)
SKEWED_COUNTS = (2, 4, 7, 12, 20, 33, 54, 88, 143, 232, 376, 609, 986, 1596, 2583, 4180, 6764, 10945, 17710)


def _texty(rng, n):
    """n bytes of words drawn from a small dictionary: literals of a skewed alphabet and matches of many lengths"""
    words = [bytes(rng.integers(97, 123, size=int(rng.integers(2, 12)), dtype=np.uint8)) for _ in range(200)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))] + b' '
    return bytes(out[:n])


def all_symbols_payload(rng):
    """Every byte value, matches of lengths 3..258 and distances from 1 to beyond 24576: the largest length symbol (285) and the
    two largest distance symbols (28, 29) get used."""
    out = bytearray(bytes(range(256)) + bytes(rng.integers(0, 256, size=37000 - 256, dtype=np.uint8)))
    lengths = list(range(3, 259, 5)) + [258, 258, 257, 130, 67, 35, 19, 11]
    for far in (True, False):
        for L in lengths:
            pos = len(out)
            src = pos - int(rng.integers(17000, 30000)) if far else pos - int(rng.integers(L, 2000))
            out += out[src:src + L] + bytes(rng.integers(0, 256, size=2, dtype=np.uint8))
    out += b'\x07' * 300                       # distance 1
    assert len(out) <= BGZF_BLOCK
    return bytes(out)


def counts_payload(rng, counts):
    data = np.repeat(np.arange(len(counts), dtype=np.uint8) + 65, counts)
    rng.shuffle(data)
    return data.tobytes()


def bam_like_blocks(n_reads=36):
    """Full BGZF payload blocks of BAM records like those of test_bam.py's 3 000-read SAM (random ACGT reads of 2-9 kb with random
    qualities): the concatenated records cut every BGZF_BLOCK bytes, the incomplete tail dropped."""
    from megapath_nano_amd import bam
    rng = np.random.default_rng(5)
    ref_id = {'t1': 0, 't2': 1}
    data = bytearray()
    for i in range(n_reads):
        L = int(rng.integers(2000, 9000))
        seq = ''.join(rng.choice(list('ACGT'), size=L))
        qual = ''.join(chr(33 + int(x)) for x in rng.integers(0, 40, size=L))
        ref, pos = ('t1', int(rng.integers(1, 2900000))) if i % 3 else ('t2', int(rng.integers(1, 1900000)))
        rec = bam.encode_record(f'r{i}\t{16 * (i % 2)}\t{ref}\t{pos}\t60\t{L}M\t*\t0\t0\t{seq}\t{qual}\tNM:i:{i % 50}'.split('\t'), ref_id)[4]
        data += struct.pack('<i', len(rec)) + rec
    return [bytes(data[o:o + BGZF_BLOCK]) for o in range(0, len(data) - BGZF_BLOCK + 1, BGZF_BLOCK)]


def big_sam(path, n_reads=3000):
    """The 3 001-record SAM of test_bam.py: more than PENDING + 10 BGZF blocks."""
    rng = np.random.default_rng(5)
    lines = ['@SQ\tSN:t1\tLN:3000000\n', '@SQ\tSN:t2\tLN:2000000\n']
    for i in range(n_reads):
        L = int(rng.integers(2000, 9000))
        seq = ''.join(rng.choice(list('ACGT'), size=L))
        qual = ''.join(chr(33 + int(x)) for x in rng.integers(0, 40, size=L))
        ref, pos = ('t1', int(rng.integers(1, 2900000))) if i % 3 else ('t2', int(rng.integers(1, 1900000)))
        lines.append(f'r{i}\t{16 * (i % 2)}\t{ref}\t{pos}\t60\t{L}M\t*\t0\t0\t{seq}\t{qual}\tNM:i:{i % 50}\n')
    n_ops = 70001
    lines.append('long\t0\tt1\t5\t60\t' + '1M1I' * 35000 + '1M' + '\t*\t0\t0\t' + 'A' * n_ops + '\t*\n')
    with open(path, 'w') as f:
        f.write(''.join(lines))
    return n_reads + 1


def make_cases():
    """-> list of (name, payload)"""
    rng = np.random.default_rng(20)
    cases = [(f'len{n}', _texty(rng, n)) for n in EDGE_LENGTHS]
    cases.append(('one_byte_65280', b'Q' * BGZF_BLOCK))
    cases.append(('one_byte_300', b'\x00' * 300))
    for period in (2, 3, 259):
        unit = bytes(rng.integers(0, 256, size=period, dtype=np.uint8))
        n = 65280 if period == 259 else 20001
        cases.append((f'period{period}', (unit * (n // period + 1))[:n]))
    cases.append(('four_symbols', bytes(rng.choice(np.frombuffer(b'ACGT', dtype=np.uint8), size=BGZF_BLOCK))))
    cases.append(('random', bytes(rng.integers(0, 256, size=BGZF_BLOCK, dtype=np.uint8))))
    x = bytes(rng.integers(0, 256, size=500, dtype=np.uint8))
    cases.append(('ends_in_repeat', bytes(rng.integers(0, 256, size=1000, dtype=np.uint8)) + x + x + x[:137]))
    cases.append(('all_symbols', all_symbols_payload(rng)))
    cases.append(('fibonacci', counts_payload(rng, FIB_COUNTS)))
    cases.append(('skewed', counts_payload(rng, SKEWED_COUNTS)))
    cases += [(f'bam{i}', b) for i, b in enumerate(bam_like_blocks())]
    return cases


def huffman_depth(counts):
    """The largest code length of an unrestricted Huffman code over the counts (heapq: the textbook merge)."""
    import heapq
    heap = [(c, 0) for c in counts if c > 0]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def check_block(block, payload):
    """Everything a BGZF block must satisfy for its payload; -> (BTYPE, HLIT, HDIST) of its one deflate block (the last two are
    None for a stored one)."""
    assert block[:16] == HEADER
    bsize = struct.unpack_from('<H', block, 16)[0]
    assert bsize == len(block) - 1 and bsize <= 65310
    body = block[18:-8]
    d = zlib.decompressobj(-15)
    data = d.decompress(body) + d.flush()
    assert d.eof and d.unused_data == b'', 'more than one deflate stream, or bytes behind it'
    assert data == payload
    crc, isize = struct.unpack_from('<II', block, len(block) - 8)
    assert crc == zlib.crc32(payload) & 0xffffffff and isize == len(payload)
    assert len(block) <= len(payload) + 31, 'larger than the stored form'
    assert body[0] & 1 == 1, 'BFINAL'
    btype = body[0] >> 1 & 3
    assert btype in (0, 2)
    if btype == 0:
        assert len(body) == 5 + len(payload)
        return 0, None, None
    bits = body[0] | body[1] << 8 | body[2] << 16
    hlit, hdist, hclen = (bits >> 3 & 31) + 257, (bits >> 8 & 31) + 1, (bits >> 13 & 15) + 4
    assert 257 <= hlit <= 286 and 1 <= hdist <= 30 and 4 <= hclen <= 19
    return 2, hlit, hdist


def zlib_raw(payload, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(payload) + c.flush()
