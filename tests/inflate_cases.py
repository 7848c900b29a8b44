"""The gzip streams every inflate test runs (tests/test_inflate_cases.py on the CPU, tests/test_inflate_gpu.py on the GPU): streams
zlib wrote, and streams written bit by bit here for what zlib never writes (a 15-bit code, a single distance code, run symbols that
cross from the literal/length lengths into the distance lengths, a distance of exactly 32768, stored blocks of 0 and 65535 bytes),
plus malformed streams with the status each must end in.  zlib itself is the oracle: test_inflate_cases.py holds every case against it.
"""
import struct
import zlib

import numpy as np

# include/mpn_ingest.h
OK, TRUNCATED, BAD_MAGIC, BAD_BLOCK, BAD_CODE, BAD_DISTANCE, BAD_CRC, BAD_SIZE, OVERFLOW, UNSUPPORTED = range(10)

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


class BitWriter:
    """RFC 1951 3.1.1: values go in starting at the least significant bit of a byte, Huffman codes most significant bit first."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, count):
        self.acc |= (value & ((1 << count) - 1)) << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        for k in range(length - 1, -1, -1):
            self.bits((code >> k) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """RFC 1951 3.2.2: lengths -> {symbol: (code, length)}"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    table = {}
    for sym, l in enumerate(lens):
        if l:
            table[sym] = (nxt[l], l)
            nxt[l] += 1
    return table


def complete_lens(symbols, n):
    """A complete code over the given symbols of an alphabet of n: lengths k - 1 and k"""
    m = len(symbols)
    assert m >= 2
    k = (m - 1).bit_length()
    short = (1 << k) - m
    lens = [0] * n
    for j, s in enumerate(sorted(symbols)):
        lens[s] = k - 1 if j < short else k
    return lens


def put_tokens(w, tokens, ll, dd):
    """tokens: ints (literals) and (length, distance) pairs; then the end-of-block symbol"""
    for t in tokens:
        if isinstance(t, int):
            w.code(*ll[t])
            continue
        length, dist = t
        ls = max(s for s in range(29) if LEN_BASE[s] <= length) if length < 258 else 28
        w.code(*ll[257 + ls])
        w.bits(length - LEN_BASE[ls], LEN_EXTRA[ls])
        ds = max(s for s in range(30) if DIST_BASE[s] <= dist)
        w.code(*dd[ds])
        w.bits(dist - DIST_BASE[ds], DIST_EXTRA[ds])
    w.code(*ll[256])


def stored_block(w, data, final, nlen=None):
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    w.raw(struct.pack('<HH', len(data), (len(data) ^ 0xffff) if nlen is None else nlen))
    w.raw(data)


def fixed_block(w, tokens, final):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    put_tokens(w, tokens, canonical(FIXED_LL), canonical(FIXED_D))


def dynamic_block(w, tokens, ll_lens, d_lens, final, header_items=None, cl_lens=None):
    """header_items: the code-length symbols as (symbol, extra value) pairs; without them every length is sent on its own."""
    hlit, hdist = len(ll_lens), len(d_lens)
    assert 257 <= hlit <= 286 and 1 <= hdist <= 30
    if header_items is None:
        header_items = [(l, 0) for l in list(ll_lens) + list(d_lens)]
    if cl_lens is None:
        used = {s for s, _ in header_items}
        cl_lens = complete_lens(used | ({0, 1} - used if len(used) < 2 else set()), 19)
    hclen = max(k for k in range(19) if cl_lens[CL_ORDER[k]]) + 1
    hclen = max(hclen, 4)
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    w.bits(hclen - 4, 4)
    for k in range(hclen):
        w.bits(cl_lens[CL_ORDER[k]], 3)
    cl = canonical(cl_lens)
    for sym, extra in header_items:
        w.code(*cl[sym])
        if sym >= 16:
            w.bits(extra, {16: 2, 17: 3, 18: 7}[sym])
    put_tokens(w, tokens, canonical(ll_lens), canonical(d_lens))


def member(deflate, data, fextra=None, fname=None, fcomment=None, fhcrc=False, ftext=False, crc=None, isize=None):
    """RFC 1952 2.3: one gzip member around a raw deflate stream of `data`"""
    flg = (1 if ftext else 0) | (2 if fhcrc else 0) | (4 if fextra is not None else 0) | (8 if fname is not None else 0) | \
        (16 if fcomment is not None else 0)
    head = bytes([0x1f, 0x8b, 8, flg, 0, 0, 0, 0, 0, 0xff])
    if fextra is not None:
        head += struct.pack('<H', len(fextra)) + fextra
    if fname is not None:
        head += fname + b'\0'
    if fcomment is not None:
        head += fcomment + b'\0'
    if fhcrc:
        head += struct.pack('<H', zlib.crc32(head) & 0xffff)
    return head + deflate + struct.pack('<II', zlib.crc32(data) if crc is None else crc, (len(data) & 0xffffffff) if isize is None else isize)


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def gz(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, **kw):
    return member(raw_deflate(data, level, strategy), data, **kw)


def bgzf(data, block=20000):
    """SAMv1 4.1: BGZF blocks and the EOF block"""
    out = b''
    for a in list(range(0, len(data), block)) + [None]:
        chunk = b'' if a is None else data[a:a + block]
        d = raw_deflate(chunk)
        out += member(d, chunk, fextra=b'BC' + struct.pack('<HH', 2, len(d) + 25))
    return out


def fasta_text(rng, n_bases, name='seq1 some description'):
    seq = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, size=n_bases)].tobytes()
    return b'>' + name.encode() + b'\n' + b''.join(seq[a:a + 80] + b'\n' for a in range(0, n_bases, 80))


def _hand_built(rng):
    """(name, deflate stream, the bytes it stands for)"""
    out = []
    # a 15-bit code: lengths 1 .. 14, 15, 15 over 'A' .. 'O' and the end-of-block symbol
    ll = [0] * 257
    for k in range(15):
        ll[65 + k] = k + 1
    ll[256] = 15
    text = bytes(rng.integers(65, 80, size=200, dtype=np.uint8)) + b'ONMLKJIHGFEDCBA'
    w = BitWriter()
    dynamic_block(w, list(text), ll, [0], True)
    out.append(('code15', w.done(), text))
    # one distance code of one bit: the incomplete code RFC 1951 3.2.7 allows
    ll = complete_lens({120, 121, 256, 257 + 7, 257 + 28}, 286)
    w = BitWriter()
    dynamic_block(w, [120, 121, (10, 1), 120, (258, 1)], ll, [1], True)
    out.append(('one_distance_code', w.done(), b'xy' + b'y' * 10 + b'x' + b'x' * 258))
    # run symbols: 18 and 17 for the zeros, 16 repeating the length of symbol 256 into symbol 257 and on into the distance lengths
    ll = [0] * 258
    for s, l in ((97, 2), (98, 2), (99, 2), (256, 3), (257, 3)):
        ll[s] = l
    items = [(18, 97 - 11), (2, 0), (2, 0), (2, 0), (18, 138 - 11), (17, 10 - 3), (17, 8 - 3), (3, 0), (16, 6 - 3), (16, 3 - 3)]
    w = BitWriter()
    dynamic_block(w, [97, 98, 99, (3, 3), 99], ll, [3] * 8, True, header_items=items)
    out.append(('runs_across_boundary', w.done(), b'abcabcc'))
    # all literals: every byte value has a code, no length and no distance code is used
    text = bytes(range(256)) * 3 + bytes(rng.integers(0, 256, size=999, dtype=np.uint8))
    w = BitWriter()
    dynamic_block(w, list(text), complete_lens(set(range(257)), 257), [0], True)
    out.append(('all_literals', w.done(), text))
    # stored blocks of 0 and of 65535 bytes
    big = bytes(rng.integers(0, 256, size=65535, dtype=np.uint8))
    w = BitWriter()
    stored_block(w, b'', False)
    stored_block(w, big, False)
    stored_block(w, b'', True)
    out.append(('stored_0_65535', w.done(), big))
    # a match at distance exactly 32768 (zlib stops at 32506): 32768 stored bytes, then 258 of them again
    win = bytes(rng.integers(0, 256, size=32768, dtype=np.uint8))
    w = BitWriter()
    stored_block(w, win, False)
    fixed_block(w, [(258, 32768), 33, (3, 32768)], True)
    out.append(('distance_32768', w.done(), win + win[:258] + b'!' + win[259:262]))
    return out


def make_cases(seed=5):
    """-> list of dicts: name, gz (the stream), data (what it inflates to; None for a malformed stream), members, status"""
    rng = np.random.default_rng(seed)
    cases = []

    def valid(name, stream, data, members=1):
        cases.append(dict(name=name, gz=stream, data=data, members=members, status=OK))

    def bad(name, stream, status):
        cases.append(dict(name=name, gz=stream, data=None, members=None, status=status))

    sizes = (0, 1, 32767, 32768, 32769, 300_000)
    payload = {('fasta', n): fasta_text(rng, n)[:n] for n in sizes}
    payload.update({('random', n): bytes(rng.integers(0, 256, size=n, dtype=np.uint8)) for n in sizes})
    for (kind, n), data in payload.items():
        for level in (0, 1, 6, 9):
            valid(f'{kind}_{n}_l{level}', gz(data, level), data)
        valid(f'{kind}_{n}_fixed', gz(data, 6, zlib.Z_FIXED), data)
    run = b'a' * 100_000
    valid('run_of_one_byte', gz(run, 9), run)
    hand = _hand_built(rng)
    for name, d, data in hand:
        valid(name, member(d, data), data)
    # a final block that ends inside a byte, then a second member
    w = BitWriter()
    fixed_block(w, list(b'mid-byte'), True)
    assert w.n != 0
    text = fasta_text(rng, 5000)
    valid('mid_byte_then_member', member(w.done(), b'mid-byte') + gz(text), b'mid-byte' + text, members=2)
    # every header flag, alone and together
    small = fasta_text(rng, 1000, 'NZ_CP000001.1 Escherichia coli')
    valid('flag_ftext', gz(small, ftext=True), small)
    valid('flag_fextra', gz(small, fextra=b'AB\x03\x00xyz'), small)
    valid('flag_fextra_empty', gz(small, fextra=b''), small)
    valid('flag_fname', gz(small, fname=b'GCF_000005845.2_ASM584v2_genomic.fna'), small)
    valid('flag_fcomment', gz(small, fcomment=b'a comment'), small)
    valid('flag_fhcrc', gz(small, fhcrc=True), small)
    valid('flag_all', gz(small, ftext=True, fextra=b'AB\x01\x00q', fname=b'n.fna', fcomment=b'c', fhcrc=True), small)
    # several members; one of five is empty
    parts = [fasta_text(rng, n, f'contig{k}') for k, n in enumerate((40000, 0, 100, 70000, 33000))]
    valid('two_members', gz(parts[0]) + gz(parts[3], 1), parts[0] + parts[3], members=2)
    valid('five_members', b''.join(gz(p) if p else gz(b'') for p in parts[:1] + [b''] + parts[2:]), parts[0] + b''.join(parts[2:]), members=5)
    text = fasta_text(rng, 70000, 'bgzf')
    valid('bgzf_with_eof', bgzf(text), text, members=(len(text) + 19999) // 20000 + 1)
    valid('zero_padding', gz(small) + b'\0' * 1000, small)
    valid('empty_file', b'', b'', members=0)

    # ---- malformed ----
    body = fasta_text(rng, 20000)
    good = gz(body, fname=b'x.fna')
    bad('truncated_in_header', good[:12], TRUNCATED)
    bad('truncated_in_deflate', good[:len(good) // 2], TRUNCATED)
    bad('truncated_in_trailer', good[:-3], TRUNCATED)
    bad('truncated_second_member', gz(small) + good[:len(good) // 3], TRUNCATED)
    w = BitWriter()
    w.bits(1, 1)
    w.bits(3, 2)
    bad('block_type_3', member(w.done() + b'\0' * 8, b''), BAD_BLOCK)
    w = BitWriter()
    stored_block(w, b'hello', True, nlen=0x1234)
    bad('nlen_mismatch', member(w.done(), b'hello'), BAD_BLOCK)
    w = BitWriter()   # a code-length code of three one-bit codes
    for value, count in ((1, 1), (2, 2), (0, 5), (0, 5), (0, 4), (1, 3), (1, 3), (1, 3), (0, 3)):
        w.bits(value, count)
    bad('oversubscribed_code', member(w.done() + b'\0' * 8, b''), BAD_CODE)
    w = BitWriter()   # a literal/length code of two codes: one of one bit, one of two bits
    ll = [0] * 257
    ll[65], ll[256] = 1, 2
    dynamic_block(w, [65, 65], ll, [0], True)
    bad('incomplete_code', member(w.done(), b'AA'), BAD_CODE)
    w = BitWriter()
    fixed_block(w, [97, (3, 5)], True)
    bad('distance_before_start', member(w.done(), b'aaaa'), BAD_DISTANCE)
    w = BitWriter()   # the second member's window starts empty: the first member's bytes are out of reach
    fixed_block(w, [97, (3, 2)], True)
    bad('distance_into_previous_member', gz(small) + member(w.done(), b'aaaa'), BAD_DISTANCE)
    flipped = bytearray(good)
    flipped[-6] ^= 0x40
    bad('flipped_crc', bytes(flipped), BAD_CRC)
    bad('wrong_isize', gz(body, isize=len(body) + 1), BAD_SIZE)
    bad('trailing_garbage', good + b'garbage!', BAD_MAGIC)
    bad('not_gzip', b'>seq\nACGT\n', BAD_MAGIC)
    return cases
