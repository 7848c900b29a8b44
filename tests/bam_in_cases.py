"""A small BAM / BGZF writer for the tests of BAM read input (struct + zlib, written from the SAM/BAM specification), which lets a case
choose where the blocks are cut, and the cases themselves: well-formed files (`files()`) and malformed texts (`malformed_texts()`)."""
import struct
import zlib

import numpy as np

CODES = '=ACMGRSVTWYHKDBN'
NIBBLE = {c: i for i, c in enumerate(CODES)}
OK, TRUNCATED, BAD_MAGIC, BAD_HEADER, BAD_RECORD = 0, 10, 11, 12, 13
EOF_BLOCK = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')
BGZF_MAX = 0xff00


def record(name, seq, qual=None, flag=0, n_cigar=0, tags=b'', block_size=None, l_seq=None, l_read_name=None):
    """One BAM record with its block_size word.  seq: a string over CODES in STORED orientation; qual: Phred bytes of its length,
    or None (0xFF).  block_size / l_seq / l_read_name: a value to store instead of the true one (malformed cases)."""
    name = name.encode() + b'\0'
    n = len(seq)
    nib = [NIBBLE[c] for c in seq] + [0]
    packed = bytes(nib[i] << 4 | nib[i + 1] for i in range(0, n, 2))
    q = bytes(qual) if qual is not None else b'\xff' * n
    assert len(q) == n
    body = (struct.pack('<iiBBHHHiiii', -1, -1, len(name) if l_read_name is None else l_read_name, 0, 4680, n_cigar, flag,
                        n if l_seq is None else l_seq, -1, -1, 0) + name + struct.pack('<%dI' % n_cigar, *[(10 << 4) | 4] * n_cigar) + packed + q + tags)
    return struct.pack('<i', len(body) if block_size is None else block_size) + body


def header(text=b'', refs=()):
    out = b'BAM\1' + struct.pack('<i', len(text)) + text + struct.pack('<i', len(refs))
    for name, length in refs:
        out += struct.pack('<i', len(name) + 1) + name.encode() + b'\0' + struct.pack('<i', length)
    return out


def bgzf_block(payload, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    data = c.compress(payload) + c.flush()
    assert len(payload) <= 1 << 16 and len(data) + 26 <= 1 << 16
    return (b'\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0' + struct.pack('<H', len(data) + 25) + data +
            struct.pack('<II', zlib.crc32(payload) & 0xffffffff, len(payload)))


def bgzf(text, cuts=(), eof=True, empty_at=(), level=6, max_block=BGZF_MAX):
    """text -> BGZF file bytes.  A block ends at every offset of `cuts` (and wherever a block would pass max_block); an empty block
    is put in front of the block that starts at an offset of `empty_at`."""
    edges = sorted({c for c in cuts if 0 < c < len(text)} | {0, len(text)})
    out = b''
    for a, b in zip(edges[:-1], edges[1:]):
        for p in range(a, b, max_block):
            if p in empty_at:
                out += bgzf_block(b'', level)
            out += bgzf_block(text[p:min(p + max_block, b)], level)
    return out + (EOF_BLOCK if eof else b'')


def _seq(rng, n):
    return ''.join(CODES[i] for i in rng.integers(0, 16, size=n))


def _qual(rng, n):
    q = rng.integers(0, 94, size=n).astype(np.uint8)
    q[:2] = [0, 93][:n]
    return q.tobytes()


LENGTHS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 70000)


def main_records(seed=5):
    """-> list of record bytes: every length of LENGTHS forward and reverse, all 16 codes in both orientations, qualities 0 and
    93, absent qualities in some records, names of 1 and 254 bytes, a 100 KB B tag, secondary and supplementary records between
    kept ones, records with CIGAR operations."""
    rng = np.random.default_rng(seed)
    recs = [record('n', CODES, _qual(rng, 16)), record('m' * 254, CODES + CODES[::-1], _qual(rng, 32), flag=0x10)]
    for k, n in enumerate(LENGTHS):
        for flag in (0, 0x10):
            quals = None if (k % 5 == 3 and flag) else _qual(rng, n)
            recs.append(record(f'len{n}_{flag}', _seq(rng, n), quals, flag=flag | (0x4 if k % 2 else 0), n_cigar=k % 3))
        if k % 4 == 1:
            recs.append(record(f'secondary{k}', _seq(rng, 40), _qual(rng, 40), flag=0x100 | (0x10 if k % 8 == 1 else 0)))
            recs.append(record(f'supplementary{k}', _seq(rng, 33), _qual(rng, 33), flag=0x800))
    big_tag = b'ZZBC' + struct.pack('<I', 100_000) + rng.integers(0, 256, size=100_000).astype(np.uint8).tobytes()
    recs.insert(9, record('big_tag', _seq(rng, 301), _qual(rng, 301), flag=0x10, tags=big_tag))
    recs.append(record('last_odd', _seq(rng, 77), _qual(rng, 77), flag=0x10, tags=b'NMC\x05'))
    return recs


def offsets(head, recs):
    """-> the offset of every record in the text head + records, and the end"""
    out, p = [], len(head)
    for r in recs:
        out.append(p)
        p += len(r)
    return out + [p]


def files():
    """-> dict name -> dict(blob=file bytes, text=its BAM text)"""
    rng = np.random.default_rng(11)
    long_text = b'@HD\tVN:1.6\tSO:unsorted\n' + b''.join(b'@CO\t' + bytes(rng.integers(65, 91, size=95).astype(np.uint8)) + b'\n' for _ in range(700))
    assert len(long_text) > 1 << 16
    refs7 = [(f'ref{i}' + 'x' * (i * 37), 1000 + i) for i in range(7)]
    recs = main_records()
    out = {}

    def add(name, text, **kw):
        out[name] = dict(blob=bgzf(text, **kw), text=text)
    head = header(long_text, refs7)
    text = head + b''.join(recs)
    offs = offsets(head, recs)
    add('main', text)
    # block ends inside a block_size word, inside the fixed fields, inside the packed bases, exactly at a record end, inside the
    # header's l_text, its text and a reference entry
    r70k = next(i for i, r in enumerate(recs) if b'len70000_16' in r[:60])
    cuts = [2, 6, 5000, len(head) - 9, offs[3] + 2, offs[4] + 21, offs[5] + 36 + 9 + 4 + 3, offs[6], offs[7], offs[r70k] + 10000, offs[r70k] + 40000, offs[-2] + 1]
    add('cuts', text, cuts=cuts, empty_at={offs[6], cuts[2]})
    add('no_eof', text, eof=False, max_block=30000)
    add('stored', text, level=0, max_block=65000)
    short = header(b'', ())
    few = [record('a', 'ACGT', None), record('b', 'TTTTTTTTTTTTTTTTTTTTG', None, flag=0x10), record('c', '', None), record('d', 'N' * 40, None)]
    add('no_quals', short + b''.join(few))
    add('header_only', header(b'@CO\tnothing\n', refs7[:1]))
    add('only_empty_reads', short + record('e1', '', None) + record('e2', '', None, flag=0x10))
    return out


def malformed_texts():
    """-> list of (name, text, status, offset of the offending header or record, records before it)"""
    head = header(b'@CO\tx\n', [('chr', 10)])
    good = [record('g1', 'ACGTN', bytes(5)), record('g2', 'GGC', None, flag=0x10)]
    pre = head + b''.join(good)
    at = len(pre)
    last = record('tail', 'ACGTACGTAC', bytes(10))
    cases = [
        ('block_size_31', pre + record('x', '', None, block_size=31), BAD_RECORD, at, 2),
        ('block_size_negative', pre + record('x', 'AC', None, block_size=-5), BAD_RECORD, at, 2),
        ('l_seq_negative', pre + record('x', 'ACGT', None, l_seq=-1) + last, BAD_RECORD, at, 2),
        ('l_seq_too_long', pre + record('x', 'ACGT', None, l_seq=1000) + last, BAD_RECORD, at, 2),
        ('l_seq_huge', pre + record('x', 'ACGT', None, l_seq=0x7fffffff) + last, BAD_RECORD, at, 2),
        ('l_read_name_0', pre + record('x', 'ACGT', None, l_read_name=0) + last, BAD_RECORD, at, 2),
        ('name_longer_than_record', pre + record('x', '', None, l_read_name=200) + last, BAD_RECORD, at, 2),
        ('cigar_longer_than_record', pre + record('x', 'ACGT', None)[:16] + struct.pack('<H', 60000) + record('x', 'ACGT', None)[18:] + last, BAD_RECORD, at, 2),
        ('truncated_last_record', pre + last[:-3], TRUNCATED, at, 2),
        ('truncated_in_block_size', pre + last[:2], TRUNCATED, at, 2),
        ('block_size_past_the_end', pre + record('x', 'ACGT', None, block_size=1 << 30), TRUNCATED, at, 2),
        ('wrong_magic', b'BAM\2' + pre[4:], BAD_MAGIC, 0, 0),
        ('cram_magic', b'CRAM' + pre[4:], BAD_MAGIC, 0, 0),
        ('l_text_negative', b'BAM\1' + struct.pack('<i', -4) + pre[8:], BAD_HEADER, 0, 0),
        ('l_text_past_the_end', b'BAM\1' + struct.pack('<i', 1 << 30) + pre[8:], TRUNCATED, 0, 0),
        ('n_ref_negative', header(b'@CO\tx\n', ())[:-4] + struct.pack('<i', -1) + b''.join(good), BAD_HEADER, 0, 0),
        ('n_ref_past_the_end', header(b'', ())[:-4] + struct.pack('<i', 1 << 30), TRUNCATED, 0, 0),
        ('l_name_0', header(b'', ())[:-4] + struct.pack('<ii', 1, 0) + b'\0' * 8 + b''.join(good), BAD_HEADER, 0, 0),
        ('l_name_past_the_end', header(b'', ())[:-4] + struct.pack('<ii', 1, 1 << 30) + b''.join(good), TRUNCATED, 0, 0),
        ('header_cut', head[:-3], TRUNCATED, 0, 0),
        ('two_bytes', b'BA', TRUNCATED, 0, 0),
        ('empty', b'', TRUNCATED, 0, 0),
    ]
    return cases
