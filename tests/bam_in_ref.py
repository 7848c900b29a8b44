"""The restatement of BAM read input (test infrastructure): what `samtools fastq` makes of a BAM file, written from the SAM/BAM
specification with gzip, struct and plain Python, and the statuses include/mpn_ingest.h gives malformed text.

    inflate(file bytes) -> text          gzip.decompress: BGZF blocks are gzip members
    walk(text)          -> rows          one dict per record, in file order; BamError(status, offset) for malformed text
    reads(text)         -> [(name, bases, qualities or None)]   records with flag & 0x900 dropped, flag & 0x10 restored
    batches(reads, batch_bases) -> [Batch]   cut as aligner.iter_read_batches cuts; buffers as mapper.PackedReads lays them out
"""
import gzip
import struct

import numpy as np

OK, TRUNCATED, BAD_MAGIC, BAD_HEADER, BAD_RECORD = 0, 10, 11, 12, 13
CODES = '=ACMGRSVTWYHKDBN'
COMPLEMENT = bytes.maketrans(b'ACMGRSVTWYHKDBN=', b'TGKCYSBAWRDMHVN=')


class BamError(Exception):
    def __init__(self, status, offset):
        super().__init__(f'status {status} at {offset}')
        self.status, self.offset = status, offset


def inflate(blob):
    return gzip.decompress(blob) if blob else b''


def header_end(text):
    """-> the offset of the first record"""
    if text[:4] != b'BAM\1'[:len(text[:4])]:
        raise BamError(BAD_MAGIC, 0)
    if len(text) < 8:
        raise BamError(TRUNCATED, 0)
    l_text, = struct.unpack_from('<i', text, 4)
    if l_text < 0:
        raise BamError(BAD_HEADER, 0)
    p = 8 + l_text
    if p + 4 > len(text):
        raise BamError(TRUNCATED, 0)
    n_ref, = struct.unpack_from('<i', text, p)
    if n_ref < 0:
        raise BamError(BAD_HEADER, 0)
    p += 4
    for _ in range(n_ref):
        if p + 4 > len(text):
            raise BamError(TRUNCATED, 0)
        l_name, = struct.unpack_from('<i', text, p)
        if l_name < 1:
            raise BamError(BAD_HEADER, 0)
        p += 8 + l_name
        if p > len(text):
            raise BamError(TRUNCATED, 0)
    return p


def walk(text, rows=None):
    """-> list of rows.  A BamError leaves the rows before the offending record in `rows` when the caller passes a list."""
    rows = [] if rows is None else rows
    p = header_end(text)
    while p < len(text):
        if p + 4 > len(text):
            raise BamError(TRUNCATED, p)
        block_size, = struct.unpack_from('<i', text, p)
        if block_size < 32:
            raise BamError(BAD_RECORD, p)
        if p + 4 + block_size > len(text):
            raise BamError(TRUNCATED, p)
        l_read_name, = struct.unpack_from('<B', text, p + 12)
        n_cigar, flag, l_seq = struct.unpack_from('<HHi', text, p + 16)
        if l_read_name < 1 or l_seq < 0:
            raise BamError(BAD_RECORD, p)
        seq = p + 36 + l_read_name + 4 * n_cigar
        qual = seq + (l_seq + 1) // 2
        if qual + l_seq > p + 4 + block_size:
            raise BamError(BAD_RECORD, p)
        rows.append(dict(off=p, l_seq=l_seq, flag=flag, l_read_name=l_read_name, has_qual=int(l_seq > 0 and text[qual] != 0xFF), seq=seq, qual=qual))
        p += 4 + block_size
    return rows


def read_of(text, row):
    name = text[row['off'] + 36:row['off'] + 36 + row['l_read_name'] - 1].decode()
    packed, n = text[row['seq']:row['qual']], row['l_seq']
    bases = ''.join(CODES[(packed[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(n)).encode()
    quals = bytes((q + 33) & 0xFF for q in text[row['qual']:row['qual'] + n]) if row['has_qual'] else None
    if row['flag'] & 0x10:
        bases = bases[::-1].translate(COMPLEMENT)
        quals = quals[::-1] if quals is not None else None
    return name, bases, quals


def reads(text):
    return [read_of(text, r) for r in walk(text) if not r['flag'] & 0x900]


class Batch:
    def __init__(self, recs):
        self.names = [r[0] for r in recs]
        self.lens = np.array([len(r[1]) for r in recs], dtype=np.int32)
        self.off = np.zeros(len(recs), dtype=np.int64)
        self.off[1:] = np.cumsum(self.lens[:-1].astype(np.int64))
        total = int(self.lens.astype(np.int64).sum())
        self.buf = np.zeros(total + 16, dtype=np.uint8)
        self.buf[:total] = np.frombuffer(b''.join(r[1] for r in recs), dtype=np.uint8)
        self.qbuf = None
        if any(r[2] is not None for r in recs):      # PackedReads' rule: '!' for the reads without qualities in a batch that has some
            self.qbuf = np.zeros(total + 16, dtype=np.uint8)
            self.qbuf[:total] = np.frombuffer(b''.join(r[2] if r[2] is not None else b'!' * len(r[1]) for r in recs), dtype=np.uint8)


def batches(recs, batch_bases):
    out, cur, acc = [], [], 0
    for r in recs:
        if cur and acc + len(r[1]) > batch_bases:
            out.append(Batch(cur))
            cur, acc = [], 0
        cur.append(r)
        acc += len(r[1])
    if cur:
        out.append(Batch(cur))
    return out


def fastq_text(recs):
    """the reads as the FASTQ file that is equivalent to the BAM (every read needs qualities)"""
    return b''.join(b'@' + n.encode() + b'\n' + s + b'\n+\n' + q + b'\n' for n, s, q in recs)
