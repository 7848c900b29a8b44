"""A plain restatement of the two definitions the read filter on the device adds (include/mpn_ingest.h): the header of a record as
the host filter reads it (mpn_fastq_heads) and the text of the records that are written (mpn_fastq_emit).

heads_ref(text, rows) -> [(off, id_len, comment_len)] per row of a scan of `text` (fastq_scan_ref.scan), comment_len = -1 for a
header without a blank or TAB.  emit_ref(text, rows, heads, picks, prefix) -> the bytes of the output; picks: (start, m,
with_comment, serial) per record.  sizes_ref: the size of every record, whose exclusive sum mpn_fastq_emit takes as out_off.
"""
import numpy as np

HEAD = np.dtype([('off', '<i8'), ('id_len', '<i4'), ('comment_len', '<i4')])
PICK = np.dtype([('start', '<i4'), ('m', '<i4'), ('with_comment', '<i4'), ('reserved', '<i4'), ('serial', '<i8')])


def heads_ref(text, rows):
    text = bytes(text)
    out = []
    for w in rows:
        lf = int(w['seq_off']) - 1                       # the line feed that ends the header line
        s = text.rfind(b'\n', 0, lf) + 1                 # behind the line feed before it, or 0
        a = min(s + 1, lf)                               # behind the '@'
        e = lf - 1 if lf > a and text[lf - 1] == 13 else lf
        head = text[a:e]
        cut = min((head.find(c) for c in (b' ', b'\t') if c in head), default=-1)
        out.append((a, len(head), -1) if cut < 0 else (a, cut, len(head) - cut - 1))
    return np.array(out, dtype=HEAD)


def picks_of(items):
    """[(start, m, with_comment, serial)] -> the array mpn_fastq_emit takes"""
    p = np.zeros(len(items), dtype=PICK)
    for k, (start, m, com, serial) in enumerate(items):
        p[k] = (start, m, com, 0, serial)
    return p


def record_ref(text, w, h, pick, prefix=b''):
    start, m, com, serial = (int(pick[k]) for k in ('start', 'm', 'with_comment', 'serial'))
    off, id_len, com_len = int(h['off']), int(h['id_len']), int(h['comment_len'])
    rid = prefix + str(serial).encode() if serial > 0 else text[off:off + id_len]
    comment = b' ' + text[off + id_len + 1:off + id_len + 1 + max(com_len, 0)] if com else b''
    so, qo = int(w['seq_off']) + start, int(w['qual_off']) + start
    return b'@' + rid + comment + b'\n' + text[so:so + m] + b'\n+\n' + text[qo:qo + m] + b'\n'


def emit_ref(text, rows, heads, picks, prefix=b''):
    text = bytes(text)
    return b''.join(record_ref(text, w, h, p, prefix) for w, h, p in zip(rows, heads, picks))


def sizes_ref(text, rows, heads, picks, prefix=b''):
    text = bytes(text)
    return np.array([len(record_ref(text, w, h, p, prefix)) for w, h, p in zip(rows, heads, picks)], dtype=np.int64)
