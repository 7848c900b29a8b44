"""Host-side mirror of the reference's `nanofastq` read filter on top of libmpn.so.

/root/reference/bin/tools/nanofastq.c reads FASTA/FASTQ (kseq) on stdin and writes the reads that pass to stdout --
cropped by -h/-t, kept if the cropped length >= -l and (FASTQ only) the mean error-probability Phred score after cropping
>= -q -- and one statistics line per read to stderr: `read_id, length, avgQ, length_after_crop, avgQ_after_crop, passed`
(:228-238; read by /root/reference/bin/megapath_nano.py:1075).  `-r PREFIX` renames reads PREFIX1, PREFIX2, ...

Same contract here: `filter_fastx()` returns the two byte strings (and the surviving reads packed for the mapper, so that
they can go straight to the GPU); `bin/mpn-nanofastq` is the executable drop-in.  The error-probability sums come from
`mpn_fastq_qsum_batch` (bit-identical doubles, include/mpn_fastq.h); log10 and the `%.2f` formatting use the same libm /
printf rules as the C program.  Reproduced quirks: `-0.00` for a perfect-zero score, and the unsigned wrap-around of
`length - headcrop - tailcrop` in the fourth column when the crops exceed the read (:231-234).

Under MPN_READ_INGEST=device the filter streams (`filter_stream`, at the end of this module): the text goes to HBM through the read
path's sources and scan (ingest.py), the headers, the sums and the output text are made from the resident bytes
(mpn_fastq_heads / mpn_fastq_qsum_rows / mpn_fastq_emit, include/mpn_ingest.h), and only log10, `%.2f` and the verdict stay here, in
`decide()`, which `assemble()` runs as well.
"""
import ctypes as ct
import gzip
import io
import math

import numpy as np

from . import _ffi

PHRED_TABLE = np.array([math.pow(10.0, -i / 10.0) for i in range(128)], dtype=np.float64)   # nanofastq.c:147-149


def parse_fastx(data):
    """kseq-style records from a bytes object -> list of (name, comment or None, seq, qual or None), all bytes."""
    if data[:2] == b'\x1f\x8b':
        data = gzip.decompress(data)
    return _parse_text(data)


def _parse_text(data):
    """parse_fastx on bytes that are text whatever they start with (what the device path hands over in the middle of a stream)"""
    lines = data.split(b'\n')
    n, i, out = len(lines), 0, []
    while i < n:
        head = lines[i]
        if not head or head[:1] not in (b'>', b'@'):
            i += 1
            continue
        head = head[1:].rstrip(b'\r')
        cut = -1
        for k, ch in enumerate(head):
            if ch in (32, 9):
                cut = k
                break
        name, comment = (head, None) if cut < 0 else (head[:cut], head[cut + 1:])
        i += 1
        seq = []
        while i < n and lines[i][:1] not in (b'>', b'@', b'+'):
            seq.append(lines[i].rstrip(b'\r'))
            i += 1
        seq = b''.join(seq)
        qual = None
        if i < n and lines[i][:1] == b'+':
            i += 1
            q, got = [], 0
            while i < n and got < len(seq):
                ln = lines[i].rstrip(b'\r')
                q.append(ln)
                got += len(ln)
                i += 1
            qual = b''.join(q)
            if len(qual) != len(seq):
                raise ValueError(f'truncated quality string for read {name.decode(errors="replace")}')
        out.append((name, comment if comment else None, seq, qual))
    return out


def qsums(quals, head_crop, tail_crop, min_len):
    """-> (total, cropped) float64 arrays for a list of quality byte strings, from the HIP kernel."""
    lib = _ffi.lib()
    n = len(quals)
    total, cropped = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
    if n == 0:
        return total, cropped
    lens = np.array([len(q) for q in quals], dtype=np.int32)
    off = np.zeros(n, dtype=np.int64)
    np.cumsum(lens[:-1], out=off[1:])
    buf = np.frombuffer(b''.join(quals) + b'\0', dtype=np.uint8)
    status = np.zeros(n, dtype=np.uint8)
    P = ct.c_void_p
    lib.mpn_fastq_qsum_batch.argtypes = [ct.c_int32, P, P, P, ct.c_int32, ct.c_int32, ct.c_int32, P, P, P, P]
    lib.mpn_fastq_qsum_batch.restype = ct.c_int
    _ffi.check(lib.mpn_fastq_qsum_batch(n, buf.ctypes.data, off.ctypes.data, lens.ctypes.data, head_crop, tail_crop, min_len,
                                        PHRED_TABLE.ctypes.data, total.ctypes.data, cropped.ctypes.data, status.ctypes.data),
               'mpn_fastq_qsum_batch')
    if status.any():
        raise ValueError(f'read {int(np.flatnonzero(status)[0])} holds a quality character outside Phred+33')
    return total, cropped


def _phred(total_err, n):
    return -10 * math.log10(total_err / n)


def assemble(records, total, cropped, min_quality=0, min_length=0, head_crop=0, tail_crop=0, read_id_prefix=None, first=0):
    """The program's outputs from the parsed records and their error sums (shared with the oracle's checker).
    -> (stdout bytes, stderr bytes, kept: list of (name, cropped seq)).  first: the reads of the input in front of these records
    (-r numbers every read of the input)."""
    out, info, kept = _assemble(records, total, cropped, min_quality, min_length, head_crop, tail_crop, read_id_prefix, first)
    return out, info, [(n, s) for n, s, _ in kept]


def read_id(name, number, read_id_prefix):
    """the id a read is written and reported under: its own, or with -r the prefix and its number in the input, from 1 (:158-163)"""
    return name if read_id_prefix is None else read_id_prefix.encode() + str(number).encode()


def decide(rid, l, fq, total, cropped, min_quality, min_length, head_crop, tail_crop):
    """One read of l > 0 bases (fq: it has qualities, with these two error sums) -> (passed, its statistics line).  min_length is
    the program's: 1 where the option is 0 (nanofastq.c:127-130).  What the host and the device path share."""
    avg = _phred(total, l) if fq else 0.0                                         # :166-173
    avg_crop = 0.0
    passed = 1
    if l - tail_crop - head_crop < min_length:                                    # :182
        passed = 0
    else:
        if fq:
            avg_crop = _phred(cropped, l - head_crop - tail_crop)                 # :196
        if fq and avg_crop < min_quality:                                         # :199
            passed = 0
    n_crop = l - head_crop - tail_crop
    col4 = n_crop % (1 << 64) if n_crop != 0 else 0                               # size_t arithmetic, :231-234
    return passed, b'%s\t%d\t%s\t%d\t%s\t%d\n' % (rid, l, ('%.2f' % avg).encode(), col4, ('%.2f' % avg_crop).encode(), passed)


def _assemble(records, total, cropped, min_quality, min_length, head_crop, tail_crop, read_id_prefix, first=0):
    """assemble for records that are reads first + 1, first + 2, .. of their input; kept: (name, cropped seq, cropped qual or None)"""
    if min_length == 0:
        min_length = 1                                                           # nanofastq.c:127-130
    out, info, kept = [], [], []
    for k, (name, comment, seq, qual) in enumerate(records):
        rid = read_id(name, first + k + 1, read_id_prefix)
        fq = qual is not None
        passed, line = decide(rid, len(seq), fq, total[k], cropped[k], min_quality, min_length, head_crop, tail_crop)
        if passed:
            start, end = head_crop, len(seq) - tail_crop
            out.append((b'@' if fq else b'>') + rid + (b' ' + comment if comment else b'') + b'\n' + seq[start:end] + b'\n')
            if fq:
                out.append(b'+\n' + qual[start:end] + b'\n')
            kept.append((rid.decode(errors='replace'), seq[start:end], qual[start:end] if fq else None))
        info.append(line)
    return b''.join(out), b''.join(info), kept


def _check_options(min_quality, min_length, head_crop, tail_crop):
    if min(min_quality, min_length, head_crop, tail_crop) < 0:
        raise ValueError('negative option')                                       # nanofastq.c:122-126 prints the usage and exits


def _filter_records(records, opts, first=0):
    """parsed records -> _assemble's three values, the sums from mpn_fastq_qsum_batch"""
    min_quality, min_length, head_crop, tail_crop, read_id_prefix = opts
    for name, _, seq, _ in records:
        if len(seq) == 0:
            raise ValueError(f'empty read {name.decode(errors="replace")}: the reference divides by its length')
    idx = [k for k, r in enumerate(records) if r[3] is not None]
    total, cropped = np.zeros(len(records)), np.zeros(len(records))
    t, c = qsums([records[k][3] for k in idx], head_crop, tail_crop, max(min_length, 1))
    total[idx], cropped[idx] = t, c
    return _assemble(records, total, cropped, min_quality, min_length, head_crop, tail_crop, read_id_prefix, first)


def filter_fastx(data, min_quality=0, min_length=0, head_crop=0, tail_crop=0, read_id_prefix=None):
    """nanofastq on a bytes object.  -> (stdout bytes, stderr bytes, kept reads [(name, seq bytes)]).  Under MPN_READ_INGEST=device
    the bytes go through filter_stream."""
    from . import ingest
    _check_options(min_quality, min_length, head_crop, tail_crop)
    if ingest.read_ingest_mode() == 'device':
        out, info, kept = io.BytesIO(), io.BytesIO(), []
        for _ in _filter_stream(io.BytesIO(data), out, info, (min_quality, min_length, head_crop, tail_crop, read_id_prefix), 'cuda', None, None, kept):
            pass
        return out.getvalue(), info.getvalue(), kept
    out, info, kept = _filter_records(parse_fastx(data), (min_quality, min_length, head_crop, tail_crop, read_id_prefix))
    return out, info, [(n, s) for n, s, _ in kept]


# ---- the filter on the device (MPN_READ_INGEST=device) ---------------------------------------------------------------------------
# include/mpn_ingest.h has the three calls; the text sources, the scan and the batcher are ingest.py's.
FASTQ_HEAD = np.dtype([('off', '<i8'), ('id_len', '<i4'), ('comment_len', '<i4')])                                       # mpn_fastq_head
FASTQ_PICK = np.dtype([('start', '<i4'), ('m', '<i4'), ('with_comment', '<i4'), ('reserved', '<i4'), ('serial', '<i8')])  # mpn_fastq_pick
_bound = False


def _dev_lib():
    global _bound
    from . import ingest
    lib = ingest._lib()
    if not _bound:
        P, I64, I32 = ct.c_void_p, ct.c_int64, ct.c_int32
        lib.mpn_fastq_heads.argtypes = [P, I64, I64, P, P, P, I64]
        lib.mpn_fastq_heads.restype = I32
        lib.mpn_fastq_qsum_rows.argtypes = [P, I64, I64, P, P, I32, I32, I32, P, P, P, P]
        lib.mpn_fastq_qsum_rows.restype = I32
        lib.mpn_fastq_emit.argtypes = [P, I64, I64, P, P, P, ct.c_char_p, I32, P, P, I64]
        lib.mpn_fastq_emit.restype = I32
        lib.mpn_fastq_filter_last_device_ms.argtypes = [ct.POINTER(ct.c_double)] * 3
        lib.mpn_fastq_filter_last_device_ms.restype = None
        lib.mpn_name_set_create.argtypes = [I64, P, P, I64, ct.POINTER(P), P]
        lib.mpn_name_set_create.restype = I32
        lib.mpn_name_set_free.argtypes = [P]
        lib.mpn_name_set_free.restype = None
        lib.mpn_fastq_name_lookup.argtypes = [P, I64, I64, P, P, P]
        lib.mpn_fastq_name_lookup.restype = I32
        lib.mpn_fastq_lookup_last_device_ms.argtypes = [ct.POINTER(ct.c_double)]
        lib.mpn_fastq_lookup_last_device_ms.restype = None
        _bound = True
    return lib


def last_filter_device_ms():
    """-> (heads ms, sums ms, emit ms) of the calling thread's last native calls"""
    v = [ct.c_double(0) for _ in range(3)]
    _dev_lib().mpn_fastq_filter_last_device_ms(*[ct.byref(x) for x in v])
    return tuple(x.value for x in v)


def fastq_heads(text, text_len, rows, with_ids=True):
    """mpn_fastq_heads on rows of ingest.fastq_scan (unmoved) -> (heads as a FASTQ_HEAD array, the ids as a list of bytes or None)"""
    from . import ingest
    lib = _dev_lib()
    rows = np.ascontiguousarray(rows, dtype=ingest.FASTQ_ROW)
    heads = np.zeros(len(rows), dtype=FASTQ_HEAD)
    # the scan's name is the id in all but odd headers: a pool of that size is enough at the first attempt
    cap = int(rows['name_len'].astype(np.int64).sum()) + 64 if with_ids else 0
    while True:
        pool = np.zeros(max(cap, 1), dtype=np.uint8) if with_ids else None
        rc = lib.mpn_fastq_heads(text.data_ptr(), int(text_len), len(rows), rows.ctypes.data, heads.ctypes.data,
                                 pool.ctypes.data if with_ids else None, cap)
        if rc == -3 and int(heads['id_len'].astype(np.int64).sum()) > cap:
            cap = int(heads['id_len'].astype(np.int64).sum())
            continue
        if rc:
            raise _ffi.MpnError(f'mpn_fastq_heads rc={rc}: {_ffi.hint(_ffi.last_error())}')
        break
    if not with_ids:
        return heads, None
    raw, ends = pool.tobytes(), np.cumsum(heads['id_len'].astype(np.int64))
    return heads, [raw[e - l:e] for e, l in zip(ends.tolist(), heads['id_len'].tolist())]


class NameSet:
    """mpn_name_set_create: a list of names (bytes) as a hash table in HBM.  first_of[i]: the smallest index with the bytes of
    name i.  slots: 0 for the default size, or a power of two larger than the number of distinct names.  close() frees the device
    memory (also a context manager)."""

    def __init__(self, names, slots=0):
        lib = _dev_lib()
        names = list(names)
        off = np.zeros(len(names) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in names], out=off[1:])
        pool = b''.join(names)
        self.first_of = np.zeros(len(names), dtype=np.int32)
        self.n, self._set = len(names), ct.c_void_p()
        rc = lib.mpn_name_set_create(len(names), pool, off.ctypes.data, int(slots), ct.byref(self._set), self.first_of.ctypes.data)
        if rc:
            self._set = None
            raise _ffi.MpnError(f'mpn_name_set_create rc={rc}: {_ffi.hint(_ffi.last_error())}')

    def close(self):
        if self._set is not None:
            _dev_lib().mpn_name_set_free(self._set)
            self._set = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def last_lookup_device_ms():
    """-> the device ms of the calling thread's last mpn_fastq_name_lookup"""
    v = ct.c_double(0)
    _dev_lib().mpn_fastq_lookup_last_device_ms(ct.byref(v))
    return v.value


def fastq_name_lookup(text, text_len, heads, name_set):
    """mpn_fastq_name_lookup -> found (int32 per head): the smallest index of name_set's list whose bytes are the record's id, or -1"""
    lib = _dev_lib()
    heads = np.ascontiguousarray(heads, dtype=FASTQ_HEAD)
    found = np.zeros(len(heads), dtype=np.int32)
    rc = lib.mpn_fastq_name_lookup(text.data_ptr(), int(text_len), len(heads), heads.ctypes.data, name_set._set, found.ctypes.data)
    if rc:
        raise _ffi.MpnError(f'mpn_fastq_name_lookup rc={rc}: {_ffi.hint(_ffi.last_error())}')
    return found


def qsum_rows(text, text_len, rows, head_crop, tail_crop, min_len, by_length=False):
    """mpn_fastq_qsum_rows -> (total, cropped, status).  by_length: reads of similar length share a wave.  The results do not depend
    on it, and it is off: on 50 000 ONT-like reads every wave is resident at once, the launch lasts as long as the longest read
    either way, and the ordering measured slower (profiles/r18_read_filter/README.md)."""
    from . import ingest
    lib = _dev_lib()
    rows = np.ascontiguousarray(rows, dtype=ingest.FASTQ_ROW)
    n = len(rows)
    total, cropped, status = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.uint8)
    order = np.argsort(rows['len'], kind='stable').astype(np.int32) if by_length else None
    big = 0x7fffffff          # a crop past any read is the same crop at 2^31 - 1: no read is longer
    rc = lib.mpn_fastq_qsum_rows(text.data_ptr(), int(text_len), n, rows.ctypes.data, order.ctypes.data if by_length else None,
                                 min(head_crop, big), min(tail_crop, big), min(min_len, big), PHRED_TABLE.ctypes.data, total.ctypes.data,
                                 cropped.ctypes.data, status.ctypes.data)
    if rc:
        raise _ffi.MpnError(f'mpn_fastq_qsum_rows rc={rc}: {_ffi.hint(_ffi.last_error())}')
    return total, cropped, status


def record_sizes(heads, picks, prefix_len=0):
    """the bytes mpn_fastq_emit writes per record (int64 array)"""
    serial = picks['serial']
    digits = np.zeros(len(picks), dtype=np.int64)
    s = serial.copy()
    while (s > 0).any():
        digits += s > 0
        s //= 10
    id_len = np.where(serial > 0, prefix_len + digits, heads['id_len'].astype(np.int64))
    com = np.where(picks['with_comment'] != 0, 1 + np.maximum(heads['comment_len'].astype(np.int64), 0), 0)
    return 1 + id_len + com + 1 + 2 * picks['m'].astype(np.int64) + 4


def fastq_emit(text, text_len, rows, heads, picks, prefix=b''):
    """mpn_fastq_emit -> (uint8 device tensor that starts with the records' text, out_off [n + 1])"""
    import torch
    from . import ingest
    lib = _dev_lib()
    rows = np.ascontiguousarray(rows, dtype=ingest.FASTQ_ROW)
    heads, picks = np.ascontiguousarray(heads, dtype=FASTQ_HEAD), np.ascontiguousarray(picks, dtype=FASTQ_PICK)
    out_off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(record_sizes(heads, picks, len(prefix)), out=out_off[1:])
    d_out = torch.empty(max(ingest._align16(int(out_off[-1])), 16), dtype=torch.uint8, device=text.device)
    rc = lib.mpn_fastq_emit(text.data_ptr(), int(text_len), len(rows), rows.ctypes.data, heads.ctypes.data, picks.ctypes.data, prefix, len(prefix),
                            out_off.ctypes.data, d_out.data_ptr(), d_out.numel())
    if rc:
        raise _ffi.MpnError(f'mpn_fastq_emit rc={rc}: {_ffi.hint(_ffi.last_error())}')
    return d_out, out_off


def _open_texts(stream, device, timings):
    """-> (ingest's text source for the stream, the stream the host reads the rest from if it has to; both None where the host takes
    the stream from its first byte: it is empty, or its text does not start with '@')"""
    from . import fastx, ingest
    if not hasattr(stream, 'peek'):
        stream = io.BufferedReader(stream, buffer_size=1 << 20)
    kind, first = fastx.query_form(stream.peek(1 << 16))
    if kind not in ('plain', 'gzip', 'bgzf') or first != b'@':
        return None, None, stream
    if kind == 'bgzf':
        return ingest._BgzfTexts(stream, device, timings), None, stream
    rest = stream if kind == 'plain' else fastx.gzip_text(stream)
    return ingest._ChunkTexts(rest, device, timings, 'read' if kind == 'plain' else 'inflate'), rest, stream


def filter_stream(stream, out, info, min_quality=0, min_length=0, head_crop=0, tail_crop=0, read_id_prefix=None, device='cuda', timings=None,
                  batches=None):
    """nanofastq as a stream, on the device: `stream` holds a file's own bytes (plain, gzip or BGZF: told as fastx.open_query tells
    them); the kept records go to `out` and the statistics lines to `info` (binary streams) text by text
    (MPN_INGEST_BATCH_BYTES), so neither the input nor the output is ever whole in memory.  Per text in HBM: ingest.fastq_scan,
    mpn_fastq_heads and mpn_fastq_qsum_rows, the decisions and lines here (decide(), the code assemble() runs), mpn_fastq_emit, one
    download.  From the first record the scan does not take (FASTA, multi-line FASTQ, ..) the rest of the stream goes through
    parse_fastx and the host's sums, with the read numbers running on; so does a stream that does not start with '@'.  An empty
    read or a quality character outside Phred+33 raises the host path's ValueError; what was written for the texts before stays
    written.

    Without `batches` the stream is filtered when the call returns, and the call returns (reads, reads kept).  With an
    ingest.ReadBatcher the kept reads, cropped, are also added to it under the ids that were written, and the call returns a
    GENERATOR of the mapper.PackedReads that became full (the last batch stays in the batcher: batches.flush())."""
    _check_options(min_quality, min_length, head_crop, tail_crop)
    opts = (min_quality, min_length, head_crop, tail_crop, read_id_prefix)
    if batches is not None:
        return _filter_stream(stream, out, info, opts, device or 'cuda', timings, batches, None)
    count = {}
    for _ in _filter_stream(stream, out, info, opts, device or 'cuda', timings, None, None, count):
        pass
    return count.get('reads', 0), count.get('kept', 0)


def _filter_stream(stream, out, info, opts, device, timings, batches, kept, count=None):
    """filter_stream's generator.  kept: None, or a list that receives (id, cropped bases) of the reads that pass; count: None, or
    a dict that receives the numbers of reads and of reads kept."""
    import time
    from . import fastx, ingest
    tick = ingest._tick
    min_quality, min_length, head_crop, tail_crop, read_id_prefix = opts
    min_len = max(min_length, 1)
    prefix = b'' if read_id_prefix is None else read_id_prefix.encode()
    texts, rest, stream = _open_texts(stream, device, timings)
    number, carry = 0, None          # number: the reads before the next one (-r serials count every read of the input)

    def on_host(data):
        t0 = time.perf_counter()
        records = parse_fastx(data) if texts is None else _parse_text(data)
        o, i, kp = _filter_records(records, opts, number)
        out.write(o)
        info.write(i)
        tick(count, 'reads', len(records))
        tick(count, 'kept', len(kp))
        for name, seq, qual in kp:
            if kept is not None:
                kept.append((name, seq))
            if batches is not None:
                yield from batches.add_host(name, seq, qual)
        tick(timings, 'host', time.perf_counter() - t0)

    if texts is None:
        yield from on_host(stream.read())
        return
    while True:
        text, text_len, final = texts.next_text(carry)
        t0 = time.perf_counter()
        rows, consumed, status, ms = ingest.fastq_scan(text, text_len, final)
        t1 = time.perf_counter()
        tick(timings, 'scan', t1 - t0)
        tick(timings, 'scan_device_ms', ms)
        tick(timings, 'records', len(rows))
        n = len(rows)
        if n:
            heads, ids = fastq_heads(text, text_len, rows, with_ids=read_id_prefix is None)
            t2 = time.perf_counter()
            tick(timings, 'heads', t2 - t1)
            tick(timings, 'heads_device_ms', last_filter_device_ms()[0])
            total, cropped, bad = qsum_rows(text, text_len, rows, head_crop, tail_crop, min_len)
            t3 = time.perf_counter()
            tick(timings, 'sums', t3 - t2)
            tick(timings, 'sums_device_ms', last_filter_device_ms()[1])
            lens = rows['len'].tolist()
            if 0 in lens:
                k = lens.index(0)
                name = ids[k] if ids is not None else b'%d' % (number + k + 1)
                raise ValueError(f'empty read {name.decode(errors="replace")}: the reference divides by its length')
            if bad.any():
                raise ValueError(f'read {number + int(np.flatnonzero(bad)[0])} holds a quality character outside Phred+33')
            lines, keep, rids = [], [], []
            for k, (l, t, c) in enumerate(zip(lens, total, cropped)):
                rid = read_id(ids[k] if ids is not None else None, number + k + 1, read_id_prefix)
                passed, line = decide(rid, l, True, t, c, min_quality, min_len, head_crop, tail_crop)
                lines.append(line)
                if passed:
                    keep.append(k)
                    rids.append(rid)
            t4 = time.perf_counter()
            tick(timings, 'decide', t4 - t3)
            keep = np.array(keep, dtype=np.int64)
            picks = np.zeros(len(keep), dtype=FASTQ_PICK)
            picks['start'] = head_crop
            picks['m'] = rows['len'][keep] - head_crop - tail_crop
            picks['with_comment'] = heads['comment_len'][keep] > 0                # nanofastq.c:218-224
            if read_id_prefix is not None:
                picks['serial'] = number + keep + 1
            d_out, out_off = fastq_emit(text, text_len, rows[keep], heads[keep], picks, prefix)
            t5 = time.perf_counter()
            tick(timings, 'emit', t5 - t4)
            tick(timings, 'emit_device_ms', last_filter_device_ms()[2])
            written = d_out[:int(out_off[-1])].cpu().numpy()
            t6 = time.perf_counter()
            tick(timings, 'd2h', t6 - t5)
            out.write(memoryview(written))
            info.write(b''.join(lines))
            tick(timings, 'write', time.perf_counter() - t6)
            tick(count, 'reads', n)
            tick(count, 'kept', len(keep))
            if kept is not None:
                for rid, a, m in zip(rids, (out_off[1:] - 2 * picks['m'] - 4).tolist(), picks['m'].tolist()):
                    kept.append((rid.decode(errors='replace'), written[a:a + m].tobytes()))
            if batches is not None and len(keep):
                cut = rows[keep].copy()           # the rows of the cropped reads: mpn_fastq_gather takes any rows inside the text
                cut['seq_off'] += head_crop
                cut['qual_off'] += head_crop
                cut['len'] = picks['m']
                yield from batches.add_rows(text, text_len, cut, names=[r.decode(errors='replace') for r in rids])
            number += n
        if status == ingest.FASTQ_UNSUPPORTED:
            # the rest of the stream for the host: parse_fastx is stateless at a record start
            tail = text[consumed:text_len].cpu().numpy().tobytes()
            del text, rows, carry
            host = ingest._TailThenStream(tail, rest if rest is not None else fastx.gzip_text(stream))
            yield from on_host(host.read())
            break
        if status != ingest.OK:
            raise _ffi.MpnError(f'mpn_fastq_scan: status {status}')
        if final:
            break
        carry = text[consumed:text_len]
