"""Target ingestion on the GPU (MPN_TARGET_INGEST=device): the files of a target set go from compressed bytes on disk to resident
index parts without existing as host strings.  include/mpn_ingest.h has the two native calls; this module groups the files, sizes the
slots, takes the fallbacks and cuts the parts.

    files --read--> pinned buffer --H2D--> mpn_gzip_inflate_device --> text in HBM --mpn_fasta_scan--> bases in the part's buffer
                                                                                                       + names and lengths on the host
    a part closes (aligner.iter_target_parts_by_length, minimap2's -I rule) --> mapper.Index.from_device

What stays on the host path (fastx.open_once / iter_fastx, which defines the records): a target set with a FIFO or a saved index in
it (aligner.target_ingest_on_device: a FIFO can be read once and its member boundaries are unknown before decoding), a file whose
inflate or scan status is not OK (read again through the host path, which yields the same records or raises its own error), and the
inflate of a stream larger than MPN_INGEST_MAX_STREAM compressed bytes (zlib on the host; its text still goes through the scan).

BAM files as READ input take the same inflate kernel, a BGZF block being a gzip member of its own (iter_bam_read_batches, at the end
of this module):

    file --framing (18-byte block headers, no byte decoded)--> pinned group buffer --H2D--> mpn_gzip_inflate_device, a wave per block
      --mpn_bam_flatten--> one text --mpn_bam_walk--> record table --(skip 0x900, cut batches like aligner.iter_read_batches)-->
      mpn_bam_decode --> mapper.PackedReads with its device copy

There is no host path for them: a block whose status is not OK, or a text that is no BAM, raises ValueError.  The steps up to the
record table are BamTexts, which the stages that read a sorted BAM (candidates, clair_tensor, clair_call, local_realign) iterate too.

FASTQ files as READ input (MPN_READ_INGEST=device, iter_fastq_read_batches): the text comes from the file as it is, from zlib on the
host for an ordinary gzip stream, or through the front half of the BAM path (_BgzfTexts) for BGZF:

    text in HBM, behind the carry of the text before --mpn_fastq_scan--> a row per plain four-line record
      --(cut batches like aligner.iter_read_batches: ReadBatcher)--> mpn_fastq_gather --> mapper.PackedReads with its device copy

At the first record that is not plain the rest of the file -- the tail of the text and what the stream still holds -- goes through
fastx.iter_fastx, and its records keep filling the same batches.

The read filter and subseq (fastq_filter.filter_stream, fastx.subseq under the same knob) take their texts from the same sources
(_ChunkTexts, _BgzfTexts), scan them with fastq_scan and hand kept rows to a ReadBatcher.
"""
import collections
import ctypes as ct
import gzip
import io
import os
import stat

import numpy as np

from . import _ffi, fastx

OK, OVERFLOW, UNSUPPORTED = 0, 8, 9
STATUS_NAMES = ('OK', 'TRUNCATED', 'BAD_MAGIC', 'BAD_BLOCK', 'BAD_CODE', 'BAD_DISTANCE', 'BAD_CRC', 'BAD_SIZE', 'OVERFLOW', 'UNSUPPORTED',
                'BAM_TRUNCATED', 'BAM_BAD_MAGIC', 'BAM_BAD_HEADER', 'BAM_BAD_RECORD')
BAM_TRUNCATED, BAM_BAD_MAGIC, BAM_BAD_HEADER, BAM_BAD_RECORD = 10, 11, 12, 13
FASTQ_UNSUPPORTED = 14      # mpn_fastq_scan only; never reported to a user: the host reads what the scan does not take

# One launch must not run long on a shared device.  A wave inflates a single stream at 1.85 MB/s of compressed input (6.0 MB/s of
# text; profiles/r15_ingest/README.md), so the longest stream one launch may hold takes about a second; larger ones are inflated by
# zlib on the host.
MAX_STREAM_DEFAULT = 2 << 20
# Inflated text per group of files.  A group holds its compressed bytes (~0.3x), its text and, at worst, a retry's copy of it in HBM
# next to the part's bases and the resident index: 1 GiB of text keeps that below 3 GiB of the device's 288 GB, and is
# ~250 assemblies of 4 Mbp, enough streams to fill the 256 CUs.
BATCH_BYTES_DEFAULT = 1 << 30

_bound = False


def ingest_mode():
    """MPN_TARGET_INGEST: unset or `host` = fastx on the host, `device` = this module."""
    how = os.environ.get('MPN_TARGET_INGEST', 'host')
    if how not in ('host', 'device'):
        raise ValueError(f'MPN_TARGET_INGEST={how}: expected host or device')
    return how


def read_ingest_mode():
    """MPN_READ_INGEST: unset or `host` = FASTQ reads parsed by fastx on the host, `device` = iter_fastq_read_batches."""
    how = os.environ.get('MPN_READ_INGEST', 'host')
    if how not in ('host', 'device'):
        raise ValueError(f'MPN_READ_INGEST={how}: expected host or device')
    return how


def max_stream():
    return int(os.environ.get('MPN_INGEST_MAX_STREAM', MAX_STREAM_DEFAULT))


def batch_bytes():
    return int(os.environ.get('MPN_INGEST_BATCH_BYTES', BATCH_BYTES_DEFAULT))


def _lib():
    global _bound
    import torch
    torch.cuda.init()          # before libmpn.so is loaded (_ffi.hint)
    lib = _ffi.lib()
    if not _bound:
        P, I64 = ct.c_void_p, ct.c_int64
        lib.mpn_gzip_inflate.argtypes = [I64] + [P] * 8
        lib.mpn_gzip_inflate.restype = ct.c_int32
        lib.mpn_gzip_inflate_device.argtypes = [I64] + [P] * 8
        lib.mpn_gzip_inflate_device.restype = ct.c_int32
        lib.mpn_fasta_scan.argtypes = [I64, P, P, P, P, I64, P, P, P, I64, P, P, P, P, P, I64]
        lib.mpn_fasta_scan.restype = ct.c_int32
        lib.mpn_ingest_last_device_ms.argtypes = [ct.POINTER(ct.c_double), ct.POINTER(ct.c_double)]
        lib.mpn_ingest_last_device_ms.restype = None
        lib.mpn_bam_flatten.argtypes = [I64, P, P, P, P, I64, P, I64, P]
        lib.mpn_bam_flatten.restype = ct.c_int32
        lib.mpn_bam_walk.argtypes = [P, I64, I64, ct.c_int32, ct.c_int32, I64, P, P, P, P]
        lib.mpn_bam_walk.restype = ct.c_int32
        lib.mpn_bam_decode.argtypes = [P, I64, I64, P, P, P, P, P, I64]
        lib.mpn_bam_decode.restype = ct.c_int32
        lib.mpn_bam_last_device_ms.argtypes = [ct.POINTER(ct.c_double)] * 3
        lib.mpn_bam_last_device_ms.restype = None
        lib.mpn_fastq_tile.argtypes = []
        lib.mpn_fastq_tile.restype = ct.c_int32
        lib.mpn_fastq_scan.argtypes = [P, I64, ct.c_int32, I64, P, P, P, P]
        lib.mpn_fastq_scan.restype = ct.c_int32
        lib.mpn_fastq_gather.argtypes = [P, I64, I64, P, P, P, P, P, I64]
        lib.mpn_fastq_gather.restype = ct.c_int32
        lib.mpn_fastq_last_device_ms.argtypes = [ct.POINTER(ct.c_double)] * 2
        lib.mpn_fastq_last_device_ms.restype = None
        _bound = True
    return lib


def last_device_ms():
    """-> (inflate ms, scan ms) of the calling thread's last native calls"""
    return _ffi.device_ms(_lib().mpn_ingest_last_device_ms, 2)


def _align16(x):
    return (int(x) + 15) & ~15


def inflate_host(n_streams, data, in_off, slot_off, slot_cap, out):
    """mpn_gzip_inflate on host arrays (uint8 data / out, int64 offsets): what the tests call.  -> (length, members, status) arrays;
    out is written in place."""
    lib = _lib()
    data, out = np.ascontiguousarray(data, dtype=np.uint8), np.require(out, dtype=np.uint8, requirements=['C', 'W'])
    in_off, slot_off, slot_cap = (np.ascontiguousarray(a, dtype=np.int64) for a in (in_off, slot_off, slot_cap))
    length, members, status = np.zeros(n_streams, np.int64), np.zeros(n_streams, np.int32), np.zeros(n_streams, np.int32)
    _ffi.check(lib.mpn_gzip_inflate(n_streams, _ffi.ptr(data), in_off.ctypes.data, _ffi.ptr(out), _ffi.ptr(slot_off), _ffi.ptr(slot_cap), _ffi.ptr(length),
                                    _ffi.ptr(members), _ffi.ptr(status)), 'mpn_gzip_inflate')
    return length, members, status


class Inflated:
    """The text of n streams in HBM: stream i is text[off[i] : off[i] + length[i]] where status[i] is OK."""

    def __init__(self, text, off, length, members, status, on_host, retried):
        self.text, self.off, self.length, self.members, self.status = text, off, length, members, status
        self.on_host, self.retried = on_host, retried      # streams zlib inflated (over the size limit); streams that took the retry
        self.n = len(off)

    def bytes(self, i):
        a = int(self.off[i])
        return self.text[a:a + int(self.length[i])].cpu().numpy().tobytes()


def _read_blob(item):
    if isinstance(item, (bytes, bytearray, memoryview)):
        return bytes(item)
    with open(item, 'rb') as f:
        return f.read()


def _size_of(item):
    return len(item) if isinstance(item, (bytes, bytearray, memoryview)) else os.path.getsize(item)


def _read_into(item, view):
    """the whole of a file (or bytes object) into a uint8 numpy view of its size: no copy on the way for a file"""
    if isinstance(item, (bytes, bytearray, memoryview)):
        view[:] = np.frombuffer(item, dtype=np.uint8)
        return
    with open(item, 'rb', buffering=0) as f:
        got = 0
        while got < len(view):
            k = f.readinto(memoryview(view)[got:])
            if not k:
                raise OSError(f'{item}: shorter than its size says')
            got += k


def _slot_guess(tail4, size):
    """ISIZE of the last member: exact for a single-member file.  Never more than deflate can expand (1032:1): a damaged ISIZE
    must not size an allocation."""
    if size < 18:
        return 0
    return min(int.from_bytes(bytes(tail4), 'little'), 1032 * size + 64)


def inflate_files(items, device='cuda', limit=None, timings=None, tail_bytes=0):
    """items: paths or bytes objects, each a whole gzip file -> Inflated.  The files are read straight into one pinned buffer and
    uploaded.  A stream that overflows the slot its last ISIZE sized is run ONCE more with the length the decoder reported -- all
    such streams of the call in one launch; a stream of more than `limit` (MPN_INGEST_MAX_STREAM) compressed bytes is inflated
    by zlib here and uploaded (zlib's exception propagates).  Any status other than OK is left for the caller.  tail_bytes: room
    the caller wants behind the slots in Inflated.text (the plain files of a group go there), from Inflated.tail on."""
    import time
    import torch
    lib = _lib()
    limit = max_stream() if limit is None else int(limit)
    t0 = time.perf_counter()
    n = len(items)
    full = [_size_of(x) for x in items]
    on_host = [i for i in range(n) if full[i] > limit]
    host_text = {i: gzip.GzipFile(fileobj=io.BytesIO(_read_blob(items[i])), mode='rb').read() for i in on_host}
    in_off = np.zeros(n + 1, dtype=np.int64)
    in_off[1:] = np.cumsum([0 if i in host_text else full[i] for i in range(n)])
    staging = torch.empty(max(int(in_off[-1]), 1), dtype=torch.uint8).pin_memory()
    view = staging.numpy()
    cap = np.zeros(n, dtype=np.int64)
    for i, x in enumerate(items):
        if i in host_text:
            cap[i] = len(host_text[i])
        else:
            _read_into(x, view[in_off[i]:in_off[i + 1]])
            cap[i] = _slot_guess(view[max(in_off[i + 1] - 4, in_off[i]):in_off[i + 1]], full[i])
    t1 = time.perf_counter()
    d_in = staging.to(device)
    torch.cuda.synchronize()
    t2 = time.perf_counter()

    def run(d_src, offs, caps, room=0):
        """the streams d_src[offs[j] : offs[j + 1]] into a fresh buffer of slots of `caps` (+ room bytes behind them)
        -> (buffer, slot offsets with their end, length, members, status, device ms)"""
        m = len(caps)
        caps, offs = np.ascontiguousarray(caps, dtype=np.int64), np.ascontiguousarray(offs, dtype=np.int64)
        so = np.zeros(m + 1, dtype=np.int64)
        so[1:] = np.cumsum([_align16(c) for c in caps])
        buf = torch.empty(max(int(so[-1]) + room, 16), dtype=torch.uint8, device=device)
        length, members, status = np.zeros(m, np.int64), np.zeros(m, np.int32), np.zeros(m, np.int32)
        if m:
            _ffi.check(lib.mpn_gzip_inflate_device(m, d_src.data_ptr(), offs.ctypes.data, buf.data_ptr(), so.ctypes.data, caps.ctypes.data,
                                                   length.ctypes.data, members.ctypes.data, status.ctypes.data), 'mpn_gzip_inflate_device')
        return buf, so, length, members, status, last_device_ms()[0] if m else 0.0

    text, so, length, members, status, ms = run(d_in, in_off, cap, room=int(tail_bytes))
    off, tail = so[:n].copy(), int(so[-1])
    for i, t in host_text.items():      # (their compressed size here is 0: the kernel saw an empty stream)
        if t:
            text[int(off[i]):int(off[i]) + len(t)] = torch.frombuffer(bytearray(t), dtype=torch.uint8).to(device)
        length[i], members[i], status[i] = len(t), 0, OK
    again = np.flatnonzero(status == OVERFLOW)
    if len(again):
        # one launch for all of them: their compressed bytes are gathered, device to device, one behind the other
        d_again = torch.cat([d_in[int(in_off[i]):int(in_off[i + 1])] for i in again])
        offs2 = np.zeros(len(again) + 1, dtype=np.int64)
        offs2[1:] = np.cumsum(in_off[again + 1] - in_off[again])
        text2, so2, length2, members2, status2, ms2 = run(d_again, offs2, length[again].copy())
        # the scan wants one text buffer: the retried streams' text is appended (a copy of the group's text; a retry is for
        # multi-member files only)
        base = _align16(text.numel())
        text = torch.cat([text, torch.empty(base - text.numel(), dtype=torch.uint8, device=device), text2])
        off[again], length[again], members[again], status[again] = so2[:-1] + base, length2, members2, status2
        ms += ms2
    torch.cuda.synchronize()
    if timings is not None:
        timings['read'] = timings.get('read', 0) + (t1 - t0)
        timings['h2d'] = timings.get('h2d', 0) + (t2 - t1)
        timings['inflate'] = timings.get('inflate', 0) + (time.perf_counter() - t2)
        timings['inflate_device_ms'] = timings.get('inflate_device_ms', 0) + ms
    res = Inflated(text, off, length, members, status, on_host, [int(i) for i in again])
    res.tail, res.launches = tail, 1 + (1 if len(again) else 0)
    return res


class FastaScan:
    """Records of the scanned streams: names / lens / stream per record, n_records / n_bases / status per stream, and `seq`, the
    device tensor that holds the bases of the records one after another from `seq_pos` on (None for a counting call)."""

    def __init__(self, names, lens, stream, n_records, n_bases, status, seq, seq_pos):
        self.names, self.lens, self.stream = names, lens, stream
        self.n_records, self.n_bases, self.status, self.seq, self.seq_pos = n_records, n_bases, status, seq, seq_pos


def scan_fasta(text, off, length, out=None, out_pos=0, count_only=False):
    """text: torch uint8 tensor in HBM; stream i is text[off[i] : off[i] + length[i]].  The bases go to out[out_pos:] (a torch uint8
    tensor in HBM with room for them; a fresh one without `out`).  count_only: records, bases and status per stream only."""
    import torch
    lib = _lib()
    off, length = np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(length, dtype=np.int64)
    n = len(off)
    if n and (off.min() < 0 or length.min() < 0 or int((off + length).max()) > text.numel()):
        raise ValueError('scan_fasta: a stream lies outside the text')
    n_rec, n_bases, status = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int32)

    def call(d_seq, seq_cap, rec_cap, rs, rno, rnl, rsl, pool, pool_cap, may_be_short=False):
        rc = lib.mpn_fasta_scan(n, text.data_ptr(), _ffi.ptr(off), _ffi.ptr(length), d_seq, seq_cap, _ffi.ptr(n_rec), _ffi.ptr(n_bases), _ffi.ptr(status), rec_cap,
                                rs, rno, rnl, rsl, pool, pool_cap)
        if not (rc == -3 and may_be_short):
            _ffi.check(rc, 'mpn_fasta_scan')
        return rc
    call(None, 0, 0, None, None, None, None, None, 0)
    ms = last_device_ms()[1]
    if count_only:
        return FastaScan([], np.zeros(0, np.int64), np.zeros(0, np.int32), n_rec, n_bases, status, None, 0)
    R, B = int(n_rec.sum()), int(n_bases.sum())
    if out is None:
        out, out_pos = torch.empty(max(B, 1), dtype=torch.uint8, device=text.device), 0
    if out.numel() - out_pos < B:
        raise ValueError(f'scan_fasta: {B} bases do not fit behind {out_pos} of {out.numel()}')
    rs, rno, rnl, rsl = np.zeros(R, np.int32), np.zeros(R, np.int64), np.zeros(R, np.int32), np.zeros(R, np.int64)
    pool = np.zeros(64 * R + 4096, dtype=np.uint8)
    if R:
        args = (out.data_ptr() + out_pos, B, R, _ffi.ptr(rs), _ffi.ptr(rno), _ffi.ptr(rnl), _ffi.ptr(rsl))
        if call(*args, pool.ctypes.data, pool.size, may_be_short=True) == -3:
            # the names are longer than guessed (the lengths are complete): once more with room for them
            ms += last_device_ms()[1]
            pool = np.zeros(int(rnl.astype(np.int64).sum()), dtype=np.uint8)
            call(*args, pool.ctypes.data, pool.size)
        ms += last_device_ms()[1]
    ends = np.cumsum(rnl.astype(np.int64))
    raw = pool.tobytes()
    names = [raw[e - l:e].decode() for e, l in zip(ends.tolist(), rnl.tolist())]
    res = FastaScan(names, rsl, rs, n_rec, n_bases, status, out, out_pos)
    res.device_ms = ms
    return res


def is_device_candidate(path):
    """A regular file that is not a saved index: what the device path takes."""
    try:
        if not stat.S_ISREG(os.stat(path).st_mode):
            return False
        with open(path, 'rb') as f:
            return f.read(8) != fastx.INDEX_MAGIC
    except OSError:
        return False


def _host_records(path):
    kind, stream = fastx.open_once(path)
    try:
        if kind == 'index':
            raise ValueError(f'{path}: a saved index cannot be mixed with sequence targets')
        if kind == 'bam':
            raise ValueError(f'{path}: a BAM file is taken as read input only, not as a target')
        return [(name, seq) for name, seq, _ in fastx.iter_fastx(stream)]
    finally:
        stream.close()


class _PartBuffer:
    """The bases of the records that have not been built into an index yet, in one device buffer: [start, used)."""

    def __init__(self, device):
        import torch
        self.torch, self.device = torch, device
        self.buf = torch.empty(1 << 20, dtype=torch.uint8, device=device)
        self.start = self.used = 0

    def reserve(self, more):
        """room for `more` bytes behind `used`; what is before `start` is dropped when the buffer has to move anyway"""
        if self.used + more <= self.buf.numel():
            return
        live = self.used - self.start
        new = self.torch.empty(max(2 * (live + more), 1 << 20), dtype=self.torch.uint8, device=self.device)
        new[:live] = self.buf[self.start:self.used]
        self.buf, self.start, self.used = new, 0, live

    def append_host(self, data):
        self.reserve(len(data))
        if data:
            self.buf[self.used:self.used + len(data)] = self.torch.frombuffer(bytearray(data), dtype=self.torch.uint8).to(self.device)
            self.used += len(data)


def _file_groups(paths, limit_bytes):
    """Consecutive files whose inflated text (the ISIZE guess; the size of a plain file) stays below limit_bytes; one file at least."""
    group, total = [], 0
    for p in paths:
        size = os.path.getsize(p)
        with open(p, 'rb') as f:
            gz = f.read(2) == b'\x1f\x8b'
            if gz and size >= 18:
                f.seek(-4, os.SEEK_END)
                size = max(size, min(int.from_bytes(f.read(4), 'little'), 1032 * size))
        if group and total + size > limit_bytes:
            yield group
            group, total = [], 0
        group.append((p, gz))
        total += size
    if group:
        yield group


def iter_device_records(paths, part, device='cuda', timings=None):
    """Yields (name, length) of every record of `paths` in order; before a record is yielded its bases are in `part` (_PartBuffer),
    behind those of the records before it.  Every path is a device candidate (the callers ask aligner.target_ingest_on_device)."""
    import time
    import torch
    for p in paths:
        if not is_device_candidate(p):
            raise ValueError(f'{p}: the device path takes regular sequence files only')
    for group in _file_groups(paths, batch_bytes()):
        t0 = time.perf_counter()
        plain = [(p, os.path.getsize(p)) for p, gz in group if not gz]
        plain_off = np.zeros(len(plain) + 1, dtype=np.int64)
        plain_off[1:] = np.cumsum([_align16(size) for _, size in plain])
        # one text buffer for the scan: the inflated slots, and behind them the plain files, read into a pinned buffer and uploaded
        inf = inflate_files([p for p, gz in group if gz], device=device, timings=timings, tail_bytes=int(plain_off[-1]))
        text = inf.text
        if plain:
            t0 = time.perf_counter()
            staging = torch.empty(int(plain_off[-1]), dtype=torch.uint8).pin_memory()
            for k, (p, size) in enumerate(plain):
                _read_into(p, staging.numpy()[plain_off[k]:plain_off[k] + size])
            text[inf.tail:inf.tail + int(plain_off[-1])] = staging.to(device)
            if timings is not None:
                timings['read'] = timings.get('read', 0) + (time.perf_counter() - t0)
        off, length, ok = np.zeros(len(group), np.int64), np.zeros(len(group), np.int64), np.ones(len(group), bool)
        gi = pi = 0
        for k, (p, gz) in enumerate(group):
            if gz:
                off[k], length[k], ok[k] = inf.off[gi], inf.length[gi], inf.status[gi] == OK
                gi += 1
            else:
                off[k], length[k] = inf.tail + plain_off[pi], plain[pi][1]
                pi += 1
        length[~ok] = 0
        t0 = time.perf_counter()
        counted = scan_fasta(text, off, length, count_only=True)
        scan_s = time.perf_counter() - t0
        ok &= counted.status == OK
        # the files the device cannot take split the group into runs; every run is scanned straight into the part's buffer
        k = 0
        while k < len(group):
            if not ok[k]:
                for name, seq in _host_records(group[k][0]):
                    part.append_host(seq)
                    yield name, len(seq)
                k += 1
                continue
            e = k
            while e < len(group) and ok[e]:
                e += 1
            t0 = time.perf_counter()
            part.reserve(int(counted.n_bases[k:e].sum()))
            got = scan_fasta(text, off[k:e], length[k:e], out=part.buf, out_pos=part.used)
            part.used += int(got.n_bases.sum())
            if timings is not None:
                timings['scan'] = timings.get('scan', 0) + scan_s + (time.perf_counter() - t0)
                timings['scan_device_ms'] = timings.get('scan_device_ms', 0) + got.device_ms
                scan_s = 0
            yield from zip(got.names, got.lens.tolist())
            k = e
        del text, inf


def iter_target_parts_device(paths, batch_bases, k=15, w=10, device='cuda', timings=None):
    """The index parts of a target set, cut like aligner.iter_target_parts cuts them, each built by mapper.Index.from_device from
    bases that were inflated and scanned on the GPU.  The caller closes every part before asking for the next one."""
    import time
    from . import aligner, mapper
    part = _PartBuffer(device)
    for recs in aligner.iter_target_parts_by_length(iter_device_records(paths, part, device, timings), batch_bases):
        names, lens = [r[0] for r in recs], np.array([r[1] for r in recs], dtype=np.int64)
        if len(lens) and int(lens.max()) > 0x7fffffff:
            raise ValueError('a target sequence of more than 2^31 - 1 bases')
        total = int(lens.sum())
        t0 = time.perf_counter()
        idx = mapper.Index.from_device(names, part.buf.data_ptr() + part.start, lens.astype(np.int32), k=k, w=w)
        if timings is not None:
            timings['index'] = timings.get('index', 0) + (time.perf_counter() - t0)
        part.start += total
        yield idx


# ---- BAM as read input --------------------------------------------------------------------------------------------------------------
BAM_ROW = np.dtype([('off', '<i8'), ('l_seq', '<i4'), ('flag', '<u2'), ('l_read_name', 'u1'), ('has_qual', 'u1')])    # mpn_bam_row
BAM_SKIP = 0x900            # secondary and supplementary records: `samtools fastq` leaves them out
BGZF_MAX_TEXT = 1 << 16     # ISIZE of a BGZF block
# Records per launch of the walk.  Its one wave pays a dependent read per record, 0.4 us if each is an HBM miss (the records of
# long reads are several KiB apart); 65 536 records keep a launch below 30 ms.  Measured: profiles/r16_bam_ingest/README.md.
BAM_WALK_RECORDS_DEFAULT = 1 << 16


def bam_walk_records():
    return int(os.environ.get('MPN_BAM_WALK_RECORDS', BAM_WALK_RECORDS_DEFAULT))


def last_bam_device_ms():
    """-> (flatten ms, walk ms, decode ms) of the calling thread's last native calls"""
    return _ffi.device_ms(_lib().mpn_bam_last_device_ms, 3)


def _tick(timings, key, value):
    if timings is not None:
        timings[key] = timings.get(key, 0) + value


def bgzf_block_size(head, offset=0):
    """head: the first 12 + XLEN bytes of a BGZF block (or more) -> its whole size, BSIZE + 1.  ValueError for anything else."""
    if len(head) < 12 or head[:4] != b'\x1f\x8b\x08\x04':
        raise ValueError(f'not a BGZF block at file offset {offset}: header {bytes(head[:4]).hex()}')
    xlen = int.from_bytes(head[10:12], 'little')
    p = 12
    while p + 4 <= 12 + xlen and p + 4 <= len(head):
        slen = int.from_bytes(head[p + 2:p + 4], 'little')
        if head[p:p + 2] == b'BC' and slen == 2 and p + 6 <= len(head):
            size = int.from_bytes(head[p + 4:p + 6], 'little') + 1
            if size < 12 + xlen + 2 + 8:
                raise ValueError(f'BGZF block at file offset {offset}: BSIZE {size - 1} is smaller than the block\'s own header and trailer')
            return size
        p += 4 + slen
    raise ValueError(f'not a BGZF block at file offset {offset}: no BC subfield')


class _BgzfGroups:
    """Framing: the BGZF blocks of one stream, group by group, in a pinned buffer.  No byte is decoded."""

    def __init__(self, stream, group_text):
        import torch
        self.torch = torch
        self.stream = stream if hasattr(stream, 'peek') else io.BufferedReader(stream)
        self.group_text = max(1, int(group_text))
        # compressed bytes a group may hold: half its text (BGZF of bases and qualities is ~0.4x) and room for one block
        self.cap = self.group_text // 2 + (1 << 17)
        self.staging = torch.empty(min(self.cap, 4 << 20), dtype=torch.uint8).pin_memory()
        self.pos = 0            # file offset of the next block
        self.blocks = 0         # blocks before the next group
        self.eof = False

    def _room(self, used, more):
        if used + more <= self.staging.numel():
            return
        new = self.torch.empty(min(max(2 * self.staging.numel(), used + more), max(self.cap, used + more)), dtype=self.torch.uint8).pin_memory()
        new[:used] = self.staging[:used]
        self.staging = new

    def _fill(self, view):
        got = 0
        while got < len(view):
            k = self.stream.readinto(memoryview(view)[got:])
            if not k:
                return got
            got += k
        return got

    def next_group(self):
        """-> (uint8 pinned tensor of the blocks' bytes, in_off [n + 1], isize [n], file offset of every block); n = 0 at the end"""
        used, text, in_off, isize, where = 0, 0, [0], [], []
        while not self.eof:
            head = self.stream.read(12)
            if not head:
                self.eof = True
                break
            if head[:4] != b'\x1f\x8b\x08\x04'[:len(head)]:
                raise ValueError(f'not a BGZF block at file offset {self.pos}: header {head[:4].hex()}')
            xlen = int.from_bytes(head[10:12], 'little') if len(head) == 12 else 0
            extra = self.stream.read(xlen)
            if len(head) < 12 or len(extra) < xlen:
                raise ValueError(f'the file ends inside the BGZF block at file offset {self.pos}')
            head += extra
            size = bgzf_block_size(head, self.pos)
            self._room(used, size)
            view = self.staging.numpy()
            view[used:used + len(head)] = np.frombuffer(head, dtype=np.uint8)
            if self._fill(view[used + len(head):used + size]) < size - len(head):
                raise ValueError(f'the file ends inside the BGZF block at file offset {self.pos}')
            n_text = int.from_bytes(view[used + size - 4:used + size].tobytes(), 'little')
            if n_text > BGZF_MAX_TEXT:
                raise ValueError(f'BGZF block at file offset {self.pos}: ISIZE {n_text} is more than a block holds')
            where.append(self.pos)
            isize.append(n_text)
            used += size
            in_off.append(used)
            self.pos += size
            text += n_text
            if text >= self.group_text or used + (1 << 16) > self.cap:
                self.eof = not self.stream.peek(1)
                break
        first = self.blocks
        self.blocks += len(isize)
        return self.staging[:used], np.array(in_off, dtype=np.int64), np.array(isize, dtype=np.int64), where, first


def bam_flatten(slots, slot_off, slot_len, carry, device):
    """mpn_bam_flatten: -> (text tensor, padded to 16, and its length).  carry: a uint8 device tensor (any view) or None."""
    import torch
    lib = _lib()
    slot_off, slot_len = np.ascontiguousarray(slot_off, dtype=np.int64), np.ascontiguousarray(slot_len, dtype=np.int64)
    n_carry = 0 if carry is None else carry.numel()
    total = n_carry + int(slot_len.sum())
    text = torch.empty(max(_align16(total), 16), dtype=torch.uint8, device=device)
    got = ct.c_int64(0)
    _ffi.check(lib.mpn_bam_flatten(len(slot_off), slots.data_ptr(), _ffi.ptr(slot_off), _ffi.ptr(slot_len), carry.data_ptr() if n_carry else None, n_carry,
                                   text.data_ptr(), text.numel(), ct.byref(got)), 'mpn_bam_flatten')
    assert got.value == total
    return text, total


def bam_walk(text, text_len, start, at_header, final, max_records):
    """mpn_bam_walk -> (rows as a BAM_ROW array, next, status)"""
    lib = _lib()
    rows = np.zeros(max_records, dtype=BAM_ROW)
    n, nxt, status = ct.c_int64(0), ct.c_int64(0), ct.c_int32(0)
    _ffi.check(lib.mpn_bam_walk(text.data_ptr(), int(text_len), int(start), int(bool(at_header)), int(bool(final)), int(max_records), _ffi.ptr(rows),
                                ct.byref(n), ct.byref(nxt), ct.byref(status)), 'mpn_bam_walk')
    return rows[:n.value], nxt.value, status.value


def bam_decode(text, text_len, rows, with_qual):
    """mpn_bam_decode on the (kept) rows -> (bases tensor, qualities tensor or None, both of total + 16 bytes rounded up to 16, names)"""
    import torch
    lib = _lib()
    rows = np.ascontiguousarray(rows, dtype=BAM_ROW)
    lens = rows['l_seq'].astype(np.int64)
    off = np.zeros(len(rows), dtype=np.int64)
    off[1:] = np.cumsum(lens[:-1])
    size = _align16(int(lens.sum()) + 16)
    seq = torch.empty(size, dtype=torch.uint8, device=text.device)
    qual = torch.empty(size, dtype=torch.uint8, device=text.device) if with_qual else None
    name_len = rows['l_read_name'].astype(np.int64) - 1
    pool = np.zeros(max(int(name_len.sum()), 1), dtype=np.uint8)
    _ffi.check(lib.mpn_bam_decode(text.data_ptr(), int(text_len), len(rows), _ffi.ptr(rows), _ffi.ptr(off), seq.data_ptr(), qual.data_ptr() if with_qual else None,
                                  pool.ctypes.data, pool.size), 'mpn_bam_decode')
    raw, ends = pool.tobytes(), np.cumsum(name_len)
    names = [raw[e - l:e].decode() for e, l in zip(ends.tolist(), name_len.tolist())]
    return seq, qual, names


def _join_batch(parts, names, lens, with_qual, device, timings, t0, stage):
    """parts: [(bases tensor, qualities tensor or None, bytes of it that count)] in read order, the pieces of one batch as
    mpn_bam_decode / mpn_fastq_gather lay them out -> mapper.PackedReads with its device copy.  t0: when the batch was begun (the
    time up to the download is booked on `stage`)."""
    import time
    import torch
    from . import mapper
    total = int(lens.astype(np.int64).sum())
    if len(parts) == 1:
        seq, qual = parts[0][0][:total + 16], (parts[0][1][:total + 16] if with_qual else None)
    else:     # a batch whose records lie in several texts: its pieces are joined, device to device
        pad = torch.zeros(16, dtype=torch.uint8, device=device)
        seq = torch.cat([s[:k] for s, _, k in parts] + [pad])
        qual = torch.cat([q[:k] for _, q, k in parts] + [pad]) if with_qual else None
    off = np.zeros(len(lens), dtype=np.int64)
    off[1:] = np.cumsum(lens[:-1].astype(np.int64))
    t1 = time.perf_counter()
    buf = seq.cpu().numpy()       # the host copy SAM output and the writers need: one download
    qbuf = qual.cpu().numpy() if with_qual else None
    dev = (seq, torch.from_numpy(off).to(device), torch.from_numpy(lens).to(device))
    torch.cuda.synchronize()
    _tick(timings, stage, t1 - t0)
    _tick(timings, 'd2h', time.perf_counter() - t1)
    return mapper.PackedReads.from_arrays(names, buf, off, lens, dev=dev, qbuf=qbuf)


def _bam_batch(pieces, device, timings):
    """pieces: [(text, text_len, kept rows)] in file order, the reads of one batch -> mapper.PackedReads with its device copy"""
    import time
    t0 = time.perf_counter()
    with_qual = any(bool(rows['has_qual'].any()) for _, _, rows in pieces)
    parts, names = [], []
    for text, text_len, rows in pieces:
        seq, qual, nm = bam_decode(text, text_len, rows, with_qual)
        _tick(timings, 'decode_device_ms', last_bam_device_ms()[2])
        parts.append((seq, qual, int(rows['l_seq'].astype(np.int64).sum())))
        names += nm
    lens = np.concatenate([rows['l_seq'] for _, _, rows in pieces]).astype(np.int32)
    return _join_batch(parts, names, lens, with_qual, device, timings, t0, 'decode')


class _BgzfTexts:
    """The text of a BGZF stream in HBM, group by group: framing (_BgzfGroups), upload, mpn_gzip_inflate_device with a wave per block,
    mpn_bam_flatten behind the carry.  What BAM and BGZF-compressed FASTQ share."""

    def __init__(self, stream, device, timings=None):
        self.groups, self.device, self.timings = _BgzfGroups(stream, batch_bytes()), device, timings

    def next_text(self, carry):
        """carry: the unconsumed tail of the text before (a uint8 device tensor, any view) or None
        -> (text tensor, padded to 16; its length; whether it is the last of the stream)"""
        import time
        import torch
        lib, device, timings = _lib(), self.device, self.timings
        t0 = time.perf_counter()
        staged, in_off, isize, where, first = self.groups.next_group()
        final = self.groups.eof
        t1 = time.perf_counter()
        n = len(isize)
        d_in = staged.to(device, non_blocking=True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        so = np.zeros(n + 1, dtype=np.int64)
        so[1:] = np.cumsum((isize + 15) & ~15)
        slots = torch.empty(max(int(so[-1]), 16), dtype=torch.uint8, device=device)
        length, members, status = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32)
        if n:
            _ffi.check(lib.mpn_gzip_inflate_device(n, d_in.data_ptr(), in_off.ctypes.data, slots.data_ptr(), so.ctypes.data, isize.ctypes.data,
                                                   length.ctypes.data, members.ctypes.data, status.ctypes.data), 'mpn_gzip_inflate_device')
            _tick(timings, 'inflate_device_ms', last_device_ms()[0])
            bad = np.flatnonzero((status != OK) | (length != isize) | (members != 1))
            if len(bad):
                b = int(bad[0])
                what = STATUS_NAMES[status[b]] if status[b] != OK else f'{members[b]} gzip members of {length[b]} bytes, ISIZE {isize[b]}'
                raise ValueError(f'BGZF block {first + b} at file offset {where[b]}: {what}')
        t3 = time.perf_counter()
        text, text_len = bam_flatten(slots, so[:n], isize, carry, device)
        _tick(timings, 'flatten_device_ms', last_bam_device_ms()[0])
        t4 = time.perf_counter()
        for key, dt in (('read', t1 - t0), ('h2d', t2 - t1), ('inflate', t3 - t2), ('flatten', t4 - t3)):
            _tick(timings, key, dt)
        return text, text_len, final


# text[:text_len]: a device tensor; rows: every record walked in it (a BAM_ROW array); final: the last text of the file; base: the
# offset of text[0] in the whole inflated stream
BamText = collections.namedtuple('BamText', 'text text_len rows final base')


class BamTexts:
    """The texts of one BAM file with their records walked, one BamText per step: what every reader of a BAM iterates over, and the
    only caller of bam_walk.  source: a path (opened at the first text, closed on leaving the `with`) or an open binary stream (read
    to its end, left open).  A text begins where the one before ended, at the first byte that no complete record holds -- or, after
    keep_from(i), at record i of the text before, for a reader that needs those records again next to the ones that follow.  The
    text before is released once the next is built: one text and its carry are resident.  Booked in `timings`: what _BgzfTexts
    books, and walk_device_ms, walk_launches and walk (seconds).  ValueError for a text that is no BAM, with its offset in the
    whole inflated stream."""

    def __init__(self, source, device='cuda', timings=None, walk_records=None):
        self.path = source if isinstance(source, (str, bytes, os.PathLike)) else None
        self.stream = None if self.path is not None else source
        self.device, self.timings = device or 'cuda', timings
        self.walk_records = max(1, bam_walk_records() if walk_records is None else int(walk_records))
        self._steps, self._n_rows, self._keep = None, 0, None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self._steps = None
        if self.path is not None and self.stream is not None:
            self.stream.close()

    def __iter__(self):
        return self

    def __next__(self):
        if self._steps is None:
            self._steps = self._run()
        return next(self._steps)

    def keep_from(self, i):
        """the next text begins at record i of the current one (i = len(rows): behind its last complete record, as without a call)"""
        if not 0 <= i <= self._n_rows:
            raise ValueError(f'keep_from({i}): the text has {self._n_rows} records')
        self._keep = int(i)

    def _run(self):
        import time
        if self.path is not None:
            self.stream = io.BufferedReader(open(self.path, 'rb', buffering=0), buffer_size=1 << 20)
        texts, timings = _BgzfTexts(self.stream, self.device, self.timings), self.timings
        where = '' if self.path is None else f'{os.fsdecode(self.path)}: '
        carry, at_header, base = None, True, 0
        while True:
            text, text_len, final = texts.next_text(carry)
            del carry
            t0 = time.perf_counter()
            start, got = 0, []
            while True:
                rows, nxt, st = bam_walk(text, text_len, start, at_header, final, self.walk_records)
                _tick(timings, 'walk_device_ms', last_bam_device_ms()[1])
                _tick(timings, 'walk_launches', 1)
                if st != OK:
                    raise ValueError(f'{where}BAM text at offset {base + nxt} of the inflated stream: {STATUS_NAMES[st]}')
                if at_header and nxt > start:
                    at_header = False
                got.append(rows)
                start = nxt
                if len(rows) < self.walk_records:
                    break
            rows = np.concatenate(got)
            _tick(timings, 'walk', time.perf_counter() - t0)
            self._n_rows, self._keep = len(rows), None
            yield BamText(text, text_len, rows, final, base)
            if final:
                return
            if self._keep is not None and self._keep < len(rows):
                start = int(rows['off'][self._keep])
            carry = text[start:text_len]
            base += start


def iter_bam_read_batches(stream_or_path, batch_bases=200_000_000, device='cuda', walk_records=None, timings=None):
    """The reads of one BAM file as mapper.PackedReads of at most batch_bases each (cut as aligner.iter_read_batches cuts FASTQ
    records), resident on the device, with the semantics of `samtools fastq`.  stream_or_path: a path, or
    the binary stream fastx.open_once returned for kind 'bam' (read to its end, not closed)."""
    device = device or 'cuda'
    pieces, acc, count = [], 0, 0
    with BamTexts(stream_or_path, device, timings, walk_records) as texts:
        for t in texts:
            _tick(timings, 'records', len(t.rows))
            rows = t.rows[(t.rows['flag'] & BAM_SKIP) == 0]
            lo = 0
            for i, l in enumerate(rows['l_seq'].tolist()):
                if count and acc + l > batch_bases:
                    if i > lo:
                        pieces.append((t.text, t.text_len, rows[lo:i]))
                    yield _bam_batch(pieces, device, timings)
                    pieces, acc, count, lo = [], 0, 0, i
                acc += l
                count += 1
            if lo < len(rows):
                pieces.append((t.text, t.text_len, rows[lo:]))
        if count:
            yield _bam_batch(pieces, device, timings)


def read_bam(stream_or_path, device='cuda'):
    """-> list of (name, bases, qualities or None) like fastx.read_fastx(with_qual=True); qualities follow the rule of a PackedReads
    batch: None if no read of the file has any, '!' for a read without them otherwise."""
    out = []
    for b in iter_bam_read_batches(stream_or_path, device=device):
        for i in range(b.n):
            a, z = int(b.off[i]), int(b.off[i]) + int(b.lens[i])
            out.append((b.names[i], b.buf[a:z].tobytes(), None if b.qbuf is None else b.qbuf[a:z].tobytes()))
    return out


# ---- FASTQ as read input ------------------------------------------------------------------------------------------------------------
FASTQ_ROW = np.dtype([('seq_off', '<i8'), ('qual_off', '<i8'), ('name_off', '<i8'), ('len', '<i4'), ('name_len', '<i4')])    # mpn_fastq_row
# Host-to-device pieces of a plain or host-inflated text: one pinned buffer of this size is filled and uploaded in turns.
FASTQ_STAGING = 16 << 20


def fastq_tile():
    """MPN_FASTQ_TILE of the library that is loaded"""
    return int(_lib().mpn_fastq_tile())


def last_fastq_device_ms():
    """-> (scan ms, gather ms) of the calling thread's last native calls"""
    return _ffi.device_ms(_lib().mpn_fastq_last_device_ms, 2)


def fastq_scan(text, text_len, final, rec_cap=None):
    """mpn_fastq_scan on text[:text_len] (a uint8 device tensor) -> (rows as a FASTQ_ROW array, consumed, status, device ms).  rec_cap: the
    size of the table of the first attempt (a guess from the text's length by default); a table that is too small is made
    again with the count the call reported."""
    lib = _lib()
    text_len = int(text_len)
    if text_len > text.numel():
        raise ValueError('fastq_scan: the text is shorter than text_len')
    cap = text_len // 64 + 1024 if rec_cap is None else int(rec_cap)
    n, consumed, status = ct.c_int64(0), ct.c_int64(0), ct.c_int32(0)
    ms = 0.0
    while True:
        rows = np.empty(cap, dtype=FASTQ_ROW)
        rc = lib.mpn_fastq_scan(text.data_ptr(), text_len, int(bool(final)), cap, _ffi.ptr(rows), ct.byref(n), ct.byref(consumed), ct.byref(status))
        ms += last_fastq_device_ms()[0]
        if rc == -3 and n.value > cap:
            cap = n.value
            continue
        _ffi.check(rc, 'mpn_fastq_scan')
        return rows[:n.value], consumed.value, status.value, ms


def fastq_gather(text, text_len, rows, with_qual=True):
    """mpn_fastq_gather on the rows -> (bases tensor, qualities tensor or None, both of total + 16 bytes rounded up to 16, names)"""
    import torch
    lib = _lib()
    rows = np.ascontiguousarray(rows, dtype=FASTQ_ROW)
    lens = rows['len'].astype(np.int64)
    off = np.zeros(len(rows), dtype=np.int64)
    off[1:] = np.cumsum(lens[:-1])
    size = _align16(int(lens.sum()) + 16)
    seq = torch.empty(size, dtype=torch.uint8, device=text.device)
    qual = torch.empty(size, dtype=torch.uint8, device=text.device) if with_qual else None
    name_len = rows['name_len'].astype(np.int64)
    pool = np.zeros(max(int(name_len.sum()), 1), dtype=np.uint8)
    _ffi.check(lib.mpn_fastq_gather(text.data_ptr(), int(text_len), len(rows), _ffi.ptr(rows), _ffi.ptr(off), seq.data_ptr(), qual.data_ptr() if with_qual else None,
                                    pool.ctypes.data, pool.size), 'mpn_fastq_gather')
    raw, ends = pool.tobytes(), np.cumsum(name_len)
    names = [raw[e - l:e].decode() for e, l in zip(ends.tolist(), name_len.tolist())]
    return seq, qual, names


class ReadBatcher:
    """Cuts reads into batches by the rule of the host loop of aligner.iter_read_batches (a read that would take a batch that is
    not empty past batch_bases starts the next one).  The reads come as rows of scanned texts in HBM (add_rows) or as host records
    (add_host: the part of a file fastx.iter_fastx read); a batch may hold both, from several texts and files, and is joined device
    to device.  add_rows, add_host and flush are generators of the batches that became full."""

    def __init__(self, batch_bases, device='cuda', timings=None):
        self.batch_bases, self.device, self.timings = batch_bases, device or 'cuda', timings
        self.pieces, self.acc, self.count = [], 0, 0      # pieces: ('rows', text, text_len, rows, names or None) or ('host', names, seqs, quals)

    def add_rows(self, text, text_len, rows, names=None):
        """names: what the reads are called, where that is not the name the rows point at (the read filter's -r serials)"""
        lo = 0
        for i, l in enumerate(rows['len'].tolist()):
            if self.count and self.acc + l > self.batch_bases:
                if i > lo:
                    self.pieces.append(('rows', text, text_len, rows[lo:i], names and names[lo:i]))
                yield self._build()
                lo = i
            self.acc += l
            self.count += 1
        if lo < len(rows):
            self.pieces.append(('rows', text, text_len, rows[lo:], names and names[lo:]))

    def add_host(self, name, seq, qual):
        if self.count and self.acc + len(seq) > self.batch_bases:
            yield self._build()
        if not self.pieces or self.pieces[-1][0] != 'host':
            self.pieces.append(('host', [], [], []))
        _, names, seqs, quals = self.pieces[-1]
        names.append(name)
        seqs.append(seq)
        quals.append(qual)
        self.acc += len(seq)
        self.count += 1

    def flush(self):
        if self.count:
            yield self._build()

    def _build(self):
        import time
        import torch
        from . import mapper
        pieces, self.pieces, self.acc, self.count = self.pieces, [], 0, 0
        if all(p[0] == 'host' for p in pieces):       # nothing of it is on the device yet: the batch of the host loop
            return mapper.PackedReads([n for p in pieces for n in p[1]], [s for p in pieces for s in p[2]], device=self.device,
                                      quals=[q for p in pieces for q in p[3]])
        t0 = time.perf_counter()
        parts, names, lens = [], [], []
        for p in pieces:
            if p[0] == 'rows':
                _, text, text_len, rows, given = p
                seq, qual, nm = fastq_gather(text, text_len, rows)
                nm = given or nm
                _tick(self.timings, 'gather_device_ms', last_fastq_device_ms()[1])
                parts.append((seq, qual, int(rows['len'].astype(np.int64).sum())))
                lens.append(rows['len'].astype(np.int32))
            else:     # host records next to '@' records: the batch has qualities, a read without them gets '!' (mapper.PackedReads)
                _, nm, seqs, quals = p
                buf, _, ln = mapper.pack_seqs(seqs)
                qbuf = mapper.pack_seqs([q if q is not None else b'!' * int(l) for q, l in zip(quals, ln)])[0]
                parts.append((torch.from_numpy(buf).to(self.device), torch.from_numpy(qbuf).to(self.device), int(ln.astype(np.int64).sum())))
                lens.append(ln)
            names += nm
        return _join_batch(parts, names, np.concatenate(lens), True, self.device, self.timings, t0, 'gather')


class _ChunkTexts:
    """The text of a stream of FASTQ bytes (a plain file, or what zlib inflates of a gzip stream) in HBM, MPN_INGEST_BATCH_BYTES at a
    time, behind the carry.  read_key: where the time spent in the stream's read is booked ('read', or 'inflate' for zlib)."""

    def __init__(self, stream, device, timings=None, read_key='read'):
        import torch
        self.torch, self.stream, self.device, self.timings, self.read_key = torch, stream, device, timings, read_key
        self.chunk = max(1, batch_bytes())
        self.staging = torch.empty(min(self.chunk, FASTQ_STAGING), dtype=torch.uint8).pin_memory()

    def next_text(self, carry):
        import time
        torch = self.torch
        parts = [] if carry is None or not carry.numel() else [carry]
        got, eof, view = 0, False, self.staging.numpy()
        while got < self.chunk and not eof:
            t0 = time.perf_counter()
            want, k = min(len(view), self.chunk - got), 0
            while k < want:
                m = self.stream.readinto(memoryview(view)[k:want])
                if not m:
                    eof = True
                    break
                k += m
            t1 = time.perf_counter()
            if k:
                parts.append(self.staging[:k].to(self.device))      # (returns when the copy is done: the buffer is filled again)
                got += k
            _tick(self.timings, self.read_key, t1 - t0)
            _tick(self.timings, 'h2d', time.perf_counter() - t1)
        final = eof or not self.stream.peek(1)
        pad = torch.zeros(16, dtype=torch.uint8, device=self.device)
        text = torch.cat(parts + [pad])
        return text, text.numel() - 16, final


class _TailThenStream:
    """readline() over `tail` (bytes) and then over `stream`: what fastx.iter_fastx reads when the device hands a file over."""

    def __init__(self, tail, stream):
        self.tail, self.stream = io.BytesIO(tail), stream

    def readline(self):
        line = self.tail.readline() if self.tail is not None else b''
        if line.endswith(b'\n'):
            return line
        self.tail = None
        return line + self.stream.readline()

    def read(self):
        """all that is left (the read filter's host path parses whole texts)"""
        rest = self.tail.read() if self.tail is not None else b''
        self.tail = None
        return rest + self.stream.read()


def iter_fastq_read_batches(stream, batch_bases=200_000_000, device='cuda', timings=None, form='plain', batcher=None):
    """The reads of one FASTQ stream as mapper.PackedReads of at most batch_bases each, resident on the device, with the records of
    fastx.iter_fastx.  stream: the file's own bytes from their first one (fastx.open_query; read to its end, not closed); form: what
    they are, 'plain', 'gzip' (inflated by zlib here, as a stream) or 'bgzf' (inflated on the device, block by block).  With a
    ReadBatcher of the caller's the reads join the batch it holds and the last batch stays in it, for the next file to fill."""
    import time
    device = device or 'cuda'
    own = batcher is None
    if own:
        batcher = ReadBatcher(batch_bases, device, timings)
    if form == 'bgzf':
        texts, rest = _BgzfTexts(stream, device, timings), None         # (the blocks that were not framed yet are a gzip stream)
    elif form in ('plain', 'gzip'):
        rest = stream if form == 'plain' else fastx.gzip_text(stream)
        texts = _ChunkTexts(rest, device, timings, 'read' if form == 'plain' else 'inflate')
    else:
        raise ValueError(f'iter_fastq_read_batches: form {form!r}')
    carry = None
    while True:
        text, text_len, final = texts.next_text(carry)
        t0 = time.perf_counter()
        rows, consumed, status, ms = fastq_scan(text, text_len, final)
        _tick(timings, 'scan', time.perf_counter() - t0)
        _tick(timings, 'scan_device_ms', ms)
        _tick(timings, 'records', len(rows))
        yield from batcher.add_rows(text, text_len, rows)
        if status == FASTQ_UNSUPPORTED:
            # the rest of the file for the host: iter_fastx is stateless at a record start
            t0 = time.perf_counter()
            tail = text[consumed:text_len].cpu().numpy().tobytes()
            del text, rows, carry
            host = _TailThenStream(tail, rest if rest is not None else fastx.gzip_text(stream))
            n = 0
            for name, seq, qual in fastx.iter_fastx(host):
                yield from batcher.add_host(name, seq, qual)
                n += 1
            _tick(timings, 'host_records', n)
            _tick(timings, 'host', time.perf_counter() - t0)
            break
        if status != OK:
            raise _ffi.MpnError(f'mpn_fastq_scan: status {status}')
        if final:
            break
        carry = text[consumed:text_len]
    if own:
        yield from batcher.flush()
