"""Realignment of a sorted BAM's reads around variant support on the GPU: a drop-in for the reference's
realignment/realign_illumina_reads.py, step 1 of realignment/realignment.sh -p illumina.  The rules, the quirks that are reproduced
and the differences are DESIGN.md section 6 item 23; the native calls are include/mpn_read_realign.h.

    realign_file(bam_fn, ref_fn, ctg_name, out)          writes the script's SAM text (`--read_fn PIPE`) to the binary stream `out`
    realign_to_bam(bam_fn, ref_fn, ctg_name, out_bam)    the same records as a coordinate-sorted BAM with its .bai
    bin/mpn-realign-reads                                the command line of the script

The BAM goes to HBM group by group (MPN_INGEST_BATCH_BYTES) through ingest.BamTexts; no samtools, .bai, .fai, pypy or intervaltree is
used.  On the device: what every record says (mpn_rr_records), the script's pileup[...]["X"] counter as one row of 5041 positions per
yield of its generator (mpn_rr_support; a row that records of two texts reach is added to by both calls), the candidates of a row
(a compare and a compaction on the row where it lies), find_max_overlap_index over all member reads for the windows of a chunk's five
splits (mpn_rr_assign), and per chunk the graph consensus and the realigner over all its windows (realigner.realign_windows).  On the
host: the chunk recurrence (mpn_rr_chunks, serial), the window rules, the fold of set_realignment_info, the flush and the text.

MPN_RR_SLICE (default 256, include/mpn_read_realign.h): the records of a row one workgroup takes; anything but a number raises
ValueError."""
import ctypes as ct
import gzip
import os
import re
import string
import struct
import sys
import tempfile
import time

import numpy as np

from . import _ffi, candidates, clair_tensor, ingest, realigner
from ._ffi import check as _check, ptr as _p

ROW, CHUNK, EXPAND = 5041, 5000, 20         # MPN_RR_ROW, realign_chunk_size, region_expansion_in_bp
WINDOW_GAP, WINDOW_PAD, MAX_WINDOW, MAX_READS = 160, 80, 1000, 1000
SPLIT, N_SPLITS = 1000, 5
GRAPH_MQ, GRAPH_BQ = 14, 15                 # graph_min_mapping_quality, the quality below which a base is left out of the graph
COUNT_MQ = 20                               # min_dbg_mapping_quality
CHAR_STR = string.digits + string.ascii_lowercase + string.ascii_uppercase + '!#$%&()*+./:;<=>?[]^`{|}~'     # the 87 digits of a name
NAME_LEN = 5
OPS = 'MIDNSHP=X'
RR_REC = np.dtype([('soft', '<i8'), ('total', '<i8'), ('del', '<i8'), ('span', '<i8'), ('ref_id', '<i4'), ('pos', '<i4'), ('l_seq', '<i4'),
                   ('next_ref', '<i4'), ('next_pos', '<i4'), ('flag', '<u2'), ('n_cigar', '<u2'), ('mapq', 'u1'), ('has_seq', 'u1'), ('has_qual', 'u1'),
                   ('hp', 'u1'), ('status', 'u1'), ('clipped', 'u1'), ('reserved', 'u1', (2,))])                                             # mpn_rr_rec
RR_TAKE = np.dtype([('off', '<i8'), ('pos', '<i4'), ('chunk_start', '<i4'), ('chunk', '<i4'), ('reserved', '<i4')])     # mpn_rr_take
OK, PAST, BAD_OP, PLACEHOLDER, BAD_AUX, HP_TEXT, BASE_EQ, NO_BASE = range(8)
WHY = {PAST: 'the CIGAR, the bases, the qualities or an aux field pass the end of the record', BAD_OP: 'a CIGAR operation code above 8',
       PLACEHOLDER: 'the CIGAR is kept in a CG tag (more than 65535 operations): not taken',
       BAD_AUX: 'an aux field of a type that is not one of A c C s S i I f Z H B', HP_TEXT: 'a Z or H aux value holds the text HP:i:',
       BASE_EQ: 'a base `=` (the reference script raises there)',
       NO_BASE: 'the CIGAR runs past the bases of the record (the reference script raises there)'}

_bound = False


def _lib():
    global _bound
    lib = clair_tensor._lib()
    if not _bound:
        P, I64, I32 = ct.c_void_p, ct.c_int64, ct.c_int32
        lib.mpn_rr_records.argtypes = [P, I64, I64, P, P]
        lib.mpn_rr_chunks.argtypes = [I64, P, P, P, P]
        lib.mpn_rr_support.argtypes = [P, I64, I64, P, P, I64, P, P, P, I64, I32, P, P, P]
        lib.mpn_rr_assign.argtypes = [I64, P, P, I32, P, P, P, P, P, I64]
        for f in (lib.mpn_rr_records, lib.mpn_rr_chunks, lib.mpn_rr_support, lib.mpn_rr_assign):
            f.restype = I32
        lib.mpn_rr_last_device_ms.argtypes = [ct.POINTER(ct.c_double)] * 3
        lib.mpn_rr_last_device_ms.restype = None
        _bound = True
    return lib


def last_device_ms():
    """-> (records ms, support ms, assign ms) of the calling thread's last native calls"""
    return _ffi.device_ms(_lib().mpn_rr_last_device_ms, 3)


def slice_records():
    """MPN_RR_SLICE: unset or 0 = MPN_RR_SLICE of the header, else the records of a row one workgroup takes"""
    how = os.environ.get('MPN_RR_SLICE', '0')
    if not how.isdigit() or int(how) > 0x7fffffff:
        raise ValueError(f'MPN_RR_SLICE={how}: expected a number of records, 0 .. 2147483647')
    return int(how)


# ---- the native calls ---------------------------------------------------------------------------------------------------------------
def rr_records(text, text_len, rows):
    """mpn_rr_records on rows of ingest.bam_walk -> an RR_REC array"""
    rows = np.ascontiguousarray(rows, dtype=ingest.BAM_ROW)
    recs = np.zeros(len(rows), dtype=RR_REC)
    _check(_lib().mpn_rr_records(text.data_ptr(), int(text_len), len(rows), _p(rows), _p(recs)), 'mpn_rr_records')
    return recs


def rr_chunks(pos, first=-1, chunk=0):
    """mpn_rr_chunks -> (chunk_of, first, chunk)"""
    pos = np.ascontiguousarray(pos, dtype=np.int32)
    chunk_of = np.zeros(len(pos), dtype=np.int32)
    f, c = ct.c_int64(first), ct.c_int64(chunk)
    _check(_lib().mpn_rr_chunks(len(pos), _p(pos), ct.byref(f), ct.byref(c), _p(chunk_of)), 'mpn_rr_chunks')
    return chunk_of, f.value, c.value


def rr_support(text, text_len, takes, reach, epoch_chunk, row_lo, contig, rows, slice_=0):
    """mpn_rr_support: adds to `rows` ((epochs, 5041) int32 on the device) -> (bad row or -1, rows that were split)"""
    takes, reach = np.ascontiguousarray(takes, dtype=RR_TAKE), np.ascontiguousarray(reach, dtype=np.int64)
    epoch_chunk, row_lo = np.ascontiguousarray(epoch_chunk, dtype=np.int32), np.ascontiguousarray(row_lo, dtype=np.int32)
    assert rows.is_contiguous() and rows.numel() == len(epoch_chunk) * ROW and len(reach) == len(takes) and len(row_lo) == len(epoch_chunk)
    bad, split = ct.c_int64(-1), ct.c_int64(0)
    import torch
    torch.cuda.current_stream(rows.device).synchronize()          # the native layer uses the default stream
    _check(_lib().mpn_rr_support(text.data_ptr(), int(text_len), len(takes), _p(takes), _p(reach), len(epoch_chunk), _p(epoch_chunk), _p(row_lo),
                                 contig.data_ptr(), contig.numel(), int(slice_), rows.data_ptr(), ct.byref(bad), ct.byref(split)), 'mpn_rr_support')
    return bad.value, split.value


def rr_assign(pos, end, splits):
    """mpn_rr_assign.  splits: per split the list of its windows (start, end) -> per split, per window, the indices of its reads (an
    int32 array, in member order)"""
    pos, end = np.ascontiguousarray(pos, dtype=np.int32), np.ascontiguousarray(end, dtype=np.int32)
    begin = np.zeros(len(splits) + 1, dtype=np.int32)
    begin[1:] = np.cumsum([len(s) for s in splits])
    flat = [w for s in splits for w in s]
    ws = np.array([w[0] for w in flat], dtype=np.int32)
    we = np.array([w[1] for w in flat], dtype=np.int32)
    count = np.zeros(max(len(flat), 1), dtype=np.int32)
    cap = max(len(pos) * len(splits), 1)
    out = np.zeros(cap, dtype=np.int32)
    _check(_lib().mpn_rr_assign(len(pos), _p(pos), _p(end), len(splits), _p(begin), _p(ws), _p(we), _p(count), _p(out), cap), 'mpn_rr_assign')
    off = np.concatenate([[0], np.cumsum(count[:len(flat)])])
    return [[out[int(off[w]):int(off[w + 1])] for w in range(int(begin[s]), int(begin[s + 1]))] for s in range(len(splits))]


# ---- the script's small rules -------------------------------------------------------------------------------------------------------
def read_name(index):
    """simplfy_read_name: the 5-character name of the record's index among the contig's viewed records"""
    index %= len(CHAR_STR) ** NAME_LEN
    out = []
    for _ in range(NAME_LEN):
        index, d = divmod(index, len(CHAR_STR))
        out.append(CHAR_STR[d])
    return ''.join(reversed(out))


def chunk_windows(cand, chunk_start):
    """cand: the ascending candidate positions of a row -> per split the windows (start, end): merged while pos <= end + 160, padded
    by 80.  A position in the 41 bases that two splits share belongs to both."""
    cand = np.asarray(cand, dtype=np.int64)
    splits = []
    for s in range(N_SPLITS):
        a = chunk_start + s * SPLIT - EXPAND - 1
        p = cand[(cand >= a) & (cand < a + SPLIT + 2 * EXPAND + 1)]
        if not len(p):
            splits.append([])
            continue
        cut = np.flatnonzero(np.diff(p) > WINDOW_GAP)
        first, last = p[np.concatenate([[0], cut + 1])], p[np.concatenate([cut, [len(p) - 1]])]
        splits.append(list(zip((first - WINDOW_PAD).tolist(), (last + WINDOW_PAD).tolist())))
    return splits


_INDEL = re.compile(r'(\d+)([ID])')


class Read:
    __slots__ = ('index', 'pos', 'end', 'mapq', 'flag', 'cigar', 'seq', 'qual', 'rnext', 'pnext', 'hp', 'best_pos', 'best_cigar', 'best_score', 'low')

    def realigned(self, position, cigar):
        """set_realignment_info"""
        cigar = cigar.replace('X', 'M')
        if cigar == self.cigar and position == self.pos:
            return
        if self.best_score and cigar == self.best_cigar and position == self.best_pos:
            return
        score = sum(int(m.group(1)) for m in _INDEL.finditer(cigar))
        if not self.best_score or score >= self.best_score:       # (a best score of 0 counts as none: the script's test)
            self.best_cigar, self.best_pos, self.best_score = cigar, position, score

    def line(self, ctg_name, with_empty_field=True):
        tail = [f'HP:i:{self.hp}'] if self.hp else ([''] if with_empty_field else [])
        return '\t'.join([read_name(self.index), str(self.flag), ctg_name, str(self.best_pos + 1), str(self.mapq), self.best_cigar, self.rnext,
                          self.pnext, self.pnext, self.seq, self.qual] + tail) + '\n'


def bam_header_text(bam_fn):
    """-> the header text of a BAM file; @SQ lines are made from its reference list if the text has none"""
    with gzip.open(bam_fn, 'rb') as f:
        head = f.read(8)
        if len(head) < 8 or head[:4] != b'BAM\1':
            raise ValueError(f'{bam_fn}: not a BAM file')
        text = f.read(struct.unpack('<i', head[4:])[0]).rstrip(b'\0').decode()
    if text and not text.endswith('\n'):
        text += '\n'
    if not any(l.startswith('@SQ') for l in text.splitlines()):
        text += ''.join(f'@SQ\tSN:{n}\tLN:{l}\n' for n, l in candidates.bam_references(bam_fn))
    return text


# ---- the file -----------------------------------------------------------------------------------------------------------------------
class _Run:
    def __init__(self, bam_fn, ctg_name, contig, d_contig, ref_names, tid, min_mq, min_coverage, sink, timings, trace):
        self.bam_fn, self.ctg_name, self.contig, self.d_contig, self.ref_names, self.tid = bam_fn, ctg_name, contig, d_contig, ref_names, tid
        self.min_mq, self.min_coverage, self.sink, self.timings, self.trace = min_mq, min_coverage, sink, timings, trace
        self.first, self.chunk, self.n_viewed, self.last_pos = -1, 0, 0, None
        self.members, self.pending = [], {}
        self.n_written = self.n_changed = self.n_windows = 0

    def tick(self, key, value):
        ingest._tick(self.timings, key, value)

    # -- one text ------------------------------------------------------------------------------------------------------------------
    def text(self, t):
        import torch
        text, text_len = t.text, t.text_len
        t0 = time.perf_counter()
        recs = rr_records(text, text_len, t.rows)
        self.tick('records_device_ms', last_device_ms()[0])
        on = np.flatnonzero((recs['ref_id'] == self.tid) & ((recs['mapq'] >= self.min_mq) if self.min_mq > 0 else True))
        rows, recs = t.rows[on], recs[on]

        def refuse(i, why):
            raise ValueError(f'{self.bam_fn}: record {candidates._record_name(text, rows[int(i)])}: {why}')
        pos = recs['pos'].astype(np.int64)
        bad = np.flatnonzero(pos < 0)
        if len(bad):
            refuse(bad[0], 'a record of the contig without a position')
        self.last_pos = candidates.check_ascending(pos, self.last_pos, lambda i: f'{self.bam_fn}: record {candidates._record_name(text, rows[i])}: the records '
                                                   f'of {self.ctg_name} are not sorted by position')
        bad = np.flatnonzero(np.isin(recs['status'], (PAST, BAD_OP, PLACEHOLDER, BAD_AUX, HP_TEXT)))
        if len(bad):
            refuse(bad[0], WHY[int(recs['status'][bad[0]])])
        # the reference: skip a read without a CIGAR or less than 55% aligned (rr_too_clipped of csrc/read_realign_core.h, in the record)
        taken = (recs['n_cigar'] > 0) & (recs['clipped'] == 0)
        bad = np.flatnonzero(taken & np.isin(recs['status'], (NO_BASE, BASE_EQ)))
        if len(bad):
            refuse(bad[0], WHY[int(recs['status'][bad[0]])])
        bad = np.flatnonzero(taken & ((recs['has_seq'] == 0) | (recs['has_qual'] == 0)))
        if len(bad):
            refuse(bad[0], 'no bases or no qualities (the reference script raises there)')
        bad = np.flatnonzero(taken & (pos + recs['span'] > len(self.contig)))
        if len(bad):
            refuse(bad[0], 'the record runs past the end of the contig (the reference script raises there)')
        chunk_before = self.chunk
        chunk_of, self.first, self.chunk = rr_chunks(recs['pos'], self.first, self.chunk)
        index0 = self.n_viewed
        self.n_viewed += len(recs)
        self.tick('records', time.perf_counter() - t0)

        # the counter: every row that a record of this text can reach
        t1 = time.perf_counter()
        cnt = np.flatnonzero(taken & (recs['mapq'] >= COUNT_MQ))
        if len(cnt):
            c = recs[cnt]
            takes = np.zeros(len(cnt), dtype=RR_TAKE)
            takes['off'], takes['pos'], takes['chunk'] = rows['off'][cnt], c['pos'], chunk_of[cnt]
            takes['chunk_start'] = self.first + CHUNK * chunk_of[cnt].astype(np.int64)
            reach = c['l_seq'].astype(np.int64) + c['span']
            base = self.first - EXPAND - 1
            klo = -((-(c['pos'].astype(np.int64) - c['l_seq'] - base - (ROW - 1))) // CHUNK)
            khi = (c['pos'].astype(np.int64) + reach - 1 - base) // CHUNK
            klo = np.maximum(klo, chunk_of[cnt])
            n = np.maximum(khi - klo + 1, 0)
            ks = np.unique(np.repeat(klo, n) + np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n))
            d_rows = torch.zeros((max(len(ks), 1), ROW), dtype=torch.int32, device=text.device)
            for i, k in enumerate(ks.tolist()):
                if k in self.pending:
                    d_rows[i] = self.pending[k]
            if len(ks):
                bad_row, _ = rr_support(text, text_len, takes, reach, ks, base + CHUNK * ks, self.d_contig, d_rows, slice_records())
                self.tick('support_device_ms', last_device_ms()[1])
                if bad_row >= 0:
                    refuse(cnt[bad_row], 'a base, a quality or a contig base that the CIGAR needs is not there')
            for i, k in enumerate(ks.tolist()):
                self.pending[k] = d_rows[i].clone()                     # (a view would keep the whole block of this text's rows alive)
        self.tick('support', time.perf_counter() - t1)

        # the reads of this text, and the chunks that end in it
        t2 = time.perf_counter()
        tk = np.flatnonzero(taken)
        reads = self.host_reads(text, text_len, rows[tk], recs[tk], index0 + tk) if len(tk) else []
        self.tick('host_reads', time.perf_counter() - t2)
        at = 0
        for i in np.flatnonzero(np.diff(chunk_of, prepend=chunk_before)).tolist():     # record i triggers the yield of the chunk before its own
            n_before = int(np.searchsorted(tk, i))
            self.members += reads[at:n_before]
            at = n_before
            self.yield_chunk(int(chunk_of[i]) - 1)
        self.members += reads[at:]

    def host_reads(self, text, text_len, rows, recs, index):
        """the taken records of a text as host objects: the CIGAR text, the bases and the quality text as samtools prints them"""
        import torch
        plain = rows.copy()
        plain['flag'] = 0                      # (the bases as they are stored: nothing is reversed)
        seq, qual, _ = ingest.bam_decode(text, text_len, plain, True)
        seq, qual = seq.cpu().numpy().tobytes().decode('latin-1'), qual.cpu().numpy().tobytes().decode('latin-1')
        n_cigar = recs['n_cigar'].astype(np.int64)
        c_off = rows['off'] + 36 + rows['l_read_name'].astype(np.int64)
        first = np.cumsum(n_cigar) - n_cigar
        where = np.repeat(c_off, n_cigar) + 4 * (np.arange(int(n_cigar.sum()), dtype=np.int64) - np.repeat(first, n_cigar))
        words = text[torch.from_numpy(where[:, None] + np.arange(4, dtype=np.int64)).to(text.device)].cpu().numpy().astype(np.uint32)
        words = words[:, 0] | (words[:, 1] << 8) | (words[:, 2] << 16) | (words[:, 3] << 24)
        ops = [f'{w >> 4}{OPS[w & 15]}' for w in words.tolist()]
        out, a = [], 0
        tid, names = self.tid, self.ref_names
        for k in range(len(rows)):
            rec = recs[k]
            r = Read()
            n, l = int(n_cigar[k]), int(rec['l_seq'])
            r.index, r.pos, r.mapq, r.flag = int(index[k]), int(rec['pos']), int(rec['mapq']), int(rec['flag'])
            r.end = r.pos + l + int(rec['del'])                              # the script's read_end: not htslib's
            r.cigar = ''.join(ops[int(first[k]):int(first[k]) + n])
            r.seq, r.qual = seq[a:a + l], qual[a:a + l]
            a += l
            nr = int(rec['next_ref'])
            r.rnext = '*' if nr < 0 or nr >= len(names) else ('=' if nr == tid else names[nr])
            r.pnext = str(int(rec['next_pos']) + 1)
            r.hp = chr(int(rec['hp'])) if rec['hp'] else None
            r.best_pos, r.best_cigar, r.best_score, r.low = r.pos, r.cigar, None, None
            out.append(r)
        return out

    # -- one yield -----------------------------------------------------------------------------------------------------------------
    def yield_chunk(self, k):
        import torch
        chunk_start = self.first + CHUNK * k
        row = self.pending.get(k)
        for old in [x for x in self.pending if x <= k]:
            del self.pending[old]
        lo = chunk_start - EXPAND - 1
        if row is None:
            cand = np.zeros(0, dtype=np.int64)
        else:
            cand = torch.nonzero(row.to(torch.float64) >= float(self.min_coverage)).reshape(-1).cpu().numpy().astype(np.int64) + lo
        entry = None
        if self.trace is not None:
            entry = dict(chunk_start=chunk_start, row=np.zeros(ROW, dtype=np.int32) if row is None else row.cpu().numpy().copy(), windows=None, members=None)
            self.trace.append(entry)
        members = self.members
        if not members or not len(cand):
            return
        t0 = time.perf_counter()
        splits = chunk_windows(cand, chunk_start)
        lists = rr_assign([r.pos for r in members], [r.end for r in members], splits)
        self.tick('assign_device_ms', last_device_ms()[2])
        if entry is not None:
            entry['windows'] = splits
            entry['members'] = [[[members[i].index for i in w.tolist()] for w in s] for s in lists]
        t1 = time.perf_counter()
        contig, todo, who = self.contig, [], []
        for windows, of_split in zip(splits, lists):
            for (start, end), idx in zip(windows, of_split):
                if end - start > MAX_WINDOW or not len(idx):
                    continue
                if start < 0:
                    print(f'{self.ctg_name}:{start}-{end}: window left out: the reference script slices its reference with a negative index there',
                          file=sys.stderr)
                    continue
                reads = [members[i] for i in idx.tolist()]
                graph = [r for r in reads if r.mapq >= GRAPH_MQ and not (r.pos > end or r.end < start)]
                for r in graph:
                    if r.low is None:
                        r.low = np.flatnonzero(np.frombuffer(r.qual.encode('latin-1'), dtype=np.uint8) < GRAPH_BQ + 33).tolist()
                ref_start = max(0, min(min(r.pos for r in reads), start) - EXPAND)
                ref_end = max(max(r.end for r in reads), end) + EXPAND
                todo.append(dict(ref=contig[start:end], graph_reads=[r.seq for r in graph], graph_bad=[r.low for r in graph],
                                 ref_prefix=contig[ref_start:start], ref_suffix=contig[end:ref_end], seqs=[r.seq for r in reads[:MAX_READS]],
                                 positions=[r.pos for r in reads[:MAX_READS]], cigars=[r.cigar for r in reads[:MAX_READS]], ref_start=ref_start))
                who.append(reads[:MAX_READS])
        t2 = time.perf_counter()
        results = realigner.realign_windows(todo) if todo else []
        self.tick('consensus_device_ms', realigner.consensus_device_ms() if todo else 0.0)
        t3 = time.perf_counter()
        self.n_windows += len(todo)
        for reads, res in zip(who, results):          # split by split, window by window: the order of the script's fold
            if res is None:
                continue
            for r, (position, cigar) in zip(reads, res):
                if cigar == '' or (r.cigar == cigar and r.pos == position):
                    continue
                r.realigned(position, cigar)
        # the flush: what lies a safe distance before the chunk is written, in the order of its best position
        limit = chunk_start - EXPAND - MAX_WINDOW
        self.write([r for r in sorted(members, key=lambda r: r.best_pos) if r.best_pos < limit])
        self.members = [r for r in members if r.best_pos >= limit]
        for key, dt in (('assign', t1 - t0), ('marshal', t2 - t1), ('realign_windows', t3 - t2), ('fold_flush', time.perf_counter() - t3)):
            self.tick(key, dt)

    def write(self, reads):
        for r in reads:
            self.n_changed += r.best_cigar != r.cigar or r.best_pos != r.pos
        self.n_written += len(reads)
        self.sink(reads)

    def finish(self):
        if self.first < 0:
            return
        self.yield_chunk(self.chunk)                                       # the last yield, behind the last record
        self.write(sorted(self.members, key=lambda r: r.best_pos))
        self.members = []
        self.pending.clear()                                               # (rows behind the last chunk: reached by a record, never yielded)


def _realign(bam_fn, ref_fn, ctg_name, sink, min_mq, min_coverage, device, timings, trace):
    import torch
    device = device or 'cuda'
    _lib()
    seq = candidates.read_contig(ref_fn, ctg_name)
    if not seq:
        raise ValueError(f'[ERROR] Failed to load reference seqeunce from file ({ref_fn}).')
    contig = bytes(seq).upper()                                            # the script upper-cases what faidx gives it
    d_contig = torch.from_numpy(np.frombuffer(contig, dtype=np.uint8).copy()).to(device)
    refs = candidates.bam_references(bam_fn)
    names = [n for n, _ in refs]
    run = _Run(bam_fn, ctg_name, contig.decode('latin-1'), d_contig, names, names.index(ctg_name) if ctg_name in names else -2, int(min_mq),
               float(min_coverage), sink, timings, trace)
    with ingest.BamTexts(bam_fn, device, timings) as texts:
        for t in texts:
            run.text(t)
    run.finish()
    return dict(viewed=run.n_viewed, reads=run.n_written, windows=run.n_windows, changed=run.n_changed)


def realign_file(bam_fn, ref_fn, ctg_name, out, min_mq=5, min_coverage=2.0, device='cuda', timings=None, trace=None):
    """Writes the text of `realign_illumina_reads.py --read_fn PIPE` to `out` (a binary stream): the header of the BAM, then one line
    per kept read of ctg_name -- the 5-character name of its index among the contig's viewed records, FLAG, the contig, the best
    position + 1, MAPQ, the best CIGAR, RNEXT, PNEXT, PNEXT again where TLEN belongs (the script's bug), the bases, the qualities,
    and `HP:i:<d>` or an empty last field.  Nothing is written for a contig without a record.  -> dict(viewed, reads, windows,
    changed).  ValueError names the record, before anything is written: records of the contig that are not sorted; a CIGAR with an
    operation code above 8 or kept in a CG tag; a Z or H aux value that holds `HP:i:`; and among the records that are kept one
    without bases or qualities, with a base `=`, with a CIGAR past its bases, or that runs past the contig's end.  A window that
    starts below 0 is left out with a message on standard error.  trace: a list that gets, per yield, dict(chunk_start, row,
    windows, members) for the tests."""
    with tempfile.SpooledTemporaryFile(max_size=256 << 20) as spool:       # a refusal comes before any output
        def sink(reads):
            spool.write(''.join(r.line(ctg_name) for r in reads).encode('latin-1'))
        got = _realign(bam_fn, ref_fn, ctg_name, sink, min_mq, min_coverage, device, timings, trace)
        if got['viewed']:
            out.write(bam_header_text(bam_fn).encode())
            spool.seek(0)
            while True:
                piece = spool.read(16 << 20)
                if not piece:
                    break
                out.write(piece)
    return got


def realign_to_bam(bam_fn, ref_fn, ctg_name, out_bam, min_mq=5, min_coverage=2.0, device='cuda', timings=None):
    """The records of realign_file (without the empty last field) as a coordinate-sorted BAM with its .bai, through the host writer
    bam.sam_to_sorted_bam.  A contig without a record gives a BAM with the header and no record.  -> dict(viewed, reads, windows,
    changed)."""
    from . import bam
    with tempfile.TemporaryDirectory() as tmp:
        sam = os.path.join(tmp, 'realigned.sam')
        with open(sam, 'wb') as f:
            f.write(bam_header_text(bam_fn).encode())

            def sink(reads):
                f.write(''.join(r.line(ctg_name, with_empty_field=False) for r in reads).encode('latin-1'))
            got = _realign(bam_fn, ref_fn, ctg_name, sink, min_mq, min_coverage, device, timings, None)
        t0 = time.perf_counter()
        bam.sam_to_sorted_bam(sam, out_bam)
        ingest._tick(timings, 'write_bam', time.perf_counter() - t0)
    return got


def main(argv, prog='mpn-realign-reads'):
    """The command line of realign_illumina_reads.py."""
    from argparse import ArgumentParser
    ap = ArgumentParser(prog=prog, description='Realign the reads of a sorted BAM around variant support (on the GPU)')
    ap.add_argument('--bam_fn', type=str, default='input.bam', help='sorted BAM file')
    ap.add_argument('--ref_fn', type=str, default='ref.fa', help='reference FASTA, plain or gzip (no .fai is needed)')
    ap.add_argument('--ctgName', type=str, default='chr17', help='the contig')
    ap.add_argument('--minMQ', type=int, default=5, help='records with a lower mapping quality are not viewed')
    ap.add_argument('--minCoverage', type=float, default=2, help='support from which a position is a candidate')
    ap.add_argument('--read_fn', type=str, default='PIPE', help='PIPE for standard output, or the path of the BAM to write (with its .bai)')
    ap.add_argument('--bed_fn', type=str, default=None, help='refused')
    ap.add_argument('--extend_confident_bed_fn', type=str, default=None, help='refused')
    for name, kind in (('--samtools', str), ('--ctgStart', int), ('--ctgEnd', int), ('--threshold', float), ('--chunk_id', int), ('--chunk_num', int),
                       ('--test_pos', int)):
        ap.add_argument(name, type=kind, default=None, help='accepted and ignored, as the script ignores or overwrites it')
    if not argv:
        ap.print_help()
        return 1
    a = ap.parse_args(argv)
    if a.bed_fn is not None or a.extend_confident_bed_fn is not None:
        print(f'{prog}: --bed_fn and --extend_confident_bed_fn are not taken (the script turns them into `samtools view -L`)', file=sys.stderr)
        return 2
    try:
        if a.read_fn == 'PIPE':
            realign_file(a.bam_fn, a.ref_fn, a.ctgName, sys.stdout.buffer, min_mq=a.minMQ, min_coverage=a.minCoverage)
            sys.stdout.buffer.flush()
        else:
            realign_to_bam(a.bam_fn, a.ref_fn, a.ctgName, a.read_fn, min_mq=a.minMQ, min_coverage=a.minCoverage)
    except (ValueError, OSError) as e:
        print(f'{prog}: {e}', file=sys.stderr)
        return 1
    return 0
