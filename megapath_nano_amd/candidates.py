"""The per-base pile-up of a sorted BAM on the GPU, and on top of it a drop-in for Clair's preprocess/ExtractVariantCandidates.py
(make_candidates without --gen4Training): per-position allele counts and the list of candidate sites.  The rules, the quirks of the
reference that are reproduced and the differences are DESIGN.md section 6; the native calls are include/mpn_pileup.h.

    pileup(bam, ctg_name, ...)                     -> Pileup: the window and its (n, 7) int32 counters A C G T I D N, resident
    extract_variant_candidates(bam_fn, ref_fn, ..) -> writes the reference's lines
    bin/mpn-candidates                             the command line of the reference script

The BAM goes to HBM group by group (MPN_INGEST_BATCH_BYTES) through ingest.BamTexts, as read input does: the file is never whole
in host memory and no .bai is read.  What the stages that read a sorted BAM share is here too: contig_tid, contig_records,
check_ascending.  What is taken -- flags, contig, MAPQ, the 0.55 soft-clip test in numpy
float64, the first-of-POS rule for leading insertions and deletions -- is decided here from the per-record table of
mpn_pileup_records; the counters and the decision per position stay on the device."""
import collections
import ctypes as ct
import gzip
import io
import struct
import sys
import time

import numpy as np

from . import _ffi, fastx, ingest

FILTER_FLAG = 2316          # param.SAMTOOLS_VIEW_FILTER_FLAG: unmapped, mate unmapped, secondary, supplementary
LABELS = 'ACGTIDN'
SLOTS = 7
PILE_REC = np.dtype([('soft', '<i8'), ('total', '<i8'), ('span', '<i8'), ('ref_id', '<i4'), ('pos', '<i4'), ('n_cigar', '<u2'), ('mapq', 'u1'),
                     ('status', 'u1'), ('reserved', '<i4')])                                                      # mpn_pileup_rec
PILE_TAKE = np.dtype([('off', '<i8'), ('pos', '<i4'), ('lead', '<i4')])                                          # mpn_pileup_take
PILE_CAND = np.dtype([('pos', '<i4'), ('depth', '<i4'), ('count', '<i4', (SLOTS,)), ('label', 'u1', (SLOTS,)), ('ref_base', 'u1')])   # mpn_pileup_cand
OK, CIGAR_PAST, BAD_OP, PLACEHOLDER, NO_BASE = range(5)
STATUS_TEXT = {CIGAR_PAST: 'the CIGAR or the bases pass the end of the record', BAD_OP: 'a CIGAR operation code above 8',
               PLACEHOLDER: 'the CIGAR is kept in a CG tag (more than 65535 operations): not taken',
               NO_BASE: 'a matched stretch reaches past the bases of the record (the reference script raises there)'}
NO_READ = ('No read has been process, either the genome region you specified has no read cover, or please check the correctness of your '
           'BAM input (%s).')

_bound = False


def _lib():
    global _bound
    lib = ingest._lib()
    if not _bound:
        P, I64, D = ct.c_void_p, ct.c_int64, ct.c_double
        lib.mpn_pileup_records.argtypes = [P, I64, I64, P, P]
        lib.mpn_pileup_records.restype = ct.c_int32
        lib.mpn_pileup_counts.argtypes = [P, I64, I64, P, P, I64, I64, ct.c_int32, P, P, P]
        lib.mpn_pileup_counts.restype = ct.c_int32
        lib.mpn_pileup_candidates.argtypes = [P, I64, I64, P, I64, P, P, D, D, I64, P, P]
        lib.mpn_pileup_candidates.restype = ct.c_int32
        lib.mpn_pileup_last_device_ms.argtypes = [ct.POINTER(D)] * 3
        lib.mpn_pileup_last_device_ms.restype = None
        _bound = True
    return lib


def last_device_ms():
    """-> (records ms, counts ms, candidates ms) of the calling thread's last native calls"""
    return _ffi.device_ms(_lib().mpn_pileup_last_device_ms, 3)


def pileup_records(text, text_len, rows):
    """mpn_pileup_records on rows of ingest.bam_walk -> a PILE_REC array"""
    rows = np.ascontiguousarray(rows, dtype=ingest.BAM_ROW)
    recs = np.zeros(len(rows), dtype=PILE_REC)
    _ffi.check(_lib().mpn_pileup_records(text.data_ptr(), int(text_len), len(rows), _ffi.ptr(rows), _ffi.ptr(recs)), 'mpn_pileup_records')
    return recs


def pileup_counts(text, text_len, takes, span, lo, hi, counts, slice_records=0):
    """mpn_pileup_counts: adds to `counts` ((hi - lo, 7) int32 on the device) -> (bad row or -1, tiles that were split)"""
    takes = np.ascontiguousarray(takes, dtype=PILE_TAKE)
    span = np.ascontiguousarray(span, dtype=np.int64)
    assert counts.is_contiguous() and counts.numel() == (hi - lo) * SLOTS and len(span) == len(takes)
    bad, sliced = ct.c_int64(-1), ct.c_int64(0)
    _ffi.check(_lib().mpn_pileup_counts(text.data_ptr(), int(text_len), len(takes), _ffi.ptr(takes), _ffi.ptr(span), int(lo), int(hi), int(slice_records),
                                    counts.data_ptr(), ct.byref(bad), ct.byref(sliced)), 'mpn_pileup_counts')
    return bad.value, sliced.value


def pileup_candidates(counts, lo, ref_bytes, bed, min_coverage, threshold):
    """mpn_pileup_candidates -> a PILE_CAND array.  ref_bytes: uint8 array, one per position of the window (0: none); bed: None or
    (starts, ends), sorted and disjoint."""
    lib = _lib()
    n_pos = len(ref_bytes)
    assert counts.numel() == n_pos * SLOTS
    ref_bytes = np.ascontiguousarray(ref_bytes, dtype=np.uint8)
    n_bed, bs, be = -1, None, None
    if bed is not None:
        bs, be = np.ascontiguousarray(bed[0], dtype=np.int64), np.ascontiguousarray(bed[1], dtype=np.int64)
        n_bed = len(bs)
    cap, n = 1 << 16, ct.c_int64(0)
    while True:
        rows = np.zeros(cap, dtype=PILE_CAND)
        rc = lib.mpn_pileup_candidates(counts.data_ptr(), int(lo), n_pos, _ffi.ptr(ref_bytes), n_bed, None if n_bed < 1 else bs.ctypes.data,
                                       None if n_bed < 1 else be.ctypes.data, float(min_coverage), float(threshold), cap, rows.ctypes.data, ct.byref(n))
        if rc == -3 and n.value > cap:
            cap = n.value
            continue
        _ffi.check(rc, 'mpn_pileup_candidates')
        return rows[:n.value]


def bam_references(path):
    """-> [(name, length)] from the header of a BAM file (its first bytes, inflated on the host)"""
    with gzip.open(path, 'rb') as f:
        head = f.read(8)
        if len(head) < 8 or head[:4] != b'BAM\1':
            raise ValueError(f'{path}: not a BAM file')
        l_text, = struct.unpack('<i', head[4:])
        f.read(l_text)
        n_ref, = struct.unpack('<i', f.read(4))
        out = []
        for _ in range(n_ref):
            l_name, = struct.unpack('<i', f.read(4))
            name = f.read(l_name)[:-1].decode()
            out.append((name, struct.unpack('<i', f.read(4))[0]))
    return out


def contig_tid(bam, ctg_name):
    """-> (the reference id the records of ctg_name carry in `bam`; -2 if its header has no such contig, which no record has; the
    contig's length by the header, 0 then)"""
    refs = bam_references(bam)
    names = [n for n, _ in refs]
    tid = names.index(ctg_name) if ctg_name in names else -2
    return tid, (refs[tid][1] if tid >= 0 else 0)


def contig_records(t, tid, filter_flag=FILTER_FLAG):
    """t: an ingest.BamText -> (keep, recs): the indices into t.rows of the records that pass the flag filter and lie on the contig
    `tid`, and their PILE_REC.  The records that pass the filter all go through mpn_pileup_records."""
    keep = np.flatnonzero((t.rows['flag'] & filter_flag) == 0)
    recs = pileup_records(t.text, t.text_len, t.rows[keep])
    on = np.flatnonzero(recs['ref_id'] == tid)
    return keep[on], recs.take(on)           # (take: a structured array indexed with [] is copied field by field)


def check_ascending(pos, last_pos, message):
    """pos: the positions of records in file order (int64); last_pos: the position before them, None at the start of the file.
    ValueError(message(i)) for the first record i that lies before its predecessor -> the last position"""
    if not len(pos):
        return last_pos
    down = np.flatnonzero(np.diff(pos, prepend=pos[0] if last_pos is None else last_pos) < 0)
    if len(down):
        raise ValueError(message(int(down[0])))
    return int(pos[-1])


Pileup =collections.namedtuple('Pileup', 'lo hi counts n_taken n_records sliced_tiles')


def _record_name(text, row):
    a = int(row['off']) + 36
    return bytes(text[a:a + int(row['l_read_name']) - 1].cpu().numpy()).decode(errors='replace')


def _window(ctg_start, ctg_end, length):
    if ctg_start is not None and ctg_end is not None:       # the reference takes a range only when both ends are given
        lo = max(int(ctg_start) - 1, 0)
        return lo, max(lo, min(int(ctg_end), length))
    return 0, length


def pileup(bam, ctg_name, ctg_start=None, ctg_end=None, min_mq=0, device='cuda', ctg_len=None, timings=None, slice_records=0):
    """The counters of the records of `bam` (a path; sorted by position) that the reference script takes on ctg_name, inside the
    window: positions ctg_start - 1 .. ctg_end - 1 (both 1-based ends given) or the whole contig -- its length is the larger of the
    BAM header's and ctg_len.  -> Pileup(lo, hi, counts: an (hi - lo, 7) int32 tensor on the device, n_taken, n_records,
    sliced_tiles).  ValueError for taken records that are not sorted by position, that keep their CIGAR in a CG tag, or that are
    malformed (code 0 or no base under M, = or X among them: the reference script raises there)."""
    import torch
    device = device or 'cuda'
    _lib()
    tid, length = contig_tid(bam, ctg_name)
    lo, hi = _window(ctg_start, ctg_end, max(length, int(ctg_len or 0), 0))
    counts = torch.zeros((hi - lo, SLOTS), dtype=torch.int32, device=device)
    n_taken = n_records = sliced_tiles = 0
    last_pos = None
    with ingest.BamTexts(bam, device, timings) as texts:
        for t in texts:
            text, text_len = t.text, t.text_len
            n_records += len(t.rows)
            t1 = time.perf_counter()
            on, recs = contig_records(t, tid)
            ingest._tick(timings, 'records_device_ms', last_device_ms()[0])
            keep = np.flatnonzero((recs['mapq'] >= min_mq) & (recs['n_cigar'] > 0))
            rows, recs = t.rows.take(on[keep]), recs.take(keep)
            bad = np.flatnonzero((recs['status'] != OK) & (recs['status'] != NO_BASE))
            if len(bad):
                b = int(bad[0])
                raise ValueError(f'{bam}: record {_record_name(text, rows[b])}: {STATUS_TEXT[int(recs["status"][b])]}')
            # the reference: skip a read less than 55% aligned -- float(S) / (T + 1) in float64, exactly as written there
            keep = ~(1.0 - recs['soft'].astype(np.float64) / (recs['total'] + 1).astype(np.float64) < 0.55)
            rows, recs = rows[keep], recs[keep]
            bad = np.flatnonzero(recs['status'] == NO_BASE)
            if len(bad):
                raise ValueError(f'{bam}: record {_record_name(text, rows[int(bad[0])])}: {STATUS_TEXT[NO_BASE]}')
            t2 = time.perf_counter()
            ingest._tick(timings, 'records', t2 - t1)
            if len(rows):
                pos = recs['pos'].astype(np.int64)
                lead = np.diff(pos, prepend=pos[0] - 1 if last_pos is None else last_pos) > 0        # the first taken record of its POS
                last_pos = check_ascending(pos, last_pos, lambda i: f'{bam}: record {_record_name(text, rows[i])}: the records that are taken are not '
                                           'sorted by position')
                takes = np.zeros(len(rows), dtype=PILE_TAKE)
                takes['off'], takes['pos'], takes['lead'] = rows['off'], recs['pos'], lead
                bad_row, sliced = pileup_counts(text, text_len, takes, recs['span'], lo, hi, counts, slice_records)
                ingest._tick(timings, 'counts_device_ms', last_device_ms()[1])
                if bad_row >= 0:
                    raise ValueError(f'{bam}: record {_record_name(text, rows[bad_row])}: base code 0 (=) or no base under a matched stretch '
                                     '(the reference script raises there)')
                n_taken += len(rows)
                sliced_tiles += sliced
            ingest._tick(timings, 'counts', time.perf_counter() - t2)
    return Pileup(lo, hi, counts, n_taken, n_records, sliced_tiles)


def read_bed(bed_fn, ctg_name):
    """The intervals of ctg_name in a BED file (plain or gzip), a zero-length one widened to one base as the reference does, merged
    -> (starts, ends), sorted and disjoint.  ValueError if the contig does not occur (the reference exits there)."""
    kind, stream = fastx.open_once(bed_fn)
    iv, seen = [], False
    with stream:
        for line in stream:
            col = line.split()
            if len(col) < 3 or col[0].decode() != ctg_name:
                continue
            seen = True
            s, e = int(col[1]), int(col[2])
            iv.append((s, e + 1 if s == e else e))
    if not seen:
        raise ValueError(f'[ERROR] ctg_name({ctg_name}) not exists in bed file({bed_fn}).')
    merged = []
    for s, e in sorted(x for x in iv if x[1] > x[0]):
        if merged and s <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], e)
        else:
            merged.append([s, e])
    return np.array([m[0] for m in merged], dtype=np.int64), np.array([m[1] for m in merged], dtype=np.int64)


def read_contig(ref_fn, ctg_name):
    """-> the bytes of ctg_name in a FASTA file, plain or gzip, as they stand (case kept).  No .fai is needed."""
    kind, stream = fastx.open_once(ref_fn)
    if kind not in ('plain', 'gzip'):
        raise ValueError(f'{ref_fn}: the reference is a FASTA file, plain or gzip')
    with stream:
        for name, seq, _ in fastx.iter_fastx(stream):
            if name == ctg_name:
                return seq
    return b''


def format_lines(ctg_name, rows):
    """PILE_CAND rows -> the bytes of the reference's lines"""
    out = []
    labels = rows['label'].tobytes().decode()
    bases = rows['ref_base'].tobytes().decode()
    for i, (pos, depth, count) in enumerate(zip(rows['pos'].tolist(), rows['depth'].tolist(), rows['count'].tolist())):
        lab = labels[SLOTS * i:SLOTS * (i + 1)]
        out.append(f'{ctg_name} {pos + 1} {bases[i]} {depth} ' + ' '.join(f'{l} {c}' for l, c in zip(lab, count)) + '\n')
    return ''.join(out).encode()


def extract_variant_candidates(bam_fn, ref_fn, ctg_name, ctg_start=None, ctg_end=None, threshold=0.125, min_coverage=4, min_mq=0, bed_fn=None,
                               out=None, device='cuda', timings=None):
    """Clair's make_candidates (without --gen4Training) on the GPU: writes the reference's lines to `out` (a binary stream;
    default: standard output) -> the number of lines.  If no record is taken, the reference's message goes to standard error and
    nothing is written.  ValueError: min_coverage <= 0 (the reference then also prints lines for positions it has already
    printed), a contig that the BED or the FASTA does not have, and what pileup() refuses."""
    out = sys.stdout.buffer if out is None else out
    if not float(min_coverage) > 0:
        raise ValueError('minCoverage must be above 0: the reference prints phantom lines otherwise, which is not taken')
    t0 = time.perf_counter()
    seq = read_contig(ref_fn, ctg_name)
    if not seq:
        raise ValueError(f'[ERROR] Failed to load reference seqeunce from file ({ref_fn}).')
    bed = read_bed(bed_fn, ctg_name) if bed_fn is not None else None
    ingest._tick(timings, 'reference', time.perf_counter() - t0)
    p = pileup(bam_fn, ctg_name, ctg_start, ctg_end, min_mq, device, ctg_len=len(seq), timings=timings)
    if timings is not None:
        timings['taken'], timings['records_seen'], timings['sliced_tiles'] = p.n_taken, p.n_records, p.sliced_tiles
    if p.n_taken == 0:
        print(NO_READ % bam_fn, file=sys.stderr)
        return 0
    t1 = time.perf_counter()
    ref_bytes = np.zeros(p.hi - p.lo, dtype=np.uint8)
    part = np.frombuffer(seq, dtype=np.uint8)[p.lo:p.hi]
    ref_bytes[:len(part)] = part
    rows = pileup_candidates(p.counts, p.lo, ref_bytes, bed, min_coverage, threshold)
    ingest._tick(timings, 'candidates_device_ms', last_device_ms()[2])
    t2 = time.perf_counter()
    out.write(format_lines(ctg_name, rows))
    ingest._tick(timings, 'candidates', t2 - t1)
    ingest._tick(timings, 'format', time.perf_counter() - t2)
    return len(rows)


def main(argv, prog='mpn-candidates'):
    """The command line of preprocess/ExtractVariantCandidates.py."""
    from argparse import ArgumentParser
    ap = ArgumentParser(prog=prog, description='Generate 1-based variant candidates using alignments (on the GPU)')
    ap.add_argument('--bam_fn', type=str, default='input.bam', help='Sorted bam file input, default: %(default)s')
    ap.add_argument('--ref_fn', type=str, default='ref.fa', help='Reference fasta file input (plain or gzip; no .fai is needed), default: %(default)s')
    ap.add_argument('--bed_fn', type=str, default=None, help='Call variant only in these regions, in intersection with ctgName, ctgStart and ctgEnd')
    ap.add_argument('--can_fn', type=str, default='PIPE', help='Pile-up count output, PIPE for standard output, any other value: a gzip file')
    ap.add_argument('--threshold', type=float, default=0.125, help='Minimum allele frequency of the 1st non-reference allele, default: %(default)f')
    ap.add_argument('--minCoverage', type=float, default=4, help='Minimum coverage required to call a variant, default: %(default)f')
    ap.add_argument('--minMQ', type=int, default=0, help='Minimum mapping quality, default: %(default)d')
    ap.add_argument('--ctgName', type=str, default='chr17', help='The name of sequence to be processed, default: %(default)s')
    ap.add_argument('--ctgStart', type=int, default=None, help='The 1-based starting position of the sequence to be processed')
    ap.add_argument('--ctgEnd', type=int, default=None, help='The 1-based inclusive ending position of the sequence to be processed')
    ap.add_argument('--samtools', type=str, default='samtools', help='accepted and ignored: no samtools is run')
    ap.add_argument('--gen4Training', action='store_true', help='refused: training only')
    ap.add_argument('--var_fn', type=str, default=None, help='refused: training only')
    ap.add_argument('--outputProb', type=float, default=None, help='refused: training only')
    if not argv:
        ap.print_help()
        return 1
    a = ap.parse_args(argv)
    if a.gen4Training or a.var_fn is not None or a.outputProb is not None:
        print(f'{prog}: --gen4Training, --var_fn and --outputProb build training sets and draw random numbers: not taken', file=sys.stderr)
        return 2
    buf = io.BytesIO()
    try:
        extract_variant_candidates(a.bam_fn, a.ref_fn, a.ctgName, a.ctgStart, a.ctgEnd, a.threshold, a.minCoverage, a.minMQ, a.bed_fn, out=buf)
    except (ValueError, OSError) as e:
        print(f'{prog}: {e}', file=sys.stderr)
        return 1
    if a.can_fn == 'PIPE':
        sys.stdout.buffer.write(buf.getvalue())
        sys.stdout.buffer.flush()
    else:
        with open(a.can_fn, 'wb') as f, gzip.GzipFile(fileobj=f, mode='wb', filename='', mtime=0) as z:
            z.write(buf.getvalue())
    return 0
