"""Clair's input tensors on the GPU: a drop-in for preprocess/CreateTensor.py (OutputAlnTensor / generate_tensor), the consumer of
the candidate sites of candidates.py.  One 33 x 8 x 4 integer tensor per candidate site and sample of at most 100 reads; the output
is the reference's byte for byte for a given state of Python's `random`.  The rules, the quirks that are reproduced and the
differences are DESIGN.md section 6; the native calls are include/mpn_tensor.h.

    tensors(bam_fn, ref_fn, can, ctg_name, ...)       -> (centres, an (n, 33, 8, 4) int32 tensor on the device, reference strings)
    create_tensor(bam_fn, ref_fn, can, ctg_name, ..)  -> writes the reference's lines
    bin/mpn-create-tensor                             the command line of the reference script

The BAM goes to HBM group by group (MPN_INGEST_BATCH_BYTES) through ingest.BamTexts, each text beginning at the first record that an
unfinished centre still needs (keep_from); no samtools, .bai or .fai is used.
The host decides what is taken (flags, contig, htslib's overlap with the region, MAPQ, the dcov run), bisects a range of records
for every centre, builds the Python set of a deep centre and draws from `rng` in the reference's order; the join, the centre flags,
the tensors and the text of the lines are made on the device."""
import gzip
import io
import random
import sys
import time
import ctypes as ct

import numpy as np

from . import _ffi, candidates, ingest
from ._ffi import check as _check, ptr as _p

FLANK = 16
POSITIONS, ROWS, CHANNELS, CELLS = 33, 8, 4, 1056
DEPTH = 100                  # matrix_depth
MAX_ITER = 100               # max_iter
EXPAND = 100000              # param.expandReferenceRegion
TENSOR_REC = np.dtype([('hts_len', '<i8'), ('l_seq', '<i4'), ('has_qual', 'u1'), ('status', 'u1'), ('reserved', '<u2')])     # mpn_tensor_rec
TENSOR_READ = np.dtype([('off', '<i8'), ('pos', '<i4'), ('reverse', '<i4')])                                              # mpn_tensor_read
TENSOR_JOB = np.dtype([('begin', '<i8'), ('c0', '<i4'), ('n', '<i4'), ('via_sel', '<i4'), ('reserved', '<i4')])             # mpn_tensor_job
TENSOR_LINE = np.dtype([('tensor', '<i8'), ('ref_off', '<i8'), ('ref_n', '<i4'), ('centre', '<i4')])                       # mpn_tensor_line

_bound = False


def _lib():
    global _bound
    lib = candidates._lib()
    if not _bound:
        P, I64, I32 = ct.c_void_p, ct.c_int64, ct.c_int32
        lib.mpn_tensor_records.argtypes = [P, I64, I64, P, P]
        lib.mpn_tensor_join.argtypes = [I64, P, P, I64, P, P, P, I32, P, P, P, I64]
        lib.mpn_tensor_centre_flags.argtypes = [P, I64, I64, P, P, I64, I64, P, P, I32, P, P]
        lib.mpn_tensor_fill.argtypes = [P, I64, I64, P, P, I64, I64, P, I64, P, I32, P, I64, I64, P, P, P]
        lib.mpn_tensor_emit.argtypes = [P, I64, I64, P, P, I64, ct.c_char_p, I32, P, P, P, I64]
        for f in (lib.mpn_tensor_records, lib.mpn_tensor_join, lib.mpn_tensor_centre_flags, lib.mpn_tensor_fill, lib.mpn_tensor_emit):
            f.restype = I32
        lib.mpn_tensor_last_device_ms.argtypes = [ct.POINTER(ct.c_double)] * 4
        lib.mpn_tensor_last_device_ms.restype = None
        _bound = True
    return lib


def last_device_ms():
    """-> (join ms, flags ms, fill ms, emit ms) of the calling thread's last native calls"""
    return _ffi.device_ms(_lib().mpn_tensor_last_device_ms, 4)


# ---- the native calls ---------------------------------------------------------------------------------------------------------------
def tensor_records(text, text_len, rows):
    """mpn_tensor_records on rows of ingest.bam_walk -> a TENSOR_REC array"""
    rows = np.ascontiguousarray(rows, dtype=ingest.BAM_ROW)
    recs = np.zeros(len(rows), dtype=TENSOR_REC)
    _check(_lib().mpn_tensor_records(text.data_ptr(), int(text_len), len(rows), _p(rows), _p(recs)), 'mpn_tensor_records')
    return recs


def join_ranges(pos, span, c0, left_edge=True):
    """The range of records [begin, end) that mpn_tensor_join looks at for every centre: from the first whose running maximum of
    pos + span passes c0 - 16 to the last whose pos is at most c0 + 17 (c0 - 16 without left edges)."""
    pos, span, c0 = np.asarray(pos, dtype=np.int64), np.asarray(span, dtype=np.int64), np.asarray(c0, dtype=np.int64)
    reach = np.maximum.accumulate(pos + span) if len(pos) else pos
    begin = np.searchsorted(reach, c0 - FLANK, side='right')
    end = np.searchsorted(pos, c0 + FLANK + 1 if left_edge else c0 - FLANK, side='right')
    return begin.astype(np.int64), np.maximum(end, begin).astype(np.int64)


def tensor_join(pos, span, c0, begin, end, left_edge=True, device='cuda'):
    """mpn_tensor_join, twice: count, then scatter -> (counts, pair offsets [m + 1], the pair list: an int32 tensor on the device,
    the device time in ms)"""
    import torch
    lib = _lib()
    pos, span = np.ascontiguousarray(pos, dtype=np.int32), np.ascontiguousarray(span, dtype=np.int64)
    c0, begin, end = np.ascontiguousarray(c0, dtype=np.int32), np.ascontiguousarray(begin, dtype=np.int64), np.ascontiguousarray(end, dtype=np.int64)
    assert len(pos) == len(span) and len(c0) == len(begin) == len(end)
    counts = np.zeros(len(c0), dtype=np.int64)
    _check(lib.mpn_tensor_join(len(pos), _p(pos), _p(span), len(c0), _p(c0), _p(begin), _p(end), int(bool(left_edge)), _p(counts), None, None, 0),
           'mpn_tensor_join')
    ms = last_device_ms()[0]
    off = np.zeros(len(c0) + 1, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    total = int(off[-1])
    pairs = torch.empty(max(total, 1), dtype=torch.int32, device=device)
    if total:
        again, first = np.zeros(len(c0), dtype=np.int64), np.ascontiguousarray(off[:-1])
        _check(lib.mpn_tensor_join(len(pos), _p(pos), _p(span), len(c0), _p(c0), _p(begin), _p(end), int(bool(left_edge)), _p(again), _p(first),
                                   pairs.data_ptr(), total), 'mpn_tensor_join')
        assert np.array_equal(again, counts)
        ms += last_device_ms()[0]
    return counts, off, pairs[:total], ms


def _reads(reads):
    return np.ascontiguousarray(reads, dtype=TENSOR_READ)


def centre_flags(text, text_len, reads, pairs, pair, c0, left_edge=True):
    """mpn_tensor_centre_flags -> (a uint8 array, one per entry of `pair`; bad read or -1)"""
    reads, pair, c0 = _reads(reads), np.ascontiguousarray(pair, dtype=np.int64), np.ascontiguousarray(c0, dtype=np.int32)
    assert len(pair) == len(c0)
    flags, bad = np.zeros(len(pair), dtype=np.uint8), ct.c_int64(-1)
    _check(_lib().mpn_tensor_centre_flags(text.data_ptr(), int(text_len), len(reads), _p(reads), pairs.data_ptr(), pairs.numel(), len(pair), _p(pair), _p(c0),
                                          int(bool(left_edge)), _p(flags), ct.byref(bad)), 'mpn_tensor_centre_flags')
    return flags, bad.value


def tensor_fill(text, text_len, reads, pairs, sel, jobs, d_ref, ref_start, left_edge=True):
    """mpn_tensor_fill -> (an (n_jobs, 1056) int32 tensor on the device, depth at the centre per job, bad read or -1)"""
    import torch
    reads, jobs = _reads(reads), np.ascontiguousarray(jobs, dtype=TENSOR_JOB)
    sel = np.ascontiguousarray(sel if sel is not None else [], dtype=np.int64)
    out = torch.empty((max(len(jobs), 1), CELLS), dtype=torch.int32, device=text.device)
    depth, bad = np.zeros(len(jobs), dtype=np.int32), ct.c_int64(-1)
    _check(_lib().mpn_tensor_fill(text.data_ptr(), int(text_len), len(reads), _p(reads), pairs.data_ptr(), pairs.numel(), len(sel), _p(sel), len(jobs),
                                  _p(jobs), int(bool(left_edge)), d_ref.data_ptr() if d_ref.numel() else None, int(ref_start), d_ref.numel(),
                                  out.data_ptr(), _p(depth), ct.byref(bad)), 'mpn_tensor_fill')
    return out[:len(jobs)], depth, bad.value


def tensor_emit(block, lines, d_ref, ctg_name, out, timings=None):
    """mpn_tensor_emit: the lines (a TENSOR_LINE array over the rows of `block`) as text, written to `out` in rounds of at most
    MPN_INGEST_BATCH_BYTES -> the bytes written"""
    import torch
    lib = _lib()
    lines = np.ascontiguousarray(lines, dtype=TENSOR_LINE)
    if not len(lines):
        return 0
    name = ctg_name.encode()
    ref_ptr = d_ref.data_ptr() if d_ref.numel() else None
    length = np.zeros(len(lines), dtype=np.int64)
    _check(lib.mpn_tensor_emit(block.data_ptr(), block.shape[0], len(lines), _p(lines), ref_ptr, d_ref.numel(), name, len(name), _p(length), None, None, 0),
           'mpn_tensor_emit')
    ingest._tick(timings, 'emit_device_ms', last_device_ms()[3])
    limit, a, written = max(1, ingest.batch_bytes()), 0, 0
    ends = np.cumsum(length)
    while a < len(lines):
        base = int(ends[a - 1]) if a else 0
        b = max(a + 1, int(np.searchsorted(ends, base + limit, side='right')))
        total = int(ends[b - 1]) - base
        off = np.ascontiguousarray(ends[a:b] - length[a:b] - base)
        text = torch.empty(total, dtype=torch.uint8, device=block.device)
        part_len, part = np.ascontiguousarray(length[a:b]), np.ascontiguousarray(lines[a:b])
        _check(lib.mpn_tensor_emit(block.data_ptr(), block.shape[0], b - a, _p(part), ref_ptr, d_ref.numel(), name, len(name), _p(part_len),
                                   _p(off), text.data_ptr(), total), 'mpn_tensor_emit')
        ingest._tick(timings, 'emit_device_ms', last_device_ms()[3])
        t0 = time.perf_counter()
        out.write(text.cpu().numpy().tobytes())
        ingest._tick(timings, 'download', time.perf_counter() - t0)
        written += total
        a = b
    return written


# ---- the host's part ----------------------------------------------------------------------------------------------------------------
def read_positions(can, ctg_start=None, ctg_end=None):
    """can: a path to a gzip (or plain) file, a text stream, or an integer array of 1-based positions -> the 0-based centres inside
    the region, ascending and without duplicates.  ValueError for positions that are not ascending."""
    if isinstance(can, (str, bytes)) and not isinstance(can, np.ndarray):
        with open(can, 'rb') as f:
            head = f.read(2)
        with (gzip.open(can, 'rb') if head == b'\x1f\x8b' else open(can, 'rb')) as f:
            pos = [int(line.split()[1]) for line in f if line.strip()]
    elif hasattr(can, 'read') or hasattr(can, 'readline'):
        pos = [int(line.split()[1]) for line in can if line.strip()]
    else:
        pos = can
    pos = np.asarray(pos, dtype=np.int64).reshape(-1)
    if ctg_start is not None and ctg_end is not None:
        pos = pos[(pos >= ctg_start) & (pos <= ctg_end)]
    if len(pos) > 1 and bool((pos[1:] < pos[:-1]).any()):
        raise ValueError('the candidate positions are not in ascending order')
    if len(pos) and (int(pos[0]) < 1 or int(pos[-1]) > 0x7ffffff0):
        raise ValueError('a candidate position is not a 1-based position')
    return np.unique(pos) - 1


def dcov_run(pos, dcov, state):
    """The script's previous_position / depthCap run over the records it walks (pos: their 0-based positions, in file order).
    state: (previous_position, depthCap), (0, 0) before the first record -- so a first record at position 0 already counts as a
    repeat.  -> (which are taken, the state behind them)"""
    pos = np.asarray(pos, dtype=np.int64)
    if not len(pos):
        return np.zeros(0, dtype=bool), state
    previous, cap = state
    new = pos != np.concatenate([[previous], pos[:-1]])
    idx = np.arange(len(pos))
    start = np.maximum.accumulate(np.where(new, idx, -1))
    rank = np.where(start >= 0, idx - start, cap + 1 + idx)
    return new | (rank < dcov), (int(pos[-1]), int(rank[-1]))


def sample_plan(d, rng):
    """The script's iterations for a centre of d reads: one draw of rng.sample(range(d), d) -> None (one tensor of all d reads, in
    order) or the lists of indices, one per tensor."""
    perm = rng.sample(range(d), d)
    iterations = min(MAX_ITER, (d + DEPTH - 1) // DEPTH)
    if iterations == 1:
        return None
    return [perm[k * DEPTH:(k + 1) * DEPTH] for k in range(iterations - 1)] + [perm[-DEPTH:]]


def reference_window(seq, ctg_start=None, ctg_end=None):
    """-> (the bytes the script loads, their 0-based start)"""
    if ctg_start is not None and ctg_end is not None:
        lo = max(int(ctg_start) - EXPAND, 1)
        return seq[lo - 1:int(ctg_end) + EXPAND], lo - 1
    return seq, 0


def contig_reads(t, tid, last_pos, unsorted, filter_flag=candidates.FILTER_FLAG):
    """What the stages that pile up columns (clair_call, local_realign) take of the text t (an ingest.BamText): every record of the
    contig `tid` that passes the flag filter -> (keep: their indices into t.rows, pos, rlen: htslib's length on the reference, the
    last position).  ValueError(unsorted) if they do not ascend from last_pos on."""
    keep, recs = candidates.contig_records(t, tid, filter_flag)
    trecs = tensor_records(t.text, t.text_len, t.rows[keep])
    pos = recs['pos'].astype(np.int64)
    return keep, pos, trecs['hts_len'].astype(np.int64), candidates.check_ascending(pos, last_pos, lambda i: unsorted)


def _run(bam_fn, ref_fn, can, ctg_name, ctg_start, ctg_end, min_mq, dcov, min_coverage, left_edge, rng, device, timings, sink):
    """The whole stage.  sink(block, centres, ref_off, ref_n, d_ref, window) per text with tensors to give: block is a
    (k, 1056) int32 tensor on the device, centres (1-based), ref_off and ref_n numpy arrays of k entries."""
    import torch
    device = device or 'cuda'
    _lib()
    t0 = time.perf_counter()
    seq = candidates.read_contig(ref_fn, ctg_name)
    if not seq:
        raise ValueError(f'Failed to load reference seqeunce. Please check if the provided reference fasta {ref_fn} and the ctgName {ctg_name} are correct.')
    region = ctg_start is not None and ctg_end is not None
    window, ref_start = reference_window(seq, ctg_start, ctg_end)
    ref_end = ref_start + len(window)
    d_ref = torch.from_numpy(np.frombuffer(window, dtype=np.uint8).copy()).to(device)
    centres = read_positions(can, ctg_start, ctg_end)
    ingest._tick(timings, 'reference', time.perf_counter() - t0)
    tid, _ = candidates.contig_tid(bam_fn, ctg_name)
    next_centre, kept_take, state, last_pos = 0, np.zeros(0, dtype=bool), (0, 0), None
    resident = dict() if timings is not None else None
    with ingest.BamTexts(bam_fn, device, resident) as texts:
        while True:
            t0 = time.perf_counter()
            t = next(texts)
            text, text_len, rows, final = t.text, t.text_len, t.rows, t.final
            n_old = len(kept_take)
            if len(rows) < n_old:
                raise ValueError(f'{bam_fn}: the records of a text were not found again in the next')
            # ---- what is taken: the records of the contig that pass the flag get their facts; the new ones their decision
            keep_f, recs = candidates.contig_records(t, tid)
            rows_f = rows[keep_f]
            trecs = tensor_records(text, text_len, rows_f)
            t1 = time.perf_counter()
            ingest._tick(timings, 'resident', t1 - t0)
            walked = recs['mapq'] >= min_mq
            if region:
                pos64 = recs['pos'].astype(np.int64)
                walked &= (pos64 < int(ctg_end)) & (pos64 + np.maximum(trecs['hts_len'], 1) > int(ctg_start) - 1)
            new = keep_f >= n_old
            for bad in np.flatnonzero(walked & new & ((recs['status'] == candidates.PLACEHOLDER) | (recs['status'] == candidates.CIGAR_PAST) |
                                                      (recs['status'] == candidates.BAD_OP) | (trecs['status'] == candidates.CIGAR_PAST)))[:1]:
                status = int(recs['status'][bad]) or int(trecs['status'][bad])
                raise ValueError(f'{bam_fn}: record {candidates._record_name(text, rows_f[bad])}: {candidates.STATUS_TEXT[status]}')
            wn = np.flatnonzero(walked & new)
            p = recs['pos'][wn].astype(np.int64)
            last_pos = candidates.check_ascending(p, last_pos, lambda i: f'{bam_fn}: record {candidates._record_name(text, rows_f[wn[i]])}: the records '
                                                  'that are taken are not sorted by position')
            took, state = dcov_run(p, dcov, state)
            take_all = np.zeros(len(rows), dtype=bool)
            take_all[:n_old] = kept_take
            take_all[keep_f[wn]] = took
            ti = np.flatnonzero(take_all[keep_f])              # the taken records, as indices into rows_f
            pos, span = recs['pos'][ti].astype(np.int64), recs['span'][ti].astype(np.int64)
            # ---- the centres that no later record can join
            todo = centres[next_centre:]
            n_fin = len(todo) if final else (int(np.searchsorted(todo, int(pos[-1]) - (FLANK + 1), side='left')) if len(ti) else 0)
            fin = todo[:n_fin]
            if n_fin and len(ti):
                _batch(text, text_len, rows_f[ti], recs[ti], trecs[ti], pos, span, fin, left_edge, min_coverage, rng, d_ref, window, ref_start, ref_end,
                       bam_fn, device, timings, sink)
            next_centre += n_fin
            if final:
                break
            # ---- the next text starts at the first record that an unfinished centre still needs
            cut = len(rows)
            if next_centre < len(centres) and len(ti):
                b = int(join_ranges(pos, span, centres[next_centre:next_centre + 1], left_edge)[0][0])
                if b < len(ti):
                    cut = int(keep_f[ti[b]])
            kept_take = take_all[cut:].copy()
            texts.keep_from(cut)
    if timings is not None:
        for key in ('read', 'h2d', 'inflate', 'flatten'):
            timings[key] = resident.get(key, 0)


def _batch(text, text_len, rows, recs, trecs, pos, span, fin, left_edge, min_coverage, rng, d_ref, window, ref_start, ref_end, bam_fn, device, timings, sink):
    """The finished centres `fin` (0-based, ascending) of one text over its taken records."""
    t0 = time.perf_counter()
    begin, end = join_ranges(pos, span, fin, left_edge)
    counts, off, pairs, ms = tensor_join(pos, span, fin, begin, end, left_edge, device)
    ingest._tick(timings, 'join_device_ms', ms)
    # what the reference answers with an IndexError: a read that a centre keeps open and that has no bases, no qualities, or
    # reaches past the end of the reference sequence
    last = np.searchsorted(fin, pos + span + FLANK, side='left') - 1            # the last centre with c0 - 16 < pos + span
    c_last = fin[np.maximum(last, 0)]
    joined = (span > 0) & (last >= 0) & ((c_last + FLANK + 1 >= pos) if left_edge else (c_last - FLANK >= pos))
    bad = np.flatnonzero(joined & ((trecs['l_seq'] == 0) | (trecs['has_qual'] == 0)))
    if len(bad):
        raise ValueError(f'{bam_fn}: record {candidates._record_name(text, rows[int(bad[0])])}: a read without bases or without qualities lies '
                         'in the window of a candidate (the reference script raises there)')
    bad = np.flatnonzero(joined & (np.minimum(pos + span, c_last + FLANK + 3) > ref_end))
    if len(bad):
        raise ValueError(f'{bam_fn}: record {candidates._record_name(text, rows[int(bad[0])])}: the read reaches past the end of the reference '
                         'sequence inside the window of a candidate (the reference script raises there)')
    reads = np.zeros(len(rows), dtype=TENSOR_READ)
    reads['off'], reads['pos'], reads['reverse'] = rows['off'], recs['pos'], (rows['flag'] & 16) != 0
    t1 = time.perf_counter()
    ingest._tick(timings, 'join', t1 - t0)
    # ---- deep centres: which of their reads have a high-quality base at the centre
    deep = np.flatnonzero(counts > DEPTH)
    high = {}
    if len(deep):
        pair = np.concatenate([np.arange(off[c], off[c + 1]) for c in deep])
        flags, bad_read = centre_flags(text, text_len, reads, pairs, pair, np.repeat(fin[deep], counts[deep]), left_edge)
        ingest._tick(timings, 'flags_device_ms', last_device_ms()[1])
        if bad_read >= 0:
            raise ValueError(f'{bam_fn}: record {candidates._record_name(text, rows[bad_read])}: {candidates.STATUS_TEXT[candidates.NO_BASE]}')
        at = 0
        for c in deep.tolist():
            high[c] = np.flatnonzero(flags[at:at + int(counts[c])]).tolist()
            at += int(counts[c])
    t2 = time.perf_counter()
    ingest._tick(timings, 'flags', t2 - t1)
    # ---- the draws, in ascending centre order, and the tensors they ask for
    jobs, sel, owner = [], [], []
    flank_ok = (fin + 1 - ref_start - (FLANK + 1)) >= 0
    for c in np.flatnonzero(counts > 0).tolist():
        d, chosen = int(counts[c]), None
        if c in high:
            s = set()
            for i in high[c]:
                s.add(i)
            if len(s) > DEPTH:
                chosen = list(s)             # in the order of the set, as the script takes them
                d = len(chosen)
        plan = sample_plan(d, rng)
        if not flank_ok[c]:
            continue
        base = int(off[c])
        if plan is None:
            jobs.append((base, int(fin[c]), d, 0, 0))
            owner.append(c)
            continue
        for part in plan:
            jobs.append((len(sel), int(fin[c]), len(part), 1, 0))
            owner.append(c)
            sel += [base + (chosen[i] if chosen is not None else i) for i in part]
    t3 = time.perf_counter()
    ingest._tick(timings, 'sampling', t3 - t2)
    if not jobs:
        return
    jobs = np.array(jobs, dtype=TENSOR_JOB)
    block, depth, bad_read = tensor_fill(text, text_len, reads, pairs, sel, jobs, d_ref, ref_start, left_edge)
    ingest._tick(timings, 'fill_device_ms', last_device_ms()[2])
    if bad_read >= 0:
        raise ValueError(f'{bam_fn}: record {candidates._record_name(text, rows[bad_read])}: no base under a matched stretch or an insertion, or '
                         'no reference byte, inside the window of a candidate (the reference script raises there)')
    # ---- a centre stops at its first tensor below the minimum coverage
    owner = np.array(owner, dtype=np.int64)
    keep = depth >= min_coverage
    again = np.flatnonzero(owner[1:] == owner[:-1]) + 1
    for j in again.tolist():
        keep[j] &= keep[j - 1]
    kept = np.flatnonzero(keep)
    ingest._tick(timings, 'fill', time.perf_counter() - t3)
    if not len(kept):
        return
    if len(kept) < len(jobs):
        block = block.index_select(0, torch_index(kept, block.device))
    c1 = jobs['c0'][kept].astype(np.int64) + 1
    ref_off = c1 - ref_start - (FLANK + 1)
    ref_n = np.clip(len(window) - ref_off, 0, POSITIONS)
    ingest._tick(timings, 'tensors', len(kept))
    sink(block, c1, ref_off, ref_n, d_ref, window)


def torch_index(idx, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(device)


def tensors(bam_fn, ref_fn, can, ctg_name, ctg_start=None, ctg_end=None, min_mq=10, dcov=1000, min_coverage=0, consider_left_edge=True, rng=random,
            device='cuda', timings=None):
    """Clair's tensors of the candidate positions `can` (a path to a gzip file, a text stream, or an integer array of 1-based
    positions) -> (the 1-based centre of every tensor in emission order, an (n, 33, 8, 4) int32 tensor on the device, the reference
    string of every line).  rng: anything with random.Random's sample; it is asked once per centre that a read joined, in ascending
    order.  ValueError for what DESIGN.md section 6 lists: candidate positions that are not ascending, taken records that are not
    sorted, a CIGAR in a CG tag, a contig the FASTA does not have, a read in a candidate's window without bases or qualities or
    past the end of the reference sequence."""
    import torch
    blocks, cs, strings = [], [], []

    def sink(block, c1, ref_off, ref_n, d_ref, window):
        blocks.append(block)
        cs.extend(c1.tolist())
        strings.extend(window[a:a + n].decode() for a, n in zip(ref_off.tolist(), ref_n.tolist()))
    _run(bam_fn, ref_fn, can, ctg_name, ctg_start, ctg_end, min_mq, dcov, min_coverage, consider_left_edge, rng, device, timings, sink)
    out = torch.cat(blocks) if blocks else torch.zeros((0, CELLS), dtype=torch.int32, device=device or 'cuda')
    return cs, out.reshape(-1, POSITIONS, ROWS, CHANNELS), strings


def create_tensor(bam_fn, ref_fn, can, ctg_name, ctg_start=None, ctg_end=None, min_mq=10, dcov=1000, min_coverage=0, consider_left_edge=True, rng=random,
                  out=None, device='cuda', timings=None):
    """Clair's OutputAlnTensor on the GPU: writes `ctg centre refseq t0 .. t1055\\n` per tensor to `out` (a binary stream; default:
    standard output) -> the number of lines.  The text of the lines is made on the device.  Arguments and refusals as tensors()."""
    out = sys.stdout.buffer if out is None else out
    n = [0]

    def sink(block, c1, ref_off, ref_n, d_ref, window):
        lines = np.zeros(len(c1), dtype=TENSOR_LINE)
        lines['tensor'], lines['ref_off'], lines['ref_n'], lines['centre'] = np.arange(len(c1)), ref_off, ref_n, c1
        t0 = time.perf_counter()
        tensor_emit(block, lines, d_ref, ctg_name, out, timings)
        ingest._tick(timings, 'emit', time.perf_counter() - t0)
        n[0] += len(c1)
    _run(bam_fn, ref_fn, can, ctg_name, ctg_start, ctg_end, min_mq, dcov, min_coverage, consider_left_edge, rng, device, timings, sink)
    return n[0]


def main(argv, prog='mpn-create-tensor'):
    """The command line of preprocess/CreateTensor.py."""
    from argparse import ArgumentParser
    ap = ArgumentParser(prog=prog, description='Generate tensors summarizing local alignments from a BAM file and a list of candidate locations (on the GPU)')
    ap.add_argument('--bam_fn', type=str, default='input.bam', help='Sorted bam file input, default: %(default)s')
    ap.add_argument('--ref_fn', type=str, default='ref.fa', help='Reference fasta file input (plain or gzip; no .fai is needed), default: %(default)s')
    ap.add_argument('--can_fn', type=str, default='PIPE', help='Variant candidate list of mpn-candidates, PIPE for standard input, default: %(default)s')
    ap.add_argument('--tensor_fn', type=str, default='PIPE', help='Tensor output, PIPE for standard output, any other value: a gzip file')
    ap.add_argument('--minMQ', type=int, default=10, help='Minimum mapping quality, default: %(default)d')
    ap.add_argument('--ctgName', type=str, default='chr17', help='The name of sequence to be processed, default: %(default)s')
    ap.add_argument('--ctgStart', type=int, default=None, help='The 1-based starting position of the sequence to be processed')
    ap.add_argument('--ctgEnd', type=int, default=None, help='The 1-based inclusive ending position of the sequence to be processed')
    ap.add_argument('--samtools', type=str, default='samtools', help='accepted and ignored: no samtools is run')
    ap.add_argument('--stop_consider_left_edge', action='store_true', help='a read joins a window only if it covers the window\'s first position')
    ap.add_argument('--dcov', type=int, default=1000, help='Cap depth per position at %(default)d')
    ap.add_argument('--minCoverage', type=int, default=0, help='Minimum coverage required to generate a tensor, default: %(default)d')
    if not argv:
        ap.print_help()
        return 1
    a = ap.parse_args(argv)
    buf = io.BytesIO()
    try:
        create_tensor(a.bam_fn, a.ref_fn, sys.stdin if a.can_fn == 'PIPE' else a.can_fn, a.ctgName, a.ctgStart, a.ctgEnd, a.minMQ, a.dcov, a.minCoverage,
                      not a.stop_consider_left_edge, out=buf)
    except (ValueError, OSError) as e:
        print(f'{prog}: {e}', file=sys.stderr)
        return 1
    if a.tensor_fn == 'PIPE':
        sys.stdout.buffer.write(buf.getvalue())
        sys.stdout.buffer.flush()
    else:
        with open(a.tensor_fn, 'wb') as f, gzip.GzipFile(fileobj=f, mode='wb', filename='', mtime=0) as z:
            z.write(buf.getvalue())
    return 0
