"""Clair's lines averaged per site on the GPU, the overlap filter of its VCF, and the chain of bin/runClair-ensemble.sh for one contig:
drop-ins for clair/post_processing/ensemble.py (`clair.py ensemble`, STEP 2) and clair/post_processing/overlap_variant.py (STEP 4).
The rules and the quirks that are reproduced are DESIGN.md section 6 item 21; the native call is include/mpn_ensemble.h.

    group(keys, minimum_count)                                  the host's grouping: a CSR of the sites in order of first appearance
    ensemble_rows(tensor_row, prob_row, tensors, probs, ..)     mpn_clair_ensemble over resident blocks
    ensemble(centres, tensors, probs_list, ..)                  one tensor block and K probability blocks (or K pairs) -> one row per site
    ensemble_lines(stream, out, minimum_count_to_output)        the lines of --output_for_ensemble -> the lines of ensemble.py
    overlap_filter(lines)                                       the rows of overlap_variant.py
    call_ensemble(bam_fn, ref_fn, chkpnt_fns, ctg_name, ..)     BAM -> snp_and_indel.vcf.gz and snp_and_indel.filtered.vcf.gz
    bin/mpn-ensemble, bin/mpn-overlap-variant, bin/mpn-clair-ensemble

The device sums the 1056 integers of a site's lines (int64, refused outside int32), adds the 90 probabilities in input order in
float64, divides by the count and rounds as `{:.6f}` rounds.  The grouping stays on the host, because the keys are strings; so does
the overlap filter, a serial chain over formatted text."""
import io
import os
import sys
import time
import ctypes as ct

import numpy as np

from . import candidates, clair_call, clair_tensor, ingest
from ._ffi import check as _check, ptr as _p

CELLS, PROBS = 1056, 90
COLUMNS = 3 + CELLS + PROBS
LIMIT = 1.0e6            # the text tool refuses a probability that is not finite or not below this (the kernel's rounding holds below 2^31)
_bound = False


def _lib():
    global _bound
    lib = candidates._lib()
    if not _bound:
        P, I64, I32 = ct.c_void_p, ct.c_int64, ct.c_int32
        lib.mpn_clair_ensemble.argtypes = [I64, P, P, P, I64, P, I64, I32, I64, P, P, P, I64, P, P, P, P]
        lib.mpn_clair_ensemble.restype = I32
        lib.mpn_clair_ensemble_last_device_ms.argtypes = [ct.POINTER(ct.c_double)]
        lib.mpn_clair_ensemble_last_device_ms.restype = None
        _bound = True
    return lib


def last_device_ms():
    """the device time of the calling thread's last mpn_clair_ensemble, in milliseconds"""
    v = ct.c_double(0)
    _lib().mpn_clair_ensemble_last_device_ms(ct.byref(v))
    return v.value


# ---- the grouping -------------------------------------------------------------------------------------------------------------------
def group(keys, minimum_count=0):
    """keys: one hashable per line (the script's (chrom, pos) pair of strings), or an integer array -> (site_off [S + 1] int64,
    site_lines int32: the lines of every site in input order, out_slot [S] int32: the running number of the sites with at least
    minimum_count lines and -1 for the others, n_out).  The sites are in the order of first appearance."""
    if isinstance(keys, np.ndarray):
        _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
        rank = np.empty(len(first), dtype=np.int64)
        rank[np.argsort(first, kind='stable')] = np.arange(len(first))
        site = rank[inverse.reshape(-1)]
    else:
        seen = {}
        site = np.fromiter((seen.setdefault(k, len(seen)) for k in keys), dtype=np.int64)
    n_sites = int(site.max()) + 1 if len(site) else 0
    counts = np.bincount(site, minlength=n_sites).astype(np.int64)
    site_off = np.zeros(n_sites + 1, dtype=np.int64)
    np.cumsum(counts, out=site_off[1:])
    site_lines = np.argsort(site, kind='stable').astype(np.int32)
    kept = counts >= int(minimum_count)
    out_slot = np.where(kept, np.cumsum(kept) - 1, -1).astype(np.int32)
    return site_off, site_lines, out_slot, int(kept.sum())


# ---- the native call ------------------------------------------------------------------------------------------------------------------
def ensemble_rows(tensor_row, prob_row, tensors, probs, site_off, site_lines, out_slot, n_out, micro=False):
    """mpn_clair_ensemble.  tensors: a contiguous int32 tensor of n_t * 1056 on the device; probs: a contiguous (n_p, 90) float32 or
    float64 tensor there -> ((n_out, 1056) int32 and (n_out, 90) float32 tensors on the device, an (n_out, 90) int64 tensor of
    micro-units or None, the smallest site whose sum leaves int32 or -1).  ValueError for lists the native layer refuses."""
    import torch
    lib = _lib()
    if not isinstance(tensors, torch.Tensor) or tensors.dtype != torch.int32 or not tensors.is_cuda or not tensors.is_contiguous() or tensors.numel() % CELLS:
        raise ValueError('the tensors are not a contiguous int32 block of 1056 per row on the device')
    if not isinstance(probs, torch.Tensor) or probs.dtype not in (torch.float32, torch.float64) or not probs.is_cuda or not probs.is_contiguous() or \
            probs.dim() != 2 or probs.shape[1] != PROBS or probs.device != tensors.device:
        raise ValueError('the probabilities are not a contiguous (n, 90) float32 or float64 block on the device of the tensors')
    tensor_row, prob_row = np.ascontiguousarray(tensor_row, dtype=np.int32), np.ascontiguousarray(prob_row, dtype=np.int32)
    site_off, site_lines = np.ascontiguousarray(site_off, dtype=np.int64), np.ascontiguousarray(site_lines, dtype=np.int32)
    out_slot = np.ascontiguousarray(out_slot, dtype=np.int32)
    n_sites = len(out_slot)
    if len(tensor_row) != len(prob_row) or len(site_off) != n_sites + 1 or (n_sites and int(site_off[-1]) != len(site_lines)) or \
            (n_sites == 0 and len(site_lines)):
        raise ValueError('mpn_clair_ensemble: the lists do not fit each other')
    n_out = int(n_out)
    device = tensors.device
    out_t = torch.empty((max(n_out, 0), CELLS), dtype=torch.int32, device=device)
    out_p = torch.empty((max(n_out, 0), PROBS), dtype=torch.float32, device=device)
    out_m = torch.empty((max(n_out, 0), PROBS), dtype=torch.int64, device=device) if micro else None
    bad = ct.c_int64(-1)
    torch.cuda.current_stream(device).synchronize()             # the native layer uses the default stream
    rc = lib.mpn_clair_ensemble(len(tensor_row), _p(tensor_row), _p(prob_row), tensors.data_ptr() if tensors.numel() else None, tensors.numel() // CELLS,
                                probs.data_ptr() if probs.numel() else None, probs.shape[0], 1 if probs.dtype == torch.float64 else 0, n_sites,
                                _p(site_off), _p(site_lines), _p(out_slot), n_out, out_t.data_ptr() if n_out > 0 else None,
                                out_p.data_ptr() if n_out > 0 else None, out_m.data_ptr() if micro and n_out > 0 else None, ct.byref(bad))
    if rc == -2:
        from . import _ffi
        raise ValueError(_ffi.last_error() or 'mpn_clair_ensemble: bad arguments')
    _check(rc, 'mpn_clair_ensemble')
    return out_t, out_p, out_m, bad.value


# ---- resident blocks ------------------------------------------------------------------------------------------------------------------
def _ensemble(centres, tensors, probs_list, ctg_name=None, minimum_count=0, keep=None, timings=None):
    """ensemble() -> (centres, tensors, probs, the first line of every site that is kept).  keep: None or the indices (into one
    model's rows) of the lines that take part, the same for every model."""
    import torch
    probs_list = list(probs_list)
    k = len(probs_list)
    if k == 0:
        raise ValueError('no probabilities')
    shared = isinstance(tensors, torch.Tensor)
    blocks = [tensors] * k if shared else list(tensors)
    cs = [np.asarray(centres, dtype=np.int64).reshape(-1)] * k if shared else [np.asarray(c, dtype=np.int64).reshape(-1) for c in centres]
    if len(blocks) != k or len(cs) != k:
        raise ValueError('the tensors, the centres and the probabilities differ in number')
    for c, b, p in zip(cs, blocks, probs_list):
        if not isinstance(b, torch.Tensor) or not isinstance(p, torch.Tensor) or b.numel() != len(c) * CELLS or p.dim() != 2 or p.shape[0] != len(c):
            raise ValueError('a block does not have one row per centre')
    t0 = time.perf_counter()
    n = [len(c) for c in cs]
    take = [np.arange(m) if keep is None else np.asarray(keep, dtype=np.int64) for m in n]
    if keep is not None and len(set(n)) > 1:
        raise ValueError('keep names the rows of every model: the models must have the same rows')
    base_p = np.concatenate([[0], np.cumsum(n)])[:-1]
    base_t = np.zeros(k, dtype=np.int64) if shared else base_p
    tensor_row = np.concatenate([t + b for t, b in zip(take, base_t)])
    prob_row = np.concatenate([t + b for t, b in zip(take, base_p)])
    keys = np.concatenate([c[t] for c, t in zip(cs, take)])
    site_off, site_lines, out_slot, n_out = group(keys, minimum_count)
    ingest._tick(timings, 'group', time.perf_counter() - t0)
    all_t = blocks[0].reshape(-1) if shared else torch.cat([b.reshape(-1) for b in blocks])
    all_p = probs_list[0] if k == 1 else torch.cat(probs_list)
    out_t, out_p, _, bad = ensemble_rows(tensor_row, prob_row, all_t.contiguous(), all_p.contiguous(), site_off, site_lines, out_slot, n_out)
    ingest._tick(timings, 'ensemble_device_ms', last_device_ms())
    first = site_lines[site_off[:-1]][out_slot >= 0] if len(out_slot) else np.zeros(0, dtype=np.int64)
    if bad >= 0:
        where = int(keys[site_lines[site_off[bad]]])
        raise ValueError(f'{ctg_name + ":" if ctg_name else "position "}{where}: a sum of tensor cells does not fit 32 bits')
    return keys[first].tolist(), out_t.reshape(-1, 33, 8, 4), out_p, (tensor_row[first] if len(first) else first)


def ensemble(centres, tensors, probs_list, ctg_name=None, minimum_count=0):
    """The lines of K models folded into one row per position.  tensors: one (n, 33, 8, 4) or (n, 1056) int32 tensor on the device
    that all K (n, 90) float32 (or float64) tensors of probs_list share, with the n positions `centres`; or K such tensors with K
    lists of centres, a pair per model.  The lines are those of model 0, then those of model 1 and so on, as the reference
    concatenates its files; a position that repeats inside a model (a deep site's resamples) counts once per line.
    -> (the position of every site with at least minimum_count lines, in order of first appearance; their (m, 33, 8, 4) int32 sums
    and (m, 90) float32 means, on the device).  The means are quantized as `{:.6f}` leaves them.  ValueError for blocks that do not
    fit and for a sum outside int32 (ctg_name is named in the message)."""
    return _ensemble(centres, tensors, probs_list, ctg_name, minimum_count)[:3]


# ---- the text tool --------------------------------------------------------------------------------------------------------------------
def micro_text(micro, negative_zero=False):
    """the text `{:.6f}` prints for an integer of micro-units"""
    if micro == 0:
        return '-0.000000' if negative_zero else '0.000000'
    a = abs(micro)
    return '%s%d.%06d' % ('-' if micro < 0 else '', a // 1000000, a % 1000000)


def ensemble_lines(stream, out, minimum_count_to_output=0, device='cuda', timings=None):
    """ensemble.py: the lines of `stream` (text or bytes; chrom, pos, refseq, 1056 integers, 90 probabilities, tab-separated) -> one
    line per (chrom, pos) pair of strings with at least minimum_count_to_output lines, in order of first appearance, written to `out`
    (a binary stream) -> the number of lines written.  The reference string is the first line's.  ValueError for a line whose column
    count is not 1149, a cell or a sum outside 32 bits, a probability that is not finite or not below 10^6 in magnitude."""
    import torch
    keys, seqs, cells, probs = [], [], [], []
    t0 = time.perf_counter()
    for no, line in enumerate(stream, 1):
        if isinstance(line, bytes):
            line = line.decode()
        f = line.split('\t')
        if len(f) != COLUMNS:
            raise ValueError(f'line {no} has {len(f)} columns, not {COLUMNS}')
        keys.append((f[0], f[1]))
        seqs.append(f[2])
        try:
            wide = np.array([int(v) for v in f[3:3 + CELLS]], dtype=np.int64)
            probs.append(np.array([float(v) for v in f[3 + CELLS:]], dtype=np.float64))
        except (ValueError, OverflowError) as e:
            raise ValueError(f'line {no}: {e}')
        cells.append(wide.astype(np.int32))
        if not bool((cells[-1] == wide).all()):
            raise ValueError(f'line {no}: a cell does not fit 32 bits')
        if not bool((np.abs(probs[-1]) < LIMIT).all()):
            raise ValueError(f'line {no}: a probability is not finite or not below {LIMIT:g}')
    if not keys:
        return 0
    site_off, site_lines, out_slot, n_out = group(keys, minimum_count_to_output)
    ingest._tick(timings, 'parse_group', time.perf_counter() - t0)
    rows = np.arange(len(keys))
    out_t, out_p, out_m, bad = ensemble_rows(rows, rows, torch.from_numpy(np.stack(cells)).to(device), torch.from_numpy(np.stack(probs)).to(device), site_off,
                                             site_lines, out_slot, n_out, micro=True)
    ingest._tick(timings, 'ensemble_device_ms', last_device_ms())
    first = site_lines[site_off[:-1]]
    if bad >= 0:
        raise ValueError('%s:%s: a sum of tensor cells does not fit 32 bits' % keys[first[bad]])
    t0 = time.perf_counter()
    out_t, out_m, minus = out_t.cpu().numpy(), out_m.cpu().numpy(), np.signbit(out_p.cpu().numpy())
    for s in np.flatnonzero(out_slot >= 0).tolist():
        k = out_slot[s]
        out.write('\t'.join([keys[first[s]][0], keys[first[s]][1], seqs[first[s]]] + [str(v) for v in out_t[k].tolist()] +
                            [micro_text(m, z) for m, z in zip(out_m[k].tolist(), minus[k].tolist())]).encode() + b'\n')
    ingest._tick(timings, 'format', time.perf_counter() - t0)
    return n_out


# ---- overlap_variant.py ---------------------------------------------------------------------------------------------------------------
NO_SECOND_ALT = 1024           # what the script takes for the length of a second ALT that is not there


def _variant(row, no):
    col = row.split('\t')
    last = col[-1].split(':')
    if len(col) < 6 or len(last) < 4:
        raise ValueError(f'line {no}: a data row needs six columns and GT:GQ:DP:AF in its last (the reference script raises here)')
    alts = col[4].split(',')
    try:
        return (col[0], int(col[1]), col[3], alts[0], None if len(alts) == 1 else alts[1], int(float(col[5])), last[0], last[2], last[3])
    except (ValueError, OverflowError) as e:
        raise ValueError(f'line {no}: {e}')


def _overlap(v1, v2):
    """is_two_variants_overlap: the deletion interval of the variant that comes first against the SNP and the deletion interval of
    the other, begin1 <= begin2 < end1"""
    if v1[0] != v2[0]:
        return False
    if v1[1] > v2[1]:
        v1, v2 = v2, v1
    longest = len(v1[2]) - min(len(v1[3]), NO_SECOND_ALT if v1[4] is None else len(v1[4]))
    if longest <= 0:
        return False
    begin1, end1 = v1[1] - 1, v1[1] + longest
    ref2, a2, b2 = len(v2[2]), len(v2[3]), (None if v2[4] is None else len(v2[4]))
    snp2 = ref2 == a2 or (b2 is not None and ref2 == b2)
    del2 = ref2 - min(a2, NO_SECOND_ALT if b2 is None else b2) > 0
    return (snp2 or del2) and begin1 <= v2[1] - 1 < end1          # (both intervals of the second begin at its position - 1)


def overlap_filter(lines):
    """overlap_variant.py, line for line: `lines` as readlines() gives them (text or bytes; the script drops the last character of
    every row, which is the newline) -> the rows it prints, without newlines.  Header rows pass through, ahead of the others.  A
    variant that the last kept variant overlaps (or is overlapped by) replaces it unless the kept one has the strictly higher
    integer QUAL; every row is rewritten with `.` for ID, FILTER and INFO and with GQ set to int(float(QUAL)).  ValueError, with the
    line number, where the script raises: a data row with fewer than six columns or fewer than four fields in its last column, a
    POS or QUAL that is no number."""
    head, kept = [], []
    for no, row in enumerate(lines, 1):
        if isinstance(row, bytes):
            row = row.decode()
        if row[:1] == '#':
            head.append(row[:-1])
            continue
        v = _variant(row[:-1], no)
        if kept and _overlap(kept[-1], v):
            if not kept[-1][5] > v[5]:
                kept[-1] = v
        else:
            kept.append(v)
    return head + ['\t'.join([v[0], str(v[1]), '.', v[2], v[3] if v[4] is None else v[3] + ',' + v[4], str(v[5]), '.', '.', 'GT:GQ:DP:AF',
                              ':'.join([v[6], str(v[5]), v[7], v[8]])]) for v in kept]


# ---- runClair-ensemble.sh for one contig ----------------------------------------------------------------------------------------------
def _write_bgzf(path, text):
    from . import bam
    with open(path, 'wb') as f:
        w = bam.BgzfWriter(f)
        w.write(text)
        w.close()


def candidate_positions(bam_fn, seq, ctg_name, threshold=0.125, min_coverage=4, device='cuda', timings=None):
    """the 1-based positions extract_variant_candidates prints for the contig `seq` (its bytes), as an int64 array, without the text"""
    p = candidates.pileup(bam_fn, ctg_name, None, None, 0, device, ctg_len=len(seq), timings=timings)
    if not p.n_taken:
        return np.zeros(0, dtype=np.int64)
    ref_bytes = np.zeros(p.hi - p.lo, dtype=np.uint8)
    part = np.frombuffer(seq, dtype=np.uint8)[p.lo:p.hi]
    ref_bytes[:len(part)] = part
    return candidates.pileup_candidates(p.counts, p.lo, ref_bytes, None, min_coverage, threshold)['pos'].astype(np.int64) + 1


def call_ensemble(bam_fn, ref_fn, chkpnt_fns, ctg_name, out_dir, threshold=0.125, sample_name='Amplicon', min_coverage=4, rng=None, nets=None,
                  show_reference=False, verify_crc=True, device='cuda', timings=None):
    """bin/runClair-ensemble.sh for one contig: candidates (threshold), tensors (one draw, shared by the models), ClairNet.predict per
    checkpoint prefix of chkpnt_fns (or per ClairNet of `nets`), ensemble with minimum_count = (K + 2) // 2, call_variants with
    pysam_for_all_indel_bases, the rows ordered by position, overlap_filter.  Everything between the BAM and the text of the VCF stays
    on the device.  Writes out_dir/snp_and_indel.vcf.gz and out_dir/snp_and_indel.filtered.vcf.gz (BGZF, no .tbi) -> (the number of
    records, the number after the filter).  rng: random.Random's sample, for sites of more than 100 reads.  show_reference:
    call_var's --showRef, which the driver does not pass.  ctg_name None: the one contig of the BAM.  ValueError for a BAM with several contigs and no name, and for what the stages refuse."""
    import random
    from . import clair_net
    names = [n for n, _ in candidates.bam_references(bam_fn)]
    if ctg_name is None:
        if len(names) != 1:
            raise ValueError(f'{bam_fn}: {len(names)} contigs: name the one to call (one contig per call)')
        ctg_name = names[0]
    if isinstance(ctg_name, (list, tuple)) or ',' in ctg_name:
        raise ValueError('one contig per call')
    t_all = time.perf_counter()
    seq = candidates.read_contig(ref_fn, ctg_name)
    if not seq:
        raise ValueError(f'{ref_fn}: no contig {ctg_name}')
    positions = candidate_positions(bam_fn, seq, ctg_name, threshold, min_coverage, device, timings)
    centres, block, refs = clair_tensor.tensors(bam_fn, ref_fn, positions, ctg_name, rng=rng or random, device=device, timings=timings)
    own = nets is None
    nets = [clair_net.ClairNet.from_checkpoint(fn, device=device, verify_crc=verify_crc) for fn in chkpnt_fns] if own else list(nets)
    try:
        probs = [net.predict(block) for net in nets]
    finally:
        if own:
            for net in nets:
                net.close()
    k = len(probs)
    # call_var's batch_output_for_ensemble prints no line for a centre base that is not one of ACGT
    keep = np.array([i for i, s in enumerate(refs) if len(s) > 16 and s[16] in 'ACGT'], dtype=np.int64)
    sites, sums, means, first = _ensemble(centres, block, probs, ctg_name, (k + 2) // 2, keep=keep, timings=timings)
    body = io.BytesIO()
    clair_call.call_variants(bam_fn, ref_fn, ctg_name, sites, sums.contiguous(), means, [refs[i] for i in first.tolist()], body,
                             show_reference=show_reference, pysam_for_all_indel_bases=True, timings=timings)
    t0 = time.perf_counter()
    rows = body.getvalue().decode().splitlines()
    rows.sort(key=lambda r: int(r.split('\t', 2)[1]))              # sort -k1,1V -k2,2n for one contig (stable; a position has one row)
    head = clair_call.vcf_header(sample_name, ref_fn)
    text = head + ''.join(r + '\n' for r in rows)
    filtered = overlap_filter(text.splitlines(keepends=True))
    ingest._tick(timings, 'overlap_filter', time.perf_counter() - t0)
    os.makedirs(out_dir, exist_ok=True)
    _write_bgzf(os.path.join(out_dir, 'snp_and_indel.vcf.gz'), text.encode())
    _write_bgzf(os.path.join(out_dir, 'snp_and_indel.filtered.vcf.gz'), ''.join(r + '\n' for r in filtered).encode())
    ingest._tick(timings, 'call_ensemble', time.perf_counter() - t_all)
    return len(rows), len(filtered) - head.count('\n')


# ---- the command lines ----------------------------------------------------------------------------------------------------------------
def main_ensemble(argv, prog='mpn-ensemble'):
    """The command line of `clair.py ensemble`."""
    from argparse import ArgumentParser
    ap = ArgumentParser(prog=prog, description='Average the lines of --output_for_ensemble per site (on the GPU): standard input to standard output')
    ap.add_argument('--minimum_count_to_output', type=int, default=0, help='minimum # of calls to output the probabilities')
    if not argv:
        ap.print_help()
        return 1
    a = ap.parse_args(argv)
    buf = io.BytesIO()
    try:
        ensemble_lines(sys.stdin.buffer, buf, a.minimum_count_to_output)
    except (ValueError, OSError) as e:
        print(f'{prog}: {e}', file=sys.stderr)
        return 1
    sys.stdout.buffer.write(buf.getvalue())
    sys.stdout.buffer.flush()
    return 0


def main_overlap(argv, prog='mpn-overlap-variant'):
    """The command line of overlap_variant.py: it takes no arguments."""
    if argv:
        print(f'usage: {prog} < sorted.vcf > filtered.vcf', file=sys.stderr)
        return 2
    try:
        rows = overlap_filter(sys.stdin.buffer.readlines())
    except ValueError as e:
        print(f'{prog}: {e}', file=sys.stderr)
        return 1
    sys.stdout.buffer.write(''.join(r + '\n' for r in rows).encode())
    sys.stdout.buffer.flush()
    return 0


def main_call(argv, prog='mpn-clair-ensemble'):
    """bin/runClair-ensemble.sh for one contig."""
    from argparse import ArgumentParser
    ap = ArgumentParser(prog=prog, description='Call the variants of one contig with an ensemble of Clair models (on the GPU)')
    ap.add_argument('-b', dest='bam', required=True, help='sorted BAM file')
    ap.add_argument('-r', dest='ref', required=True, help='reference FASTA, plain or gzip (no .fai is needed)')
    ap.add_argument('-m', dest='models', required=True, help='checkpoint prefixes, separated by commas')
    ap.add_argument('-c', dest='contig', default=None, help='the contig; needed when the BAM has more than one')
    ap.add_argument('-o', dest='out', required=True, help='output folder: snp_and_indel.vcf.gz and snp_and_indel.filtered.vcf.gz')
    ap.add_argument('-t', dest='threads', type=int, default=1, help='accepted and ignored: one process does all sites')
    ap.add_argument('--no_crc', action='store_true', help='do not verify the checkpoints\' checksums')
    if not argv:
        ap.print_help()
        return 1
    a = ap.parse_args(argv)
    try:
        n, m = call_ensemble(a.bam, a.ref, [x for x in a.models.split(',') if x], a.contig, a.out, verify_crc=not a.no_crc)
    except (ValueError, OSError) as e:
        print(f'{prog}: {e}', file=sys.stderr)
        return 1
    print(f'{prog}: {n} records, {m} after the overlap filter', file=sys.stderr)
    return 0
