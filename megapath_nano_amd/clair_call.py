"""Clair's probabilities decoded into VCF records on the GPU: a drop-in for output_with / output_from of clair/call_var.py
(--input_probabilities, and the decoding behind a model's own run) and for its pysam look-ups.  The rules, the quirks that are
reproduced and the differences are DESIGN.md section 6 item 19; the native calls are include/mpn_call.h.

    indel_events(bam_fn, ctg_name, positions, contig_len)            -> the distinct indel events of every site's pile-up column
    decode(centres, tensors, probs, refs, events, contig, ..)        -> the compact rows of the sites that give a record
    call_variants(bam_fn, ref_fn, ctg_name, centres, tensors, ..)    resident tensors and probabilities -> VCF text
    call_var_with_probabilities(stream, bam_fn, ref_fn, out, ..)     the lines of --output_for_ensemble -> VCF text
    vcf_header(sample_name, ref_fn)                                  the reference's header; ##contig from the FASTA itself
    bin/mpn-call-vcf                                                 the command line of the reference script

The BAM goes to HBM group by group (MPN_INGEST_BATCH_BYTES) through ingest.BamTexts, each text beginning at the first record that an
unfinished site still needs (keep_from); no pysam, .bai or .fai is used.
The device gives, per record, the alleles, the genotype, the float32 product p and the integer counts; the host keeps what hangs on
libm and printf: the quality from p (math.log in float64, as NumPy 1.x promotes `1.0 - p`), `%.4f` of the allele frequency
(float64, capped at 1), PASS / LowQual and the line."""
import gzip
import io
import math
import os
import sys
import ctypes as ct

import numpy as np

from . import _ffi, candidates, clair_tensor, fastx, ingest
from ._ffi import check as _check, ptr as _p

FLANK, CELLS, PROBS, REF_BYTES = 16, 1056, 90, 33
MAX_LEN, MAX_EVENTS, ALLELE_BYTES, ALT1_AT, ALT2_AT = 50, 256, 256, 51, 152
PYSAM_ALL, HAPLOID, SHOW_REF = 1, 2, 4
EMITTED, NOT_ACGT, NO_DEPTH, REFERENCE, SAME, RAISES, BAD_PROB, LONG_KEY = range(8)
CALL_READ = np.dtype([('off', '<i8'), ('rlen', '<i8'), ('pos', '<i4'), ('reverse', '<i4')])                                   # mpn_call_read
CALL_EVENT = np.dtype([('kind', '<i4'), ('len', '<i4'), ('count', '<i4'), ('rank', '<i4'), ('clip', '<i4'), ('key_len', '<i4'),
                       ('bases', '<i8')])                                                                                      # mpn_call_event
CALL_ROW = np.dtype([('site', '<i4'), ('flags', '<i4'), ('genotype', '<i4'), ('gt21', '<i4'), ('genotype_task', '<i4'), ('p', '<f4'),
                     ('supported', '<i4'), ('depth', '<i4'), ('ref_len', '<i4'), ('alt1_len', '<i4'), ('alt2_len', '<i4'), ('reserved', '<i4')])   # mpn_call_row
GENOTYPES = ('0/0', '1/1', '0/1', '1/2')
HEADER = '''##fileformat=VCFv4.1
##FILTER=<ID=PASS,Description="All filters passed">
##FILTER=<ID=LowQual,Description="Confidence in this variant being real is below calling threshold.">
##ALT=<ID=DEL,Description="Deletion">
##ALT=<ID=INS,Description="Insertion of novel sequence">
##INFO=<ID=SVTYPE,Number=1,Type=String,Description="Type of structural variant">
##INFO=<ID=LENGUESS,Number=.,Type=Integer,Description="Best guess of the indel length">
##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">
##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype Quality">
##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Read Depth">
##FORMAT=<ID=AF,Number=1,Type=Float,Description="Estimated allele frequency in the range (0,1)">
'''

_bound = False


def _lib():
    global _bound
    lib = candidates._lib()
    if not _bound:
        P, I64, I32 = ct.c_void_p, ct.c_int64, ct.c_int32
        lib.mpn_call_indels.argtypes = [P, I64, I64, P, I64, P, P, P, I64, P, P, P, P, I64, P, P]
        lib.mpn_call_decode.argtypes = [I64, P, P, P, P, P, P, I64, P, P, P, P, I64, I32, P, P, P, P]
        lib.mpn_call_quantize.argtypes = [P, I64]
        for f in (lib.mpn_call_indels, lib.mpn_call_decode, lib.mpn_call_quantize):
            f.restype = I32
        lib.mpn_call_last_device_ms.argtypes = [ct.POINTER(ct.c_double)] * 3
        lib.mpn_call_last_device_ms.restype = None
        _bound = True
    return lib


def last_device_ms():
    """-> (indels ms, decode ms, quantize ms) of the calling thread's last native calls"""
    return _ffi.device_ms(_lib().mpn_call_last_device_ms, 3)


class Events:
    """The events of a list of sites: sites (1-based, ascending), off (len(sites) + 1 offsets), events (a uint8 tensor on the device,
    32 bytes an event: mpn_call_event), bases (a uint8 tensor on the device, 50 bytes an event)."""

    def __init__(self, sites, off, events, bases):
        self.sites, self.off, self.events, self.bases = sites, off, events, bases

    def host(self):
        """-> [[(kind, len, count, rank, clip, the key's text; None for an insertion whose key is too long)] per site]"""
        ev = np.frombuffer(self.events.cpu().numpy().tobytes(), dtype=CALL_EVENT)
        bases = self.bases.cpu().numpy().tobytes()
        out = []
        for c in range(len(self.sites)):
            out.append([(int(e['kind']), int(e['len']), int(e['count']), int(e['rank']), int(e['clip']),
                         (bases[i * MAX_LEN:i * MAX_LEN + int(e['key_len'])].decode() if e['key_len'] >= 0 else None) if e['kind'] == 0 else '')
                        for i, e in zip(range(int(self.off[c]), int(self.off[c + 1])), ev[int(self.off[c]):int(self.off[c + 1])])])
        return out


# ---- the native calls ---------------------------------------------------------------------------------------------------------------
def site_ranges(pos, rlen, sites):
    """The range of records [begin, end) that mpn_call_indels looks at for every site (1-based): from the first whose running
    maximum of pos + max(rlen, 1) passes the 0-based base `site` to the last whose pos is at most `site`."""
    pos, rlen, sites = np.asarray(pos, dtype=np.int64), np.asarray(rlen, dtype=np.int64), np.asarray(sites, dtype=np.int64)
    reach = np.maximum.accumulate(pos + np.maximum(rlen, 1)) if len(pos) else pos
    begin = np.searchsorted(reach, sites, side='right')
    end = np.searchsorted(pos, sites, side='right')
    return begin.astype(np.int64), np.maximum(end, begin).astype(np.int64)


def call_indels(text, text_len, reads, sites, begin, end, contig_len):
    """mpn_call_indels, twice: count, then fill -> (counts, offsets [m + 1], events and bases: uint8 tensors on the device, bad
    read or -1, bad site or -1)"""
    import torch
    lib = _lib()
    reads = np.ascontiguousarray(reads, dtype=CALL_READ)
    sites = np.ascontiguousarray(sites, dtype=np.int32)
    begin, end = np.ascontiguousarray(begin, dtype=np.int64), np.ascontiguousarray(end, dtype=np.int64)
    if not (len(sites) == len(begin) == len(end)):
        raise ValueError('mpn_call_indels: the sites and their ranges differ in number')
    counts, bad_read, bad_site = np.zeros(len(sites), dtype=np.int64), ct.c_int64(-1), ct.c_int64(-1)
    _check(lib.mpn_call_indels(text.data_ptr(), int(text_len), len(reads), _p(reads), len(sites), _p(sites), _p(begin), _p(end), int(contig_len),
                               _p(counts), None, None, None, 0, ct.byref(bad_read), ct.byref(bad_site)), 'mpn_call_indels')
    ms = last_device_ms()[0]
    off = np.zeros(len(sites) + 1, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    total = int(off[-1])
    events = torch.zeros(max(total, 1) * CALL_EVENT.itemsize, dtype=torch.uint8, device=text.device)
    bases = torch.zeros(max(total, 1) * MAX_LEN, dtype=torch.uint8, device=text.device)
    if total and bad_read.value < 0 and bad_site.value < 0:
        first = np.ascontiguousarray(off[:-1])
        _check(lib.mpn_call_indels(text.data_ptr(), int(text_len), len(reads), _p(reads), len(sites), _p(sites), _p(begin), _p(end), int(contig_len),
                                   _p(counts), _p(first), events.data_ptr(), bases.data_ptr(), total, ct.byref(bad_read), ct.byref(bad_site)),
               'mpn_call_indels')
        ms += last_device_ms()[0]
    return counts, off, events[:total * CALL_EVENT.itemsize], bases[:total * MAX_LEN], bad_read.value, bad_site.value, ms


def quantize(probs):
    """mpn_call_quantize in place: what `%.6f` and a float32 parse leave of the probabilities"""
    import torch
    if not isinstance(probs, torch.Tensor) or probs.dtype != torch.float32 or not probs.is_cuda or not probs.is_contiguous():
        raise ValueError('the probabilities are not a contiguous float32 tensor on the device')
    torch.cuda.current_stream(probs.device).synchronize()
    _check(_lib().mpn_call_quantize(probs.data_ptr() if probs.numel() else None, probs.numel()), 'mpn_call_quantize')
    return probs


# ---- the events of a file -------------------------------------------------------------------------------------------------------------
def indel_events(bam_fn, ctg_name, positions, contig_len, device='cuda', timings=None):
    """The distinct indel events of the pile-up column of every 1-based position (ascending, without duplicates) -> Events.
    ValueError for positions that are not ascending, records of the contig that are not sorted, a read of a column whose CIGAR
    or bases do not fit, more than 256 distinct events at a site."""
    import torch
    device = device or 'cuda'
    _lib()
    sites = np.asarray(positions, dtype=np.int64).reshape(-1)
    if len(sites) and (bool((sites[1:] <= sites[:-1]).any()) or int(sites[0]) < 1 or int(sites[-1]) > 0x7ffffff0):
        raise ValueError('the sites are not ascending 1-based positions')
    tid, _ = candidates.contig_tid(bam_fn, ctg_name)
    next_site, last_pos = 0, None
    offs, evs, bss = [np.zeros(1, dtype=np.int64)], [], []
    with ingest.BamTexts(bam_fn, device) as texts:
        while next_site < len(sites):
            t = next(texts)
            text, text_len, rows, final = t.text, t.text_len, t.rows, t.final
            keep, pos, rlen, last_pos = clair_tensor.contig_reads(t, tid, last_pos, f'{bam_fn}: the records of {ctg_name} are not sorted by position')
            todo = sites[next_site:]
            n_fin = len(todo) if final else (int(np.searchsorted(todo, int(pos[-1]), side='left')) if len(pos) else 0)
            if n_fin:
                fin = todo[:n_fin]
                begin, end = site_ranges(pos, rlen, fin)
                reads = np.zeros(len(keep), dtype=CALL_READ)
                reads['off'], reads['rlen'], reads['pos'], reads['reverse'] = rows['off'][keep], rlen, pos, (rows['flag'][keep] & 16) != 0
                counts, off, events, bases, bad_read, bad_site, ms = call_indels(text, text_len, reads, fin, begin, end, contig_len)
                ingest._tick(timings, 'indels_device_ms', ms)
                if bad_read >= 0:
                    raise ValueError(f'{bam_fn}: record {candidates._record_name(text, rows[keep[bad_read]])}: in the pile-up column of a site its '
                                     'CIGAR or bases do not fit')
                if bad_site >= 0:
                    raise ValueError(f'{bam_fn}: position {int(fin[bad_site])}: more than {MAX_EVENTS} distinct indel events')
                offs.append(off[1:] + offs[-1][-1])
                evs.append(events.clone())
                bss.append(bases.clone())
                next_site += n_fin
            if final:
                break
            cut = len(rows)
            if next_site < len(sites) and len(pos):
                b = int(site_ranges(pos, rlen, sites[next_site:next_site + 1])[0][0])
                if b < len(keep):
                    cut = int(keep[b])
                    last_pos = int(pos[b])                # the next text starts again at this record
            texts.keep_from(cut)
    off = np.concatenate(offs)
    if len(off) < len(sites) + 1:                      # (the file ended before the last sites)
        off = np.concatenate([off, np.full(len(sites) + 1 - len(off), off[-1], dtype=np.int64)])
    events = torch.cat(evs) if evs else torch.zeros(0, dtype=torch.uint8, device=device)
    bases = torch.cat(bss) if bss else torch.zeros(0, dtype=torch.uint8, device=device)
    if events.numel():                                 # the offsets into the arena of this list
        events.view(torch.int64).view(-1, 4)[:, 3] = torch.arange(events.numel() // CALL_EVENT.itemsize, device=events.device) * MAX_LEN
    return Events(sites, off, events, bases)


# ---- the decoding ---------------------------------------------------------------------------------------------------------------------
def _options(pysam_for_all_indel_bases, haploid, show_reference):
    return (PYSAM_ALL if pysam_for_all_indel_bases else 0) | (HAPLOID if haploid else 0) | (SHOW_REF if show_reference else 0)


def decode(centres, tensors, probs, refs, events, contig, pysam_for_all_indel_bases=False, haploid=False, show_reference=False):
    """centres: the 1-based position per tensor (any order, repeats allowed; each must be one of events.sites); tensors: an
    (n, 33, 8, 4) or (n, 1056) int32 tensor on the device; probs: an (n, 90) float32 tensor there; refs: the reference string per
    tensor; contig: the bytes of the contig (or a uint8 tensor of them on the device) -> (rows: a CALL_ROW array of the sites that
    give a record, in the order of the tensors; alleles: a (len(rows), 256) uint8 array; status: one per tensor; LONG_KEY marks a site
    that is left out because the chosen insertion has a deletion spelled behind it and the text passes 50 bytes).  ValueError for
    wrong dtypes or shapes, a probability that is NaN, negative or infinite, and where the reference script raises."""
    import torch
    lib = _lib()
    n = len(centres)
    if not isinstance(tensors, torch.Tensor) or tensors.dtype != torch.int32 or not tensors.is_cuda or not tensors.is_contiguous() or \
            tensors.numel() != n * CELLS or (n and tuple(tensors.shape[1:]) not in ((33, 8, 4), (CELLS,))):
        raise ValueError('the tensors are not a contiguous (n, 33, 8, 4) int32 block on the device')
    if not isinstance(probs, torch.Tensor) or probs.dtype != torch.float32 or not probs.is_cuda or not probs.is_contiguous() or \
            tuple(probs.shape) != (n, PROBS):
        raise ValueError('the probabilities are not a contiguous (n, 90) float32 block on the device')
    if len(refs) != n:
        raise ValueError('the reference strings and the tensors differ in number')
    site = np.asarray(centres, dtype=np.int64).reshape(-1)
    at = np.searchsorted(events.sites, site)
    if n and (bool((at >= len(events.sites)).any()) or bool((events.sites[np.minimum(at, len(events.sites) - 1)] != site).any())):
        raise ValueError('a tensor\'s position is not among the sites of the events')
    ref_n = np.array([len(s) for s in refs], dtype=np.int32)
    if n and (int(ref_n.min()) <= FLANK or int(ref_n.max()) > REF_BYTES):
        raise ValueError('a reference string has no centre base, or more than 33 bases')
    flat = np.zeros((n, REF_BYTES), dtype=np.uint8)
    for i, s in enumerate(refs):
        flat[i, :len(s)] = np.frombuffer(s.encode() if isinstance(s, str) else s, dtype=np.uint8)
    device = tensors.device
    d_refs = torch.from_numpy(flat).to(device)
    d_contig = contig if isinstance(contig, torch.Tensor) else torch.from_numpy(np.frombuffer(bytes(contig), dtype=np.uint8).copy()).to(device)
    ev_begin, ev_end = np.ascontiguousarray(events.off[at]), np.ascontiguousarray(events.off[at + 1] if n else events.off[:0])
    site32, status, n_rows = np.ascontiguousarray(site, dtype=np.int32), np.zeros(n, dtype=np.int32), ct.c_int64(0)
    d_rows = torch.zeros(max(n, 1) * CALL_ROW.itemsize, dtype=torch.uint8, device=device)
    d_alleles = torch.zeros(max(n, 1) * ALLELE_BYTES, dtype=torch.uint8, device=device)
    n_events = events.events.numel() // CALL_EVENT.itemsize
    torch.cuda.current_stream(device).synchronize()             # the native layer uses the default stream
    _check(lib.mpn_call_decode(n, _p(site32), probs.data_ptr() if n else None, tensors.data_ptr() if n else None, d_refs.data_ptr() if n else None,
                               _p(ref_n), d_contig.data_ptr() if d_contig.numel() else None, d_contig.numel(), _p(ev_begin), _p(ev_end),
                               events.events.data_ptr() if n_events else None, events.bases.data_ptr() if n_events else None, n_events,
                               _options(pysam_for_all_indel_bases, haploid, show_reference), _p(status), d_rows.data_ptr(), d_alleles.data_ptr(),
                               ct.byref(n_rows)), 'mpn_call_decode')
    for what, text in ((BAD_PROB, 'a probability is NaN, negative or infinite'),
                       (RAISES, 'the reference script raises here (a centre base U in a heterozygous call)')):
        bad = np.flatnonzero(status == what)
        if len(bad):
            raise ValueError(f'position {int(site[bad[0]])}: {text}')
    k = int(n_rows.value)
    rows = np.frombuffer(d_rows[:k * CALL_ROW.itemsize].cpu().numpy().tobytes(), dtype=CALL_ROW)
    alleles = d_alleles[:k * ALLELE_BYTES].cpu().numpy().reshape(k, ALLELE_BYTES)
    return rows, alleles, status


# ---- the host's part ------------------------------------------------------------------------------------------------------------------
def quality_score(p):
    """quality_score_from for the float32 product p, in float64 as NumPy 1.x promotes `1.0 - p`"""
    p = float(p)
    tmp = max((-10 * math.log(math.e, 10)) * math.log(((1.0 - p) + 1e-300) / (p + 1e-300)) + 16, 0)
    return int(round(tmp * tmp))


def format_rows(ctg_name, centres, rows, alleles, qual=None):
    """the lines of output_with for the rows of decode() -> [text]"""
    out = []
    for row, a in zip(rows, alleles):
        a = a.tobytes()
        ref, alt = a[:row['ref_len']].decode(), a[ALT1_AT:ALT1_AT + row['alt1_len']].decode()
        if row['alt2_len']:
            alt += ',' + a[ALT2_AT:ALT2_AT + row['alt2_len']].decode()
        q = quality_score(row['p'])
        af = (int(row['supported']) + 0.0) / int(row['depth'])
        if af > 1:
            af = 1
        filt = '.' if qual is None else ('PASS' if q >= qual else 'LowQual')
        out.append('%s\t%d\t.\t%s\t%s\t%d\t%s\t%s\tGT:GQ:DP:AF\t%s:%d:%d:%.4f' % (ctg_name, int(centres[row['site']]), ref, alt, q, filt, '.',
                                                                                GENOTYPES[row['genotype']], q, int(row['depth']), af))
    return out


def vcf_header(sample_name='SAMPLE', ref_fn=None):
    """The reference's header.  The ##contig lines come from the FASTA itself (the name up to the first blank, and the length),
    not from a .fai."""
    text = HEADER
    if ref_fn is not None:
        kind, stream = fastx.open_once(ref_fn)
        if kind not in ('plain', 'gzip'):
            raise ValueError(f'{ref_fn}: the reference is a FASTA file, plain or gzip')
        with stream:
            for name, seq, _ in fastx.iter_fastx(stream):
                text += '##contig=<ID=%s,length=%d>\n' % (name.decode() if isinstance(name, bytes) else name, len(seq))
    return text + '#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n' % sample_name


def call_variants(bam_fn, ref_fn, ctg_name, centres, tensors, probs, refs, out, qual=None, show_reference=False, haploid=False,
                  pysam_for_all_indel_bases=False, quantize_probs=False, timings=None):
    """Resident tensors and probabilities of one contig -> the lines of the VCF (without the header), written to `out` (a binary
    stream) -> the number of lines.  quantize_probs: the probabilities first take the round trip through `%.6f` (on a copy), so the
    lines are those of the text pipeline."""
    seq = candidates.read_contig(ref_fn, ctg_name)
    if not seq:
        raise ValueError(f'{ref_fn}: no contig {ctg_name}')
    if quantize_probs:
        probs = quantize(probs.clone())
    sites = np.unique(np.asarray(centres, dtype=np.int64))
    events = indel_events(bam_fn, ctg_name, sites, len(seq), device=tensors.device, timings=timings)
    rows, alleles, status = decode(centres, tensors, probs, refs, events, seq, pysam_for_all_indel_bases, haploid, show_reference)
    for i in np.flatnonzero(status == LONG_KEY).tolist():
        print(f'{ctg_name}:{int(centres[i])}: left out: the chosen insertion is directly followed by a deletion and the text the reference '
              'would print as its bases is longer than 50 bytes', file=sys.stderr)
    ingest._tick(timings, 'decode_device_ms', last_device_ms()[1])
    lines = format_rows(ctg_name, centres, rows, alleles, qual)
    out.write(''.join(line + '\n' for line in lines).encode())
    return len(lines)


def read_probability_lines(stream):
    """the lines of --output_for_ensemble -> [(ctg, pos, refseq)], an (n, 1056) int32 array, an (n, 90) float32 array"""
    heads, cells, probs = [], [], []
    for line in stream:
        if isinstance(line, bytes):
            line = line.decode()
        f = line.rstrip('\n').split('\t')
        if len(f) <= 1:
            continue
        if len(f) != 3 + CELLS + PROBS:
            raise ValueError(f'a line has {len(f)} columns, not {3 + CELLS + PROBS}')
        heads.append((f[0], int(f[1]), f[2]))
        cells.append(np.array(f[3:3 + CELLS], dtype=np.float32).astype(np.int32))
        probs.append(np.array(f[3 + CELLS:], dtype=np.float32))
    return heads, (np.stack(cells) if cells else np.zeros((0, CELLS), dtype=np.int32)), (np.stack(probs) if probs else np.zeros((0, PROBS), dtype=np.float32))


def _by_contig(heads):
    at = 0
    while at < len(heads):
        b = at
        while b < len(heads) and heads[b][0] == heads[at][0]:
            b += 1
        yield at, b
        at = b


def call_var_with_probabilities(stream, bam_fn, ref_fn, out, sample_name='SAMPLE', qual=None, show_reference=False, haploid=False,
                                pysam_for_all_indel_bases=False, device='cuda'):
    """call_var.py --input_probabilities: the lines of `stream` -> the VCF with its header, written to `out` -> the number of records"""
    import torch
    heads, cells, probs = read_probability_lines(stream)
    out.write(vcf_header(sample_name, ref_fn).encode())
    n = 0
    for a, b in _by_contig(heads):
        n += call_variants(bam_fn, ref_fn, heads[a][0], [h[1] for h in heads[a:b]], torch.from_numpy(cells[a:b]).to(device).reshape(-1, 33, 8, 4),
                           torch.from_numpy(probs[a:b]).to(device), [h[2] for h in heads[a:b]], out, qual, show_reference, haploid,
                           pysam_for_all_indel_bases)
    return n


def main(argv, prog='mpn-call-vcf'):
    """The command line of clair/call_var.py, for the VCF."""
    from argparse import ArgumentParser
    ap = ArgumentParser(prog=prog, description='Call variants from tensors or probabilities of candidate sites: the VCF (on the GPU)')
    ap.add_argument('--tensor_fn', type=str, default='PIPE', help='Tensor input of mpn-create-tensor: a gzip file, PIPE for standard input')
    ap.add_argument('--chkpnt_fn', type=str, default=None, help='the prefix of a model checkpoint')
    ap.add_argument('--call_fn', type=str, default=None, help='Output variant predictions; standard output when not given')
    ap.add_argument('--bam_fn', type=str, default='bam.bam', help='BAM file input, default: %(default)s')
    ap.add_argument('--ref_fn', type=str, default=None, help='Reference fasta file input (plain or gzip; no .fai is needed)')
    ap.add_argument('--qual', type=int, default=None, help='If set, variant with equal or higher quality will be marked PASS, or LowQual otherwise')
    ap.add_argument('--sampleName', type=str, default='SAMPLE', help='Define the sample name to be shown in the VCF file')
    ap.add_argument('--showRef', action='store_true', help='Show reference calls')
    ap.add_argument('--haploid', action='store_true', help='call haploid instead of diploid')
    ap.add_argument('--pysam_for_all_indel_bases', action='store_true', help='Always take the indel bases from the reads')
    ap.add_argument('--input_probabilities', action='store_true', help='Accept probabilities as input (standard input)')
    ap.add_argument('--debug', action='store_true', help='refused')
    ap.add_argument('--activation_only', action='store_true', help='refused')
    ap.add_argument('--output_for_ensemble', action='store_true', help='refused: that is bin/mpn-call-var')
    ap.add_argument('--no_crc', action='store_true', help='do not verify the checkpoint\'s checksums')
    if not argv:
        ap.print_help()
        return 1
    a = ap.parse_args(argv)
    if a.debug or a.activation_only:
        print(f'{prog}: --debug and --activation_only are not implemented', file=sys.stderr)
        return 2
    if a.output_for_ensemble:
        print(f'{prog}: --output_for_ensemble is bin/mpn-call-var; this tool writes the VCF', file=sys.stderr)
        return 2
    if a.ref_fn is None:
        print(f'{prog}: --ref_fn is needed: the deleted bases are read from it', file=sys.stderr)
        return 2
    buf = io.BytesIO()
    kw = dict(qual=a.qual, show_reference=a.showRef, haploid=a.haploid, pysam_for_all_indel_bases=a.pysam_for_all_indel_bases)
    try:
        if a.input_probabilities:
            call_var_with_probabilities(sys.stdin.buffer, a.bam_fn, a.ref_fn, buf, sample_name=a.sampleName, **kw)
        else:
            import torch
            from . import clair_net
            if not a.chkpnt_fn:
                print(f'{prog}: --chkpnt_fn is needed', file=sys.stderr)
                return 2
            net = clair_net.ClairNet.from_checkpoint(a.chkpnt_fn, verify_crc=not a.no_crc)
            if a.tensor_fn == 'PIPE':
                heads, cells = clair_net.read_tensor_lines(sys.stdin.buffer)
            else:
                with gzip.open(a.tensor_fn, 'rb') as f:
                    heads, cells = clair_net.read_tensor_lines(f)
            buf.write(vcf_header(a.sampleName, a.ref_fn).encode())
            for x, y in _by_contig(heads):
                block = torch.from_numpy(cells[x:y]).to(net.device).reshape(-1, 33, 8, 4)
                call_variants(a.bam_fn, a.ref_fn, heads[x][0], [int(h[1]) for h in heads[x:y]], block, net.predict(block), [h[2] for h in heads[x:y]],
                              buf, **kw)
    except (ValueError, OSError) as e:
        print(f'{prog}: {e}', file=sys.stderr)
        return 1
    if a.call_fn:
        os.makedirs(os.path.dirname(os.path.abspath(a.call_fn)), exist_ok=True)
        with open(a.call_fn, 'wb') as f:
            f.write(buf.getvalue())
    else:
        sys.stdout.buffer.write(buf.getvalue())
        sys.stdout.buffer.flush()
    return 0
