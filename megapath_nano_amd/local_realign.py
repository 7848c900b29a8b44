"""Local realignment around called variants on the GPU: a drop-in for the reference's realignment/realignment.sh -p ont, that is for
local_realignment.py (one process per VCF position there, with three samtools processes each) and extract_vcf_position.py.  The
rules, the quirks that are reproduced and the differences are DESIGN.md section 6 item 20; the native calls are
include/mpn_local_realign.h.

    alt_info(bam_fn, ref_fn, ctg_name, positions)                 -> {position: (depth, {allele: count})}, ascending
    local_realignment(bam_fn, ref_fn, ctg_name, positions, out)   writes the script's lines `ctg pos depth json pos`
    extract_vcf_position(vcf_fn, alt, output_fn)                  ExtractVcfPosition: DP and AF of the VCF from those lines
    bin/mpn-local-realign                                         the command line of realignment.sh

The BAM goes to HBM group by group (MPN_INGEST_BATCH_BYTES) through ingest.BamTexts, each text beginning at the first record that an
unfinished site still needs (keep_from); no samtools, .bai or .fai is used.
Per group the host bisects every site's range of records and keeps those that overlap its region (numpy; samtools' -d 8000 rule runs
in the native layer for the sites that have 8000 candidates); the device finds the surviving columns, builds every read's fragment,
aligns it (SSW) against the site's reference window and counts the alleles.  Fragments, SSW results and CIGARs never leave HBM; the host
gets, per site, the depth and the ordered list of (key, count), and formats JSON.

MPN_LR_SSW_CHUNK (default 262144: the sweep in profiles/r24_local_realign/README.md gets faster up to there and gains 0.4 % beyond):
the (site, read) pairs of one SSW launch; sites are not split, so a site of 8001 reads is one chunk however small the knob.  Workspace of a chunk on the device, per pair: the fragment twice (letters and codes, <= ~1 KiB), 36 bytes of
results, 1280 bytes of column maxima, 4 bytes per CIGAR slot (<= 601 + fragment + 4), 64 bytes of keys and table, and per band round
(2 * band + 1) * fragment bytes of direction codes: about 12 KiB a pair, 3 GiB for the default."""
import ctypes as ct
import gzip
import io
import json
import os
import sys

import numpy as np

from . import _ffi, candidates, clair_tensor, ingest
from ._ffi import check as _check, ptr as _p

FILTER_FLAG = 1796          # mpileup's default --ff: UNMAP, SECONDARY, QCFAIL, DUP (supplementary records are piled up)
WINDOW, REGION, FLANK, MAXCNT, MASK_WORDS, MAX_KEYS = 200, 233, 300, 8000, 13, 4
LR_READ = np.dtype([('off', '<i8'), ('pos', '<i4'), ('reserved', '<i4')])          # mpn_lr_read
LR_PAIR = np.dtype([('site', '<i4'), ('read', '<i4')])                             # mpn_lr_pair
LR_KEY = np.dtype([('count', '<i4'), ('len', '<i4'), ('off', '<i8')])              # mpn_lr_key
WHY = {1: 'the record, its CIGAR or its bases pass the end of the record', 2: 'a CIGAR operation code above 8',
       3: 'an N or P operation inside the region of a site: mpileup\'s text makes the script drop the column, which is not modelled',
       4: 'a record without bases', 5: 'a base `=`', 6: 'the CIGAR runs past the bases'}
SSW_CHUNK_DEFAULT = 262144

_bound = False


def ssw_chunk():
    return max(1, int(os.environ.get('MPN_LR_SSW_CHUNK', SSW_CHUNK_DEFAULT)))


def _lib():
    global _bound
    lib = clair_tensor._lib()
    if not _bound:
        P, I64, I32 = ct.c_void_p, ct.c_int64, ct.c_int32
        lib.mpn_lr_depth_rule.argtypes = [I64, P, P, I32, P]
        lib.mpn_lr_columns.argtypes = [P, I64, I64, P, I64, P, I64, P, P, P, P, P, I64, P]
        lib.mpn_lr_fragments.argtypes = [P, I64, I64, P, I64, P, I64, P, P, P, P, P, P, P, I64, P, P]
        lib.mpn_lr_align_tally.argtypes = [I64, P, P, I64, P, P, P, P, P, I64, P, P, P, P, I64, P, I64, P, P]
        lib.mpn_ssw_align_resident.argtypes = [I32, P, P, P, P, P, P, P, I32, ct.c_int8, ct.c_uint8, ct.c_uint8, ct.c_uint8, ct.c_uint16, I32, P, P, P, I64,
                                               P, P, P]
        for f in (lib.mpn_lr_depth_rule, lib.mpn_lr_columns, lib.mpn_lr_fragments, lib.mpn_lr_align_tally, lib.mpn_ssw_align_resident):
            f.restype = I32
        lib.mpn_lr_last_device_ms.argtypes = [ct.POINTER(ct.c_double)] * 4
        lib.mpn_lr_last_device_ms.restype = None
        _bound = True
    return lib


def last_device_ms():
    """-> (columns ms, fragments ms, SSW ms, tally ms) of the calling thread's last native calls"""
    return _ffi.device_ms(_lib().mpn_lr_last_device_ms, 4)


# ---- the native calls ---------------------------------------------------------------------------------------------------------------
def depth_rule(start, end, maxcnt=MAXCNT):
    """mpn_lr_depth_rule -> a bool array: which candidates of one site (start ascending, end exclusive) are piled up"""
    start, end = np.ascontiguousarray(start, dtype=np.int64), np.ascontiguousarray(end, dtype=np.int64)
    keep = np.zeros(len(start), dtype=np.uint8)
    _check(_lib().mpn_lr_depth_rule(len(start), _p(start), _p(end), int(maxcnt), _p(keep)), 'mpn_lr_depth_rule')
    return keep.astype(bool)


def site_pairs(pos, end, sites, maxcnt=MAXCNT):
    """Membership: pos, end (exclusive; htslib's bam_endpos) of the records mpileup may take, in file order; sites: 1-based, ascending
    -> an LR_PAIR array sorted by site, then by record: the records that overlap the site's region pos - 233 .. pos + 234 by htslib's
    rule and pass samtools' -d rule."""
    pos, end, sites = np.asarray(pos, dtype=np.int64), np.asarray(end, dtype=np.int64), np.asarray(sites, dtype=np.int64)
    beg0, end0 = sites - REGION - 1, sites + REGION + 1
    reach = np.maximum.accumulate(end) if len(end) else end
    b = np.searchsorted(reach, beg0, side='right')
    e = np.maximum(np.searchsorted(pos, end0, side='left'), b)
    n = e - b
    total = int(n.sum())
    site = np.repeat(np.arange(len(sites), dtype=np.int64), n)
    read = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(n) - n, n) + np.repeat(b, n)
    over = end[read] > beg0[site]
    site, read = site[over], read[over]
    cand = np.bincount(site, minlength=len(sites)) if len(site) else np.zeros(len(sites), dtype=np.int64)
    keep = np.ones(len(site), dtype=bool)
    first = np.concatenate([[0], np.cumsum(cand)])
    for c in np.flatnonzero(cand >= maxcnt).tolist():             # (a loop over the deep sites, not over their reads)
        a, z = int(first[c]), int(first[c + 1])
        keep[a:z] = depth_rule(pos[read[a:z]], end[read[a:z]], maxcnt)
    out = np.zeros(int(keep.sum()), dtype=LR_PAIR)
    out['site'], out['read'] = site[keep], read[keep]
    return out


def columns(text, text_len, reads, sites, pairs):
    """mpn_lr_columns -> (mask: an (m, 13) int32 tensor on the device, bad pair or -1, why, the sites (indices) at which the script's
    parser raises)"""
    import torch
    reads, pairs = np.ascontiguousarray(reads, dtype=LR_READ), np.ascontiguousarray(pairs, dtype=LR_PAIR)
    sites = np.ascontiguousarray(sites, dtype=np.int32)
    mask = torch.zeros((max(len(sites), 1), MASK_WORDS), dtype=torch.int32, device=text.device)
    bad, why, n_hz, cap = ct.c_int64(-1), ct.c_int32(0), ct.c_int64(0), 1024
    torch.cuda.current_stream(text.device).synchronize()          # the native layer uses the default stream
    while True:
        hazards = np.zeros((cap, 3), dtype=np.int64)
        mask.zero_()
        rc = _lib().mpn_lr_columns(text.data_ptr(), int(text_len), len(reads), _p(reads), len(sites), _p(sites), len(pairs), _p(pairs), mask.data_ptr(),
                                   ct.byref(bad), ct.byref(why), _p(hazards), cap, ct.byref(n_hz))
        if rc == -3 and n_hz.value > cap:
            cap = int(n_hz.value)
            continue
        _check(rc, 'mpn_lr_columns')
        break
    hazards = hazards[:n_hz.value]
    raising = np.unique(pairs['site'][hazards[hazards[:, 2] != 0, 0]]) if len(hazards) else np.zeros(0, dtype=np.int32)
    return mask[:len(sites)], bad.value, why.value, raising


def fragment_lengths(text, text_len, reads, sites, pairs, mask):
    """mpn_lr_fragments, the count pass -> (len, first column, bad pair or -1, why)"""
    reads, pairs = np.ascontiguousarray(reads, dtype=LR_READ), np.ascontiguousarray(pairs, dtype=LR_PAIR)
    sites = np.ascontiguousarray(sites, dtype=np.int32)
    length, first = np.zeros(len(pairs), dtype=np.int32), np.zeros(len(pairs), dtype=np.int32)
    bad, why = ct.c_int64(-1), ct.c_int32(0)
    _check(_lib().mpn_lr_fragments(text.data_ptr(), int(text_len), len(reads), _p(reads), len(sites), _p(sites), len(pairs), _p(pairs), mask.data_ptr(),
                                   _p(length), _p(first), None, None, None, 0, ct.byref(bad), ct.byref(why)), 'mpn_lr_fragments')
    return length, first, bad.value, why.value


def fragment_bytes(text, text_len, reads, sites, pairs, mask, length):
    """mpn_lr_fragments, the fill pass -> (offsets, letters and codes: uint8 / int8 tensors on the device)"""
    import torch
    reads, pairs = np.ascontiguousarray(reads, dtype=LR_READ), np.ascontiguousarray(pairs, dtype=LR_PAIR)
    sites, length = np.ascontiguousarray(sites, dtype=np.int32), np.ascontiguousarray(length, dtype=np.int32)
    off = np.zeros(len(pairs), dtype=np.int64)
    off[1:] = np.cumsum(length[:-1], dtype=np.int64)
    cap = int(length.sum(dtype=np.int64))
    letters = torch.zeros(max(cap, 1), dtype=torch.uint8, device=text.device)
    codes = torch.zeros(max(cap, 1), dtype=torch.int8, device=text.device)
    bad, why = ct.c_int64(-1), ct.c_int32(0)
    torch.cuda.current_stream(text.device).synchronize()
    _check(_lib().mpn_lr_fragments(text.data_ptr(), int(text_len), len(reads), _p(reads), len(sites), _p(sites), len(pairs), _p(pairs), mask.data_ptr(),
                                   _p(length), None, _p(off), letters.data_ptr(), codes.data_ptr(), cap, ct.byref(bad), ct.byref(why)), 'mpn_lr_fragments')
    if bad.value >= 0:
        raise _ffi.MpnError('mpn_lr_fragments: the fill pass refuses a pair that the count pass took')
    return off, letters, codes


def align_tally(sites, pair_begin, frag_off, frag_len, letters, codes, contig):
    """mpn_lr_align_tally -> (depth, raises, key_begin, keys: an LR_KEY array, their bytes; the last two read back from the device)"""
    import torch
    sites = np.ascontiguousarray(sites, dtype=np.int32)
    pair_begin, frag_off = np.ascontiguousarray(pair_begin, dtype=np.int64), np.ascontiguousarray(frag_off, dtype=np.int64)
    frag_len = np.ascontiguousarray(frag_len, dtype=np.int32)
    m, n = len(sites), len(frag_len)
    keys_cap = max(MAX_KEYS * n, 1)
    bytes_cap = max(int(frag_len.sum(dtype=np.int64)) + n * (2 * FLANK + 8), 1)
    d_keys = torch.zeros(keys_cap * LR_KEY.itemsize, dtype=torch.uint8, device=contig.device)
    d_bytes = torch.zeros(bytes_cap, dtype=torch.uint8, device=contig.device)
    depth, raises, key_begin = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32), np.zeros(m + 1, dtype=np.int64)
    bad, why = ct.c_int64(-1), ct.c_int32(0)
    torch.cuda.current_stream(contig.device).synchronize()
    _check(_lib().mpn_lr_align_tally(m, _p(sites), _p(pair_begin), n, _p(frag_off), _p(frag_len), letters.data_ptr(), codes.data_ptr(), contig.data_ptr(),
                                     contig.numel(), _p(depth), _p(raises), _p(key_begin), d_keys.data_ptr(), keys_cap, d_bytes.data_ptr(), bytes_cap,
                                     ct.byref(bad), ct.byref(why)), 'mpn_lr_align_tally')
    if bad.value >= 0:
        raise ValueError(f'position {int(sites[np.searchsorted(pair_begin, bad.value, side="right") - 1])}: SSW refuses a fragment (status {why.value}, '
                         'include/mpn_ssw.h): it is longer than 131072 bases, or its traceback needs a band wider than this library takes (an indel of '
                         'about 4 kb against the window); ssw.c has a result there, this library does not')
    k = int(key_begin[-1])
    keys = np.frombuffer(d_keys[:k * LR_KEY.itemsize].cpu().numpy().tobytes(), dtype=LR_KEY)
    used = int((keys['off'] + keys['len']).max()) if k else 0
    return depth, raises, key_begin, keys, d_bytes[:used].cpu().numpy().tobytes()


# ---- the sites of a file --------------------------------------------------------------------------------------------------------------
def _site_chunks(n_per_site, limit):
    """ranges of sites [a, b) whose pairs together stay within `limit` (a single site may pass it)"""
    a, total = 0, 0
    for c, n in enumerate(n_per_site.tolist()):
        if c > a and total + n > limit:
            yield a, c
            a, total = c, 0
        total += n
    if a < len(n_per_site):
        yield a, len(n_per_site)


def _sites_of_text(bam_fn, text, text_len, rows, reads, pos, end, fin, contig, result, timings):
    """the sites `fin` (1-based, ascending) whose records all lie in this text"""
    import time
    t0 = time.perf_counter()
    pairs = site_pairs(pos, end, fin)
    paired = np.flatnonzero((rows['flag'][pairs['read']] & 1) != 0)
    if len(paired):
        raise ValueError(f'{bam_fn}: record {candidates._record_name(text, rows[int(pairs["read"][paired[0]])])}: a paired read (FLAG bit 1): mpileup drops '
                         'orphans and merges overlapping mates, which is not taken')
    ingest._tick(timings, 'membership', time.perf_counter() - t0)

    def refuse(bad, why):
        if bad >= 0:
            raise ValueError(f'{bam_fn}: record {candidates._record_name(text, rows[int(pairs["read"][bad])])}: {WHY.get(why, why)}')
    t1 = time.perf_counter()
    mask, bad, why, raising = columns(text, text_len, reads, fin, pairs)
    ingest._tick(timings, 'columns_device_ms', last_device_ms()[0])
    refuse(bad, why)
    parser_raises = set(raising.tolist())
    length, first, bad, why = fragment_lengths(text, text_len, reads, fin, pairs, mask)
    ingest._tick(timings, 'fragments_device_ms', last_device_ms()[1])
    refuse(bad, why)
    has = length > 0                                           # a read with an empty fragment is not a read of the site
    pairs, length, first = pairs[has], length[has], first[has]
    order = np.lexsort((pairs['read'], first, pairs['site']))  # the script's dict: by first contributing column, then file order
    pairs, length = pairs[order], length[order]
    per_site = np.bincount(pairs['site'], minlength=len(fin)) if len(pairs) else np.zeros(len(fin), dtype=np.int64)
    begin = np.concatenate([[0], np.cumsum(per_site)]).astype(np.int64)
    ingest._tick(timings, 'fragments', time.perf_counter() - t1)
    for a, b in _site_chunks(per_site, ssw_chunk()):
        t2 = time.perf_counter()
        lo, hi = int(begin[a]), int(begin[b])
        off, letters, codes = fragment_bytes(text, text_len, reads, fin, pairs[lo:hi], mask, length[lo:hi])
        ingest._tick(timings, 'fragments_device_ms', last_device_ms()[1])
        t3 = time.perf_counter()
        depth, raises, key_begin, keys, text_of = align_tally(fin[a:b], begin[a:b + 1] - lo, off, length[lo:hi], letters, codes, contig)
        ms = last_device_ms()
        ingest._tick(timings, 'ssw_device_ms', ms[2])
        ingest._tick(timings, 'tally_device_ms', ms[3])
        t4 = time.perf_counter()
        for c in range(b - a):
            if raises[c] or (a + c) in parser_raises:
                result[int(fin[a + c])] = 'parser' if (a + c) in parser_raises else 'score'
                continue
            ks = keys[int(key_begin[c]):int(key_begin[c + 1])]
            result[int(fin[a + c])] = (int(depth[c]), {text_of[int(k['off']):int(k['off']) + int(k['len'])].decode(): int(k['count']) for k in ks})
        for key, dt in (('fragments', t3 - t2), ('ssw_tally', t4 - t3), ('host_text', time.perf_counter() - t4)):
            ingest._tick(timings, key, dt)
        if timings is not None:
            timings['pairs'] = timings.get('pairs', 0) + hi - lo


def alt_info(bam_fn, ref_fn, ctg_name, positions, device='cuda', timings=None):
    """The depth and the ordered {allele: count} mapping of local_realignment.py for every 1-based position (deduplicated and sorted
    here) -> {position: (depth, mapping)} in ascending order.  The contig's own base at the position is not in the mapping, as the
    script deletes it.  Left out, with a message on standard error: a position <= 300 (the script slices its reference with a
    negative index there), one behind the contig's end, and one at which the script raises: its first read has SSW score 0, or a row of its
    pile-up begins with a read whose base is not one of ACGTN and has an indel behind it (decode_pileup_bases raises IndexError).
    ValueError names the record: unsorted records, and among the records of a site's region a paired one, one with an N or P
    operation, an operation code above 8, no bases, a base `=`, or a CIGAR that runs past its bases."""
    import torch
    device = device or 'cuda'
    _lib()
    seq = candidates.read_contig(ref_fn, ctg_name)
    if not seq:
        raise ValueError(f'{ref_fn}: no contig {ctg_name}')
    sites = np.unique(np.asarray(list(positions), dtype=np.int64).reshape(-1))
    for p in sites[(sites <= FLANK) | (sites > len(seq))].tolist():
        print(f'{ctg_name}:{p}: left out: ' + ('the reference script slices its reference window with a negative index at positions up to 300'
                                               if p <= FLANK else 'behind the end of the contig'), file=sys.stderr)
    sites = sites[(sites > FLANK) & (sites <= len(seq))]
    contig = torch.from_numpy(np.frombuffer(bytes(seq), dtype=np.uint8).copy()).to(device)
    tid, _ = candidates.contig_tid(bam_fn, ctg_name)
    next_site, last_pos, result = 0, None, {}
    with ingest.BamTexts(bam_fn, device, timings) as texts:
        while next_site < len(sites):
            t = next(texts)
            text, text_len, final = t.text, t.text_len, t.final
            keep, pos, rlen, last_pos = clair_tensor.contig_reads(t, tid, last_pos, f'{bam_fn}: the records of {ctg_name} are not sorted by position',
                                                                  FILTER_FLAG)
            rows, end = t.rows[keep], pos + np.maximum(rlen, 1)
            todo = sites[next_site:]
            # a site is complete when a record starts behind its region (0-based: at site + 234 or later)
            n_fin = len(todo) if final else (int(np.searchsorted(todo, int(pos[-1]) - REGION - 1, side='right')) if len(pos) else 0)
            if n_fin:
                reads = np.zeros(len(rows), dtype=LR_READ)
                reads['off'], reads['pos'] = rows['off'], pos
                _sites_of_text(bam_fn, text, text_len, rows, reads, pos, end, todo[:n_fin], contig, result, timings)
                next_site += n_fin
            if final:
                break
            cut = len(t.rows)
            if next_site < len(sites) and len(pos):
                reach = np.maximum.accumulate(end)
                b = int(np.searchsorted(reach, int(sites[next_site]) - REGION - 1, side='right'))
                if b < len(keep):
                    cut = int(keep[b])
                    last_pos = int(pos[b])                # the next text starts again at this record
            texts.keep_from(cut)
    out = {}
    for p in sites.tolist():
        got = result.get(p, (0, {}))                       # (the file ended before the site: no read reaches it)
        if isinstance(got, str):
            print(f'{ctg_name}:{p}: left out: the reference script raises there (' + ('the first read of the site has SSW score 0' if got == 'score' else
                  'a row of the pile-up begins with a base that is not one of ACGTN and an indel behind it') + ')', file=sys.stderr)
            continue
        depth, mapping = got
        mapping.pop(chr(seq[p - 1]).upper(), None)
        out[p] = (depth, mapping)
    return out


def format_line(ctg_name, pos, depth, mapping):
    return '\t'.join([ctg_name, str(pos), str(depth), json.dumps(mapping), str(pos)]) + '\n'


def local_realignment(bam_fn, ref_fn, ctg_name, positions, out, device='cuda', timings=None):
    """Writes the script's lines `ctg\\tpos\\tdepth\\t<json>\\tpos`, one per site in ascending position, to `out` (a binary stream)
    -> the number of lines"""
    info = alt_info(bam_fn, ref_fn, ctg_name, positions, device=device, timings=timings)
    out.write(''.join(format_line(ctg_name, p, d, m) for p, (d, m) in info.items()).encode())
    return len(info)


# ---- extract_vcf_position.py ----------------------------------------------------------------------------------------------------------
def decode_alt(alt):
    """the lines of local_realignment (a path, or their text) -> {'ctg pos': (depth, mapping)}"""
    if isinstance(alt, dict):
        return alt
    if isinstance(alt, bytes):
        text = alt.decode()
    else:
        with open(alt) as f:
            text = f.read()
    out = {}
    for line in text.rstrip().split('\n'):
        f = line.rstrip().split('\t')
        if len(f) < 4:
            raise ValueError('[ERROR] Index error: a line of the allele file has fewer than four columns')
        out[f[0] + ' ' + str(int(f[1]))] = (int(f[2]), json.loads(f[3]))
    return out


def find_af(depth, mapping, ref_base, alt_base):
    count = 0
    if len(ref_base) == len(alt_base) == 1:
        count = int(mapping.get(alt_base, 0))
    elif len(ref_base) < len(alt_base):
        count = int(mapping.get('I' + alt_base[1:], 0))
    elif len(ref_base) > len(alt_base):
        count = int(mapping.get('D' + ref_base[1:], 0))
    return count / float(depth) if count > 0 else None


def extract_vcf_position(vcf_fn, alt, output_fn, keep=None, said=None):
    """ExtractVcfPosition: vcf_fn (gzip or plain), alt (the path of the lines of local_realignment, their bytes, or decode_alt's
    mapping) -> output_fn: the header, then the rows whose `CHROM POS` has a line: with GT:GQ:<DP>:<%.4f AF> when find_AF gives a
    positive value, unchanged otherwise.  As in the script a row without a line is not written, unless keep(chrom, pos) says so
    (bin/mpn-local-realign keeps the rows of other contigs).  Rows are joined by a newline without a final one.  The `[INFO]` lines go to
    `said` (default: standard output).  ValueError for a matched row whose last column has not the four fields GT:GQ:DP:AF."""
    said = sys.stdout if said is None else said
    alts = decode_alt(alt)
    with open(vcf_fn, 'rb') as f:
        raw = f.read()
    text = (gzip.decompress(raw) if raw[:2] == b'\x1f\x8b' else raw).decode()
    head, body = [], []
    for row in text.splitlines():
        row = row.rstrip()
        if not row:
            continue
        if row[0] == '#':
            head.append(row)
            continue
        col = row.strip().split('\t')
        key = col[0] + ' ' + str(int(col[1]))
        if key not in alts:
            if keep is not None and keep(col[0], int(col[1])):
                body.append(row)
            continue
        field = col[-1].split(':')
        if len(field) != 4:
            raise ValueError(f'{vcf_fn}: {col[0]}:{col[1]}: the last column is not GT:GQ:DP:AF')
        dp, mapping = alts[key]
        af = find_af(dp, mapping, col[3], col[4])
        if af and af > 0:
            print('[INFO] {}:{} updates allele frequency to {}'.format(col[0], int(col[1]), round(af, 4)), file=said)
            row = '\t'.join(col[:-1] + ['%s:%s:%d:%.4f' % (field[0], field[1], dp, af)])
        body.append(row)
    with open(output_fn, 'w') as f:
        f.write('\n'.join(head + body))


def vcf_positions(vcf_fn, ctg_name):
    """the POS of the rows of ctg_name"""
    with open(vcf_fn, 'rb') as f:
        raw = f.read()
    text = (gzip.decompress(raw) if raw[:2] == b'\x1f\x8b' else raw).decode()
    return [int(r.split('\t')[1]) for r in text.splitlines() if r.strip() and r[0] != '#' and r.split('\t')[0] == ctg_name]


def main(argv, prog='mpn-local-realign'):
    """The command line of realignment/realignment.sh."""
    from argparse import ArgumentParser
    ap = ArgumentParser(prog=prog, description='Realign reads around the positions of a VCF and update its DP and AF (on the GPU)')
    ap.add_argument('-b', dest='bam', required=True, help='sorted BAM file')
    ap.add_argument('-v', dest='vcf', required=True, help='VCF of the caller, gzip or plain')
    ap.add_argument('-r', dest='ref', required=True, help='reference FASTA, plain or gzip (no .fai is needed)')
    ap.add_argument('-c', dest='contig', required=True, help='the contig')
    ap.add_argument('-p', dest='platform', default='ont', help='ont; illumina is refused')
    ap.add_argument('-o', dest='out', required=True, help='output folder: tmp/0_all_alt_info and 0_realign.vcf')
    ap.add_argument('-t', dest='threads', type=int, default=1, help='accepted and ignored: one process does all sites')
    if not argv:
        ap.print_help()
        return 1
    a = ap.parse_args(argv)
    if a.platform != 'ont':
        print(f'{prog}: -p {a.platform}: only the ont path is taken (the Illumina path realigns the reads with a de Bruijn graph first)', file=sys.stderr)
        return 2
    try:
        os.makedirs(os.path.join(a.out, 'tmp'), exist_ok=True)
        alt_fn = os.path.join(a.out, 'tmp', '0_all_alt_info')
        buf = io.BytesIO()
        local_realignment(a.bam, a.ref, a.contig, vcf_positions(a.vcf, a.contig), buf)
        with open(alt_fn, 'wb') as f:
            f.write(buf.getvalue())
        # (no position of the contig gave a line: the rows of other contigs still pass through)
        extract_vcf_position(a.vcf, alt_fn if buf.getvalue() else {}, os.path.join(a.out, '0_realign.vcf'), keep=lambda ctg, pos: ctg != a.contig)
    except (ValueError, OSError) as e:
        print(f'{prog}: {e}', file=sys.stderr)
        return 1
    return 0
