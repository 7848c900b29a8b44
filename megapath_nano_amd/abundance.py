"""Per-assembly abundance statistic over an alignment table.

Reference: `align_list_to_align_stat_by_assembly_id` (/root/reference/bin/megapath_nano.py:485-541) with its helpers
`summary_stat_1` (:440-449), `align_list_to_bed` (:313-330: bedtools sort + merge of (assembly, sequence) intervals),
`bed_to_covered_bp_by_assembly_id` (:333-347) and `summary_stat_2` (:451-482), including the noise-BED branch
(`covered_bed.subtract(noise_bed)` and `noise_span_bp`, :516-541; the noise filters that produce such a BED are off by default,
megapath_nano.py:4985-4996).

Steps: per (read, assembly) keep the alignment with the largest (alignment_score, tiebreaker); sum per assembly; covered bp
= length of the union of the kept alignments' target intervals per (assembly, sequence), where overlapping AND
book-ended intervals merge (`bedtools merge` default distance 0), minus what a noise BED covers; then the derived columns of
summary_stat_2, with the reference's inf -> nan -> 0 clean-up and the rounded `adjusted_total_aligned_bp`.

The interval union runs on the GPU (include/mpn_abundance.h: mpn_cover_by_group -- a radix sort and a segmented sweep;
`device=True`, the default when libmpn.so can reach a GPU); the numpy form below (`device=False`) is the host statement of
the same sums and is what the CPU tests pin against plain loops.  `device_sort_order` is the same sort behind
bam.sam_to_sorted_bam (`samtools sort`).

Depth: `align_list_to_depth_bed` (the reference's bin/megapath_nano.py:417-482: `bedtools genomecov -bg` over the target
intervals, a per-assembly depth threshold on the profile rows, `bedtools sort | merge` of the rows that pass and their summed
length per assembly) is the source of every depth-based noise BED: `step_spike_filter` (:1759-1806), the closing spike filter
(:2359), `step_variable_region` (:1729-1734).  Here it is mpn_depth_by_key (events, the same radix sort, two scans) behind
`depth_profile`, `align_list_to_depth_bed` and `spike_noise`; `host_depth_by_key` is its numpy statement.  bedtools is restated,
not run: DESIGN.md section 2 says what that restatement rests on.

Applying a noise BED: `select_alignment_by_bed` (the reference's :666-717: `bedtools annotate` of one row per alignment against
the BED, then a threshold on the covered fraction) behind `step_noise_removal` (:2259-2272) and `step_closing_spike_filter`
(:2353-2408), and `merge_bed_with_assembly_id` (:362-382: `bedtools sort | merge` of several BEDs on assembly_id + ',' +
sequence_id).  Here they are mpn_cover_by_bed (the BED merged on the device, then two binary searches per alignment) and
mpn_bed_union behind the functions of the same names, `noise_removal` and `closing_spike_filter`; `host_bed_union` and
`host_cover_by_bed` are the numpy statements.  The covered base pairs are exact integers from either; the fraction they are
compared through is bedtools' float32 quotient printed with six decimals, computed on the host.

The best alignment of every read: `align_list_to_best_align_list` (the reference's :244-310) keeps the best row per (read,
assembly), takes the rows that reach their read's largest score as candidates, and decides a read with several candidates by a
random draw weighted with the abundance of the candidates' assemblies among the reads that have one candidate only.  Behind it
are mpn_best_candidates (the radix sort by (read, assembly), segmented scans) and mpn_pick_weighted; mpn_second_best_by_read is the
device half of `unique_alignment` (step_unique_alignment, :2553-2593).  `short_alignment_removal` (:2293-2327), `closing_spike_step`
(:2330-2422 with its two draws) and `combine_with_human_and_decoy` (:2425-2446) complete the steps that stand on it.  The random
numbers come from the host, one `rng()` per candidate of a read with several, in the order of (read_id, assembly_id): the number
and order of the calls are the reference's.

From species to assemblies: `step_assembly_selection` (the reference's :1400-1476, on by default) is `assembly_selection`.  Under it
`good_align_list` (:642-663: the best row per (read, assembly), of those the rows that reach good_align_threshold percent of their
read's best score -- one float64 product, as pandas forms it), `best_align_per_read` (the sort_values / drop_duplicates idiom of
:1287 and :1459) and `align_stat_by_sequence_id` (:585-639) all stand on mpn_good_rows -- the same sort and scans as
mpn_best_candidates with another compaction -- and the grouped sums of summary_stat_1 (:485-493) on mpn_sum_by_key, a segmented scan
that carries a count and six sums and puts no atomic on its output; `host_good_rows` and `host_sum_by_key` are the numpy
statements.  The summed tiebreaker, the one float sum, is np.bincount on the host either way.
"""
import ctypes as ct
import math
import random

import numpy as np
import pandas

from . import _ffi

_bound = False


def _lib():
    global _bound
    lib = _ffi.lib()
    if not _bound:
        P = ct.c_void_p
        lib.mpn_sort_order.argtypes = [ct.c_int64, P, P, P]
        lib.mpn_sort_order.restype = ct.c_int
        lib.mpn_cover_by_group.argtypes = [ct.c_int64, P, P, P, P, ct.c_int32, P]
        lib.mpn_cover_by_group.restype = ct.c_int
        lib.mpn_depth_by_key.argtypes = [ct.c_int64, P, P, P, ct.c_int32, P, P, ct.c_int32, P, P, ct.c_int64, P, P, P, P, P, P, P, P, P, P]
        lib.mpn_depth_by_key.restype = ct.c_int
        lib.mpn_bed_union.argtypes = [ct.c_int64, P, P, P, ct.c_int32, P, ct.c_int32, ct.c_int64, P, P, P, P, P]
        lib.mpn_bed_union.restype = ct.c_int
        lib.mpn_cover_by_bed.argtypes = [ct.c_int64, P, P, P, ct.c_int64, P, P, P, ct.c_int32, P]
        lib.mpn_cover_by_bed.restype = ct.c_int
        lib.mpn_best_candidates.argtypes = [ct.c_int64, P, P, P, P, ct.c_int32, ct.c_int32, P, P, P, P, P]
        lib.mpn_best_candidates.restype = ct.c_int
        lib.mpn_pick_weighted.argtypes = [ct.c_int64, P, P, P, P, ct.c_int32, P, P]
        lib.mpn_pick_weighted.restype = ct.c_int
        lib.mpn_second_best_by_read.argtypes = [ct.c_int64, P, P, P, ct.c_int32, P, P]
        lib.mpn_second_best_by_read.restype = ct.c_int
        lib.mpn_good_rows.argtypes = [ct.c_int64, P, P, P, P, ct.c_int32, ct.c_int32, ct.c_int32, ct.c_double, P, P, P]
        lib.mpn_good_rows.restype = ct.c_int
        lib.mpn_sum_by_key.argtypes = [ct.c_int64, P, ct.c_int32, ct.c_int32, P, P, P]
        lib.mpn_sum_by_key.restype = ct.c_int
        _bound = True
    return lib


def device_sort_order(tid_key, pos, rev):
    """Order of BAM records by (reference, position, strand), ties in input order: the GPU form of `samtools sort`
    (bam.sam_to_sorted_bam's sort_keys hook).  tid_key < 2^41, 0 <= pos < 2^62, rev in {0, 1}."""
    tid_key = np.ascontiguousarray(tid_key, dtype=np.uint64)
    lo = np.ascontiguousarray(np.asarray(pos, dtype=np.uint64) << np.uint64(1) | np.asarray(rev, dtype=np.uint64))
    order = np.empty(len(tid_key), dtype=np.int64)
    _ffi.check(_lib().mpn_sort_order(len(tid_key), tid_key.ctypes.data, lo.ctypes.data, order.ctypes.data), 'mpn_sort_order')
    return order


def device_cover_by_group(group, seq, start, end, n_groups):
    """-> int64[n_groups]: union length of [start, end) per (group, seq), summed per group (mpn_cover_by_group)."""
    group = np.ascontiguousarray(group, dtype=np.int32)
    seq = np.ascontiguousarray(seq, dtype=np.int32)
    start = np.ascontiguousarray(start, dtype=np.int64)
    end = np.ascontiguousarray(end, dtype=np.int64)
    out = np.zeros(max(int(n_groups), 1), dtype=np.int64)
    _ffi.check(_lib().mpn_cover_by_group(len(group), group.ctypes.data, seq.ctypes.data, start.ctypes.data, end.ctypes.data, int(n_groups),
                                         out.ctypes.data), 'mpn_cover_by_group')
    return out[:n_groups]


def _codes(col):
    u, inv = np.unique(col.to_numpy(dtype=object).astype(str), return_inverse=True)
    return u, inv


def best_per_read_and_assembly(align_list):
    _, rc = _codes(align_list['read_id'])
    _, ac = _codes(align_list['assembly_id'])
    order = np.lexsort((align_list['alignment_score_tiebreaker'].to_numpy(), align_list['alignment_score'].to_numpy(), ac, rc))
    last = np.ones(len(order), dtype=bool)
    last[:-1] = (rc[order][1:] != rc[order][:-1]) | (ac[order][1:] != ac[order][:-1])
    return align_list.iloc[order[last]]


def host_cover_by_group(ac, sc, start, end, n_groups):
    """numpy statement of mpn_cover_by_group (one global running maximum serves all groups)."""
    if len(ac) == 0:
        return np.zeros(n_groups, dtype=np.int64)
    order = np.lexsort((end, start, sc, ac))
    ac, sc, start, end = ac[order], sc[order], start[order], end[order]
    new_group = np.ones(len(order), dtype=bool)
    new_group[1:] = (ac[1:] != ac[:-1]) | (sc[1:] != sc[:-1])
    gid = np.cumsum(new_group) - 1
    span = int(end.max() - min(start.min(), 0)) + 2
    run_end = np.maximum.accumulate(end + gid * span) - gid * span
    prev_end = np.empty_like(run_end)
    prev_end[0] = 0
    prev_end[1:] = run_end[:-1]
    opens = new_group | (start > prev_end)                      # book-ended intervals (start == previous end) merge
    add = np.where(opens, end - start, np.maximum(end - np.maximum(prev_end, start), 0))
    return np.bincount(ac, weights=add.astype(np.float64), minlength=n_groups).astype(np.int64)


def covered_bp_by_assembly(rows, noise_bed=None, device=None):
    r"""Union length of [sequence_from, sequence_to) per (assembly_id, sequence_id), summed per assembly.
    noise_bed: DataFrame(sequence_id, start, end[, assembly_id]) -- what it covers on a sequence is subtracted
    (`covered_bed.subtract(noise_bed)`, megapath_nano.py:516-518): |A \ N| = |A u N| - |N| per sequence.
    device: None / True = the HIP path (libmpn.so and a GPU are REQUIRED: like every product path of this package it raises
    MpnError without them, there is no silent fallback); False = the numpy restatement the tests compare it with."""
    if rows.shape[0] == 0:
        return {}
    if device is None:
        device = True
    cover = device_cover_by_group if device else host_cover_by_group
    asm, ac = _codes(rows['assembly_id'])
    seqs, sc = _codes(rows['sequence_id'])
    start, end = rows['sequence_from'].to_numpy(dtype=np.int64), rows['sequence_to'].to_numpy(dtype=np.int64)
    ac, sc = ac.astype(np.int32), sc.astype(np.int32)
    if noise_bed is None or noise_bed.shape[0] == 0:
        return dict(zip(asm, cover(ac, sc, start, end, len(asm))))
    # noise intervals on the sequences that carry alignments, once under every assembly that has alignments on that sequence
    # (bedtools subtract matches on the chromosome column alone, which is the sequence_id)
    where = pandas.Index(seqs).get_indexer(noise_bed['sequence_id'].astype(str))
    hit = where >= 0
    pairs = pandas.DataFrame({'ac': ac, 'sc': sc}).drop_duplicates()
    nz = pandas.DataFrame({'sc': where[hit].astype(np.int32), 'start': noise_bed['start'].to_numpy(dtype=np.int64)[hit],
                           'end': noise_bed['end'].to_numpy(dtype=np.int64)[hit]}).merge(pairs, on='sc', how='inner')
    n_ac, n_sc = nz['ac'].to_numpy(dtype=np.int32), nz['sc'].to_numpy(dtype=np.int32)
    n_start, n_end = nz['start'].to_numpy(dtype=np.int64), nz['end'].to_numpy(dtype=np.int64)
    both = cover(np.concatenate([ac, n_ac]), np.concatenate([sc, n_sc]), np.concatenate([start, n_start]), np.concatenate([end, n_end]), len(asm))
    noise = cover(n_ac, n_sc, n_start, n_end, len(asm))
    return dict(zip(asm, both - noise))


def _float_sums(code, n, cols):
    """count and integer sums per code through np.bincount (float64 additions: exact while the sums stay below 2^53)"""
    return (np.bincount(code, minlength=n).astype(np.int64),
            [np.bincount(code, weights=np.asarray(v, dtype=np.float64), minlength=n).astype(np.int64) for v in cols])


def _summary_stat_1(best, code, n, sums):
    """The grouped sums of the reference's summary_stat_1 (megapath_nano.py:485-493) as columns, in its order.  sums(code, n,
    cols) -> count, [sum per column]: _float_sums, or mpn_sum_by_key / its host statement.  The summed tiebreaker, the one float
    sum, is always np.bincount over the rows in their order."""
    aligned = (best['sequence_to'] - best['sequence_from']).to_numpy()
    count, (read_bp, aligned_bp, match, edit_dist, score) = sums(code, n, [best['read_length'], aligned, best['match'], best['edit_dist'],
                                                                           best['alignment_score']])
    return {
        'total_number_of_read': count,
        'total_read_bp': read_bp,
        'total_aligned_bp': aligned_bp,
        'match': match,
        'edit_dist': edit_dist,
        'alignment_score': score,
        'alignment_score_tiebreaker': np.bincount(code, weights=np.asarray(best['alignment_score_tiebreaker'], dtype=np.float64), minlength=n),
    }


def _summary_stat_2(out, length_col):
    """The derived columns of the reference's summary_stat_2 (megapath_nano.py:495-518) added to `out`, which has the sums,
    `length_col`, covered_bp and noise_span_bp."""
    L = out[length_col].to_numpy(dtype=np.float64)
    noise = out['noise_span_bp'].to_numpy(dtype=np.float64)
    tab = out['total_aligned_bp'].to_numpy(dtype=np.float64)

    def clean(x):
        x = np.asarray(x, dtype=np.float64)
        return np.where(np.isfinite(x), x, 0.0)

    with np.errstate(divide='ignore', invalid='ignore'):
        out['average_read_length'] = clean(out['total_read_bp'] / out['total_number_of_read'])
        out['average_depth'] = clean(tab / L)
        out['covered_percent'] = clean(out['covered_bp'] / L)
        out['noise_span_percent'] = clean(noise / L)
        acp = clean(out['covered_bp'] / (L - noise))
        out['adjusted_covered_percent'] = acp
        out['average_identity'] = clean(out['match'] / tab)
        out['average_edit_dist'] = clean(out['edit_dist'] / tab)
        out['average_alignment_score'] = clean(out['alignment_score'] / tab)
        # the reference cleans inf/nan AFTER this block of columns and again after the next one
        aad = acp * tab / (L - noise)
        out['adjusted_average_depth'] = aad
        out['adjusted_total_aligned_bp'] = np.round(clean(aad * L), 0).astype(np.int64)
        out['adjusted_average_depth'] = clean(aad)
    return out


def _stat_of_best_rows(best, assembly_length, assembly_tax, noise_bed, device, sums):
    """align_stat_by_assembly_id from the best rows per (read, assembly), listed in (read_id, assembly_id) order"""
    asm, ac = _codes(best['assembly_id'])
    n = len(asm)
    out = pandas.DataFrame({'assembly_id': asm, **_summary_stat_1(best, ac, n, sums)})
    length = dict(zip(assembly_length['assembly_id'], assembly_length['assembly_length']))
    out['assembly_length'] = np.array([int(length.get(a, 0)) for a in asm], dtype=np.int64)
    for col in ('tax_id', 'species_tax_id', 'genus_tax_id', 'genus_height'):
        lut = dict(zip(assembly_tax['assembly_id'], assembly_tax[col])) if assembly_tax is not None and col in assembly_tax else {}
        out[col] = np.array([int(lut.get(a, 0)) for a in asm], dtype=np.int64)
    cov = covered_bp_by_assembly(best, noise_bed=noise_bed, device=device)
    out['covered_bp'] = np.array([int(cov.get(a, 0)) for a in asm], dtype=np.int64)
    out['noise_span_bp'] = 0
    if noise_bed is not None and noise_bed.shape[0]:
        # bed_to_covered_bp_by_assembly_id(noise_bed): the plain sum of the noise intervals' lengths per assembly (:523-533)
        span = (noise_bed['end'] - noise_bed['start']).groupby(noise_bed['assembly_id'].astype(str)).sum()
        out['noise_span_bp'] = np.array([int(span.get(a, 0)) for a in asm], dtype=np.int64)
    return _summary_stat_2(out, 'assembly_length')


def align_stat_by_assembly_id(align_list, assembly_length, assembly_tax=None, noise_bed=None, device=None):
    """align_list: the Align() table.  assembly_length: DataFrame(assembly_id, assembly_length); assembly_tax (optional):
    DataFrame(assembly_id, tax_id, species_tax_id, genus_tax_id, genus_height); noise_bed (optional): DataFrame(sequence_id,
    start, end, assembly_id) as the reference's noise BEDs carry them (name column = assembly_id).  -> DataFrame, one row per
    assembly."""
    return _stat_of_best_rows(best_per_read_and_assembly(align_list), assembly_length, assembly_tax, noise_bed, device, _float_sums)


# ---- depth profile, depth BED, depth span -----------------------------------------------------------------------------------
DEPTH_TILE = 2048   # MPN_DEPTH_TILE of include/mpn_abundance.h: the events one block of the device sweep scans (the tests put
#                     their sizes around its multiples; tests/test_depth_bed.py checks that the two numbers agree)


def _depth_args(key, start, end, key_len, key_group, depth_lo, depth_hi):
    key = np.ascontiguousarray(key, dtype=np.int32)
    start = np.ascontiguousarray(start, dtype=np.int64)
    end = np.ascontiguousarray(end, dtype=np.int64)
    key_len = np.ascontiguousarray(key_len, dtype=np.int64)
    key_group = np.ascontiguousarray(key_group, dtype=np.int32)
    if (depth_lo is None) != (depth_hi is None):
        raise ValueError('depth_lo and depth_hi are given together or not at all')
    if depth_lo is not None:
        depth_lo, depth_hi = np.ascontiguousarray(depth_lo, dtype=np.int32), np.ascontiguousarray(depth_hi, dtype=np.int32)
    return key, start, end, key_len, key_group, depth_lo, depth_hi


def device_depth_by_key(key, start, end, key_len, key_group, n_groups, depth_lo=None, depth_hi=None):
    """mpn_depth_by_key.  Interval i = [start[i], end[i]) on key[i]; key k has length key_len[k] and group key_group[k];
    depth_lo / depth_hi: inclusive int32 depth range per group (both None: every row passes).
    -> (row_key, row_start, row_end, row_depth), (bed_key, bed_start, bed_end), span[n_groups]: the whole, unfiltered
    profile ordered by (key, start); the rows that pass with touching rows merged, in the same order; the summed length of the
    passing rows per group."""
    key, start, end, key_len, key_group, depth_lo, depth_hi = _depth_args(key, start, end, key_len, key_group, depth_lo, depth_hi)
    n, cap = len(key), max(2 * len(key), 1)
    rk, rs, re, rd = np.empty(cap, np.int32), np.empty(cap, np.int64), np.empty(cap, np.int64), np.empty(cap, np.int32)
    bk, bs, be = np.empty(cap, np.int32), np.empty(cap, np.int64), np.empty(cap, np.int64)
    n_rows, n_bed = ct.c_int64(0), ct.c_int64(0)
    span = np.zeros(max(int(n_groups), 1), dtype=np.int64)
    lo_p, hi_p = (None, None) if depth_lo is None else (depth_lo.ctypes.data, depth_hi.ctypes.data)
    _ffi.check(_lib().mpn_depth_by_key(n, key.ctypes.data, start.ctypes.data, end.ctypes.data, len(key_len), key_len.ctypes.data, key_group.ctypes.data,
                                       int(n_groups), lo_p, hi_p, cap, rk.ctypes.data, rs.ctypes.data, re.ctypes.data, rd.ctypes.data, ct.byref(n_rows),
                                       bk.ctypes.data, bs.ctypes.data, be.ctypes.data, ct.byref(n_bed), span.ctypes.data), 'mpn_depth_by_key')
    r, b = n_rows.value, n_bed.value
    return (rk[:r], rs[:r], re[:r], rd[:r]), (bk[:b], bs[:b], be[:b]), span[:n_groups]


def host_depth_by_key(key, start, end, key_len, key_group, n_groups, depth_lo=None, depth_hi=None):
    """numpy statement of mpn_depth_by_key (same arguments, same result): +1 / -1 events sorted by (key, position), the net
    change per position, positions without a change dropped, the depth as the running sum."""
    key, start, end, key_len, key_group, depth_lo, depth_hi = _depth_args(key, start, end, key_len, key_group, depth_lo, depth_hi)
    end = np.minimum(end, key_len[key]) if len(key) else end        # the clip; start >= key_len then has start >= end
    on = start < end
    key, start, end = key[on], start[on], end[on]
    ek, ep = np.concatenate([key, key]).astype(np.int64), np.concatenate([start, end])
    ed = np.concatenate([np.ones(len(key), dtype=np.int64), -np.ones(len(key), dtype=np.int64)])
    order = np.lexsort((ep, ek))
    ek, ep, ed = ek[order], ep[order], ed[order]
    first = np.ones(len(ek), dtype=bool)
    first[1:] = (ek[1:] != ek[:-1]) | (ep[1:] != ep[:-1])
    net = np.add.reduceat(ed, np.flatnonzero(first)) if len(ek) else ed
    change = net != 0                                             # equal-depth neighbours merge here
    pk, pp, depth = ek[first][change], ep[first][change], np.cumsum(net[change])
    opens = np.flatnonzero(depth > 0)                             # every key's events sum to 0: the next point is on the same key
    rk, rs, re, rd = pk[opens].astype(np.int32), pp[opens], pp[opens + 1] if len(opens) else pp[opens], depth[opens].astype(np.int32)
    g = key_group[rk]
    ok = np.ones(len(rk), dtype=bool) if depth_lo is None else (depth_lo[g] <= rd) & (rd <= depth_hi[g])
    span = np.bincount(g[ok], weights=(re - rs)[ok].astype(np.float64), minlength=int(n_groups)).astype(np.int64)[:n_groups]
    fk, fs, fe = rk[ok], rs[ok], re[ok]
    head = np.ones(len(fk), dtype=bool)
    head[1:] = (fk[1:] != fk[:-1]) | (fs[1:] != fe[:-1])         # passing rows never overlap: touching is all `merge` can meet
    tail = np.ones(len(fk), dtype=bool)
    tail[:-1] = head[1:]
    return (rk, rs, re, rd), (fk[head], fs[head], fe[tail]), span


def depth_bound(threshold, comparison):
    """The integer bound of a float depth threshold: comparison '<' -> hi = ceil(x) - 1, '<=' -> hi = floor(x),
    '>' -> lo = floor(x) + 1, '>=' -> lo = ceil(x); clamped to int32."""
    x = float(threshold)
    if math.isinf(x):
        v = x
    else:
        v = {'<': math.ceil(x) - 1, '<=': math.floor(x), '>': math.floor(x) + 1, '>=': math.ceil(x)}[comparison]
    return int(min(max(v, -2 ** 31), 2 ** 31 - 1))


def _depth_keys(align_list):
    """(assembly, sequence) pairs coded in the byte order of assembly_id + ',' + sequence_id (`bedtools sort` on that chrom
    column; numpy orders str by code point, which is the order of the UTF-8 bytes).
    -> key[n], key_asm[n_keys] (str), key_seq[n_keys] (str), key_len[n_keys], assemblies (sorted, unique), key_group[n_keys]"""
    asm = align_list['assembly_id'].to_numpy(dtype=object).astype(str)
    seq = align_list['sequence_id'].to_numpy(dtype=object).astype(str)
    code, pairs = pandas.MultiIndex.from_arrays([asm, seq]).factorize()
    p_asm = np.array([p[0] for p in pairs], dtype=object).astype(str)
    p_seq = np.array([p[1] for p in pairs], dtype=object).astype(str)
    order = np.argsort(np.char.add(np.char.add(p_asm, ','), p_seq), kind='stable')
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    key = rank[code]
    length = align_list['sequence_length'].to_numpy(dtype=np.int64)
    key_len = np.zeros(len(order), dtype=np.int64)
    key_len[key] = length
    if not np.array_equal(key_len[key], length):
        bad = int(key[np.flatnonzero(key_len[key] != length)[0]])
        raise ValueError(f'sequence_length differs within ({p_asm[order][bad]}, {p_seq[order][bad]})')
    assemblies, key_group = np.unique(p_asm[order], return_inverse=True)
    return key.astype(np.int32), p_asm[order], p_seq[order], key_len, assemblies, key_group.astype(np.int32)


def _depth_call(align_list, depth_lo, depth_hi, device):
    if device is None:
        device = True
    key, key_asm, key_seq, key_len, assemblies, key_group = _depth_keys(align_list)
    run = device_depth_by_key if device else host_depth_by_key
    out = run(key, align_list['sequence_from'].to_numpy(dtype=np.int64), align_list['sequence_to'].to_numpy(dtype=np.int64), key_len, key_group,
              len(assemblies), depth_lo(assemblies) if depth_lo else None, depth_hi(assemblies) if depth_hi else None)
    return out, key_asm, key_seq, assemblies


def depth_profile(align_list, device=None):
    """The bedGraph of the alignments' target intervals (`bedtools genomecov -bg`): DataFrame(assembly_id, sequence_id, start,
    end, depth), the maximal runs of constant non-zero depth, ordered like the depth BED.  align_list: assembly_id, sequence_id,
    sequence_from, sequence_to, sequence_length.  device: as in covered_bp_by_assembly."""
    cols = ['assembly_id', 'sequence_id', 'start', 'end', 'depth']
    if align_list.shape[0] == 0:
        return pandas.DataFrame({c: np.zeros(0, dtype=object if c.endswith('_id') else np.int64) for c in cols})
    ((rk, rs, re, rd), _, _), key_asm, key_seq, _ = _depth_call(align_list, None, None, device)
    return pandas.DataFrame({'assembly_id': key_asm[rk], 'sequence_id': key_seq[rk], 'start': rs, 'end': re, 'depth': rd.astype(np.int64)}, columns=cols)


def _bounds(table, column, assemblies, nan_value, comparison, absent):
    """int32 bound per assembly from a threshold table; an assembly the table lacks gets `absent` (it passes nothing: the
    reference merges the table with how='inner')."""
    ids = table['assembly_id'].astype(str).to_numpy()
    if len(set(ids)) != len(ids):
        raise ValueError(f'{column}: an assembly_id occurs twice')
    out = np.full(len(assemblies), absent, dtype=np.int64)
    where = pandas.Index(assemblies).get_indexer(ids)
    for w, x in zip(where, table[column].to_numpy(dtype=np.float64)):
        if w >= 0:
            out[w] = depth_bound(nan_value if np.isnan(x) else x, comparison)
    return out


def align_list_to_depth_bed(*, align_list, min_depth=None, can_equal_to_min=True, max_depth=None, can_equal_to_max=True, temp_dir_name=None,
                            device=None):
    """The reference's align_list_to_depth_bed with its keyword arguments (temp_dir_name is accepted and ignored).
    align_list: assembly_id, sequence_id, sequence_from, sequence_to, sequence_length (one length per (assembly, sequence):
    ValueError otherwise).  min_depth / max_depth: DataFrame(assembly_id, min_depth) / (assembly_id, max_depth), floats; NaN is
    -1 / 99999999; with a table given, an assembly it lacks passes nothing.
    -> depth_bed: DataFrame(sequence_id, start, end, assembly_id) ordered by the bytes of assembly_id + ',' + sequence_id, then
    start (what align_stat_by_assembly_id(noise_bed=...) takes); depth_span_bp: DataFrame(assembly_id, span_bp) of the
    assemblies with at least one passing row."""
    if align_list.shape[0] == 0:
        return (pandas.DataFrame({'sequence_id': np.zeros(0, dtype=object), 'start': np.zeros(0, dtype=np.int64), 'end': np.zeros(0, dtype=np.int64),
                                  'assembly_id': np.zeros(0, dtype=object)}),
                pandas.DataFrame({'assembly_id': np.zeros(0, dtype=object), 'span_bp': np.zeros(0, dtype=np.int64)}))
    lo = hi = None
    if min_depth is not None or max_depth is not None:
        # a table that is not given bounds nothing; an assembly absent from a given one gets an empty range from that side
        def lo(assemblies):
            if min_depth is None:
                return np.zeros(len(assemblies), dtype=np.int64)
            return _bounds(min_depth, 'min_depth', assemblies, -1, '>=' if can_equal_to_min else '>', 2 ** 31 - 1)

        def hi(assemblies):
            if max_depth is None:
                return np.full(len(assemblies), 2 ** 31 - 1, dtype=np.int64)
            return _bounds(max_depth, 'max_depth', assemblies, 99999999, '<=' if can_equal_to_max else '<', 0)
    (_, (bk, bs, be), span), key_asm, key_seq, assemblies = _depth_call(align_list, lo, hi, device)
    depth_bed = pandas.DataFrame({'sequence_id': key_seq[bk], 'start': bs, 'end': be, 'assembly_id': key_asm[bk]},
                                 columns=['sequence_id', 'start', 'end', 'assembly_id'])
    has = span > 0                                                # a passing row is never empty
    return depth_bed, pandas.DataFrame({'assembly_id': assemblies[has], 'span_bp': span[has]}, columns=['assembly_id', 'span_bp'])


def spike_noise(align_list, assembly_length, expected_max_depth_stdev=6, assembly_tax=None, device=None):
    """step_spike_filter's computation (megapath_nano.py:1768-1798; the closing filter is the same with stdev 9): the statistic
    without noise, expected_max_depth = max(1, int(aad + stdev * sqrt(aad))) per assembly with aad = adjusted_average_depth,
    and the depth BED of the WHOLE table where depth > expected_max_depth.
    -> noise_bed (as align_list_to_depth_bed), noise_stat: DataFrame(assembly_id, spike_span_bp, spike_span_percent) of the
    assemblies that have a spike."""
    stat = align_stat_by_assembly_id(align_list, assembly_length, assembly_tax, device=device)
    aad = stat['adjusted_average_depth'].to_numpy(dtype=np.float64)
    expected = np.maximum((aad + expected_max_depth_stdev * np.sqrt(aad)).astype(np.int64), 1)
    noise_bed, span = align_list_to_depth_bed(align_list=align_list, min_depth=pandas.DataFrame({'assembly_id': stat['assembly_id'], 'min_depth': expected}),
                                              can_equal_to_min=False, device=device)
    noise_stat = stat[['assembly_id', 'assembly_length']].merge(span.rename(columns={'span_bp': 'spike_span_bp'}), on='assembly_id', how='inner')
    with np.errstate(divide='ignore', invalid='ignore'):
        noise_stat['spike_span_percent'] = noise_stat['spike_span_bp'].to_numpy(dtype=np.float64) / noise_stat['assembly_length'].to_numpy(dtype=np.float64)
    return noise_bed, noise_stat[['assembly_id', 'spike_span_bp', 'spike_span_percent']]


# ---- union of BEDs, alignments selected by their overlap with a BED -----------------------------------------------------------
BED_TILE = 2048   # MPN_BED_TILE of include/mpn_abundance.h: the records one block of the device's union sweep scans (the tests
#                   put their sizes around its multiples; tests/test_bed_select.py checks that the two numbers agree)


def _interval_args(key, start, end):
    return np.ascontiguousarray(key, dtype=np.int32), np.ascontiguousarray(start, dtype=np.int64), np.ascontiguousarray(end, dtype=np.int64)


def device_bed_union(key, start, end, n_keys, key_group=None, n_groups=1):
    """mpn_bed_union.  Interval i = [start[i], end[i]) on key[i] in [0, n_keys); key_group (default: all 0) maps a key to one of
    n_groups.  -> (out_key int32, out_start int64, out_end int64), span int64[n_groups]: the merged intervals ordered by (key,
    start) -- overlapping and touching ones merged, empty ones (start >= end) dropped -- and their summed length per group."""
    key, start, end = _interval_args(key, start, end)
    key_group = np.zeros(int(n_keys), dtype=np.int32) if key_group is None else np.ascontiguousarray(key_group, dtype=np.int32)
    if len(key_group) != int(n_keys):
        raise ValueError('key_group has one entry per key')
    n, cap = len(key), max(len(key), 1)
    ok, os_, oe = np.empty(cap, np.int32), np.empty(cap, np.int64), np.empty(cap, np.int64)
    n_out = ct.c_int64(0)
    span = np.zeros(max(int(n_groups), 1), dtype=np.int64)
    _ffi.check(_lib().mpn_bed_union(n, key.ctypes.data, start.ctypes.data, end.ctypes.data, int(n_keys), key_group.ctypes.data, int(n_groups), cap,
                                    ok.ctypes.data, os_.ctypes.data, oe.ctypes.data, ct.byref(n_out), span.ctypes.data), 'mpn_bed_union')
    m = n_out.value
    return (ok[:m], os_[:m], oe[:m]), span[:n_groups]


def host_bed_union(key, start, end, n_keys, key_group=None, n_groups=1):
    """numpy statement of mpn_bed_union (same arguments, same result): sorted by (key, start), the running maximum of
    (key + 1) << 32 | end is the running maximum of `end` on the current key."""
    key, start, end = _interval_args(key, start, end)
    key_group = np.zeros(int(n_keys), dtype=np.int32) if key_group is None else np.ascontiguousarray(key_group, dtype=np.int32)
    on = start < end
    key, start, end = key[on], start[on], end[on]
    order = np.lexsort((start, key))
    key, start, end = key[order], start[order], end[order]
    k1 = key.astype(np.uint64) + np.uint64(1)
    incl = np.maximum.accumulate(k1 << np.uint64(32) | end.astype(np.uint64)) if len(key) else np.zeros(0, dtype=np.uint64)
    before = np.concatenate([np.zeros(1, dtype=np.uint64), incl[:-1]]) if len(key) else incl
    head = (before >> np.uint64(32) != k1) | (start.astype(np.uint64) > (before & np.uint64(0xffffffff)))   # touching merges
    tail = np.ones(len(key), dtype=bool)
    tail[:-1] = head[1:]
    ok, os_, oe = key[head], start[head], (incl[tail] & np.uint64(0xffffffff)).astype(np.int64)
    span = np.bincount(key_group[ok], weights=(oe - os_).astype(np.float64), minlength=int(n_groups)).astype(np.int64)[:n_groups]
    return (ok, os_, oe), span


def device_cover_by_bed(bed_key, bed_start, bed_end, q_key, q_start, q_end, n_keys):
    """mpn_cover_by_bed -> int64[n_q]: the positions of query i = [q_start[i], q_end[i]) on q_key[i] that a BED interval of the
    same key covers.  q_start <= q_end; BED intervals with start >= end count for nothing."""
    bed_key, bed_start, bed_end = _interval_args(bed_key, bed_start, bed_end)
    q_key, q_start, q_end = _interval_args(q_key, q_start, q_end)
    covered = np.zeros(max(len(q_key), 1), dtype=np.int64)
    _ffi.check(_lib().mpn_cover_by_bed(len(bed_key), bed_key.ctypes.data, bed_start.ctypes.data, bed_end.ctypes.data, len(q_key), q_key.ctypes.data,
                                       q_start.ctypes.data, q_end.ctypes.data, int(n_keys), covered.ctypes.data), 'mpn_cover_by_bed')
    return covered[:len(q_key)]


def host_cover_by_bed(bed_key, bed_start, bed_end, q_key, q_start, q_end, n_keys):
    """numpy statement of mpn_cover_by_bed: the union, the summed length before every merged interval, and per query the first
    merged interval that ends after q_start and the last that starts before q_end, both found on (key, coordinate)."""
    q_key, q_start, q_end = _interval_args(q_key, q_start, q_end)
    if len(q_key) and (q_start > q_end).any():
        raise ValueError(f'query {int(np.flatnonzero(q_start > q_end)[0])}: start > end')
    (mk, ms, me), _ = host_bed_union(bed_key, bed_start, bed_end, n_keys)
    if len(mk) == 0 or len(q_key) == 0:
        return np.zeros(len(q_key), dtype=np.int64)
    before = np.concatenate([[0], np.cumsum(me - ms)])              # before[r] = summed length of the merged intervals < r
    kk, qk = mk.astype(np.int64) << 32, q_key.astype(np.int64) << 32
    a = np.searchsorted(kk | me, qk | q_start, side='right')         # the intervals of a key are disjoint: ends ascend like starts
    b = np.searchsorted(kk | ms, qk | q_end, side='left') - 1
    some = a <= b                                                   # then a..b all lie on the query's key
    a, b = np.where(some, a, 0), np.where(some, b, 0)
    inner = before[b + 1] - before[a] - np.maximum(q_start - ms[a], 0) - np.maximum(me[b] - q_end, 0)
    return np.where(some, inner, 0).astype(np.int64)


_BED_COLUMNS = ['sequence_id', 'start', 'end', 'assembly_id']


def _empty_bed():
    return pandas.DataFrame({'sequence_id': np.zeros(0, dtype=object), 'start': np.zeros(0, dtype=np.int64), 'end': np.zeros(0, dtype=np.int64),
                             'assembly_id': np.zeros(0, dtype=object)})


def _str_objects(col):
    """a column of ids as an object array of str (what pandas.factorize hashes fastest); anything but str is converted"""
    arr = col.to_numpy(dtype=object)
    return arr if pandas.api.types.infer_dtype(arr, skipna=False) == 'string' else arr.astype(str).astype(object)


def _bed_ids(bed):
    """(assembly_id, sequence_id) of a BED as object arrays of str; a BED without assembly_id has '' (megapath_nano.py:370-371)."""
    seq = _str_objects(bed['sequence_id'])
    asm = _str_objects(bed['assembly_id']) if 'assembly_id' in bed.columns else np.full(len(seq), '', dtype=object)
    return asm, seq


def _pair_codes(asm, seq):
    """int32 code per row of its (assembly, sequence) pair, and the number of pairs; the codes carry no order."""
    ac, a_names = pandas.factorize(asm)
    sc, s_names = pandas.factorize(seq)
    code, pairs = pandas.factorize(ac.astype(np.int64) * max(len(s_names), 1) + sc)
    return code.astype(np.int32), len(pairs)


def merge_bed_with_assembly_id(bed_list, device=None):
    """The reference's merge_bed_with_assembly_id: the union of several BEDs per (assembly_id, sequence_id).  A BED is a
    DataFrame(sequence_id, start, end[, assembly_id]); without the last column every row has assembly_id ''; None and empty BEDs
    are skipped.  -> DataFrame(sequence_id, start, end, assembly_id) ordered by the bytes of assembly_id + ',' + sequence_id,
    then start: intervals that overlap or touch merged, empty ones dropped.  device: as in covered_bp_by_assembly."""
    beds = [b for b in bed_list if b is not None and b.shape[0] > 0]
    if not beds:
        return _empty_bed()
    if device is None:
        device = True
    ids = [_bed_ids(b) for b in beds]
    asm, seq = np.concatenate([i[0] for i in ids]), np.concatenate([i[1] for i in ids])
    code, n_pairs = _pair_codes(asm, seq)
    first = np.zeros(n_pairs, dtype=np.int64)
    first[code[::-1]] = np.arange(len(code))[::-1]                   # a row of every pair
    p_asm, p_seq = asm[first].astype(str), seq[first].astype(str)
    order = np.argsort(np.char.add(np.char.add(p_asm, ','), p_seq), kind='stable')
    rank = np.empty(n_pairs, dtype=np.int32)
    rank[order] = np.arange(n_pairs, dtype=np.int32)
    start = np.concatenate([b['start'].to_numpy(dtype=np.int64) for b in beds])
    end = np.concatenate([b['end'].to_numpy(dtype=np.int64) for b in beds])
    (mk, ms, me), _ = (device_bed_union if device else host_bed_union)(rank[code], start, end, n_pairs)
    return pandas.DataFrame({'sequence_id': p_seq[order][mk], 'start': ms, 'end': me, 'assembly_id': p_asm[order][mk]}, columns=_BED_COLUMNS)


def overlap_fraction(covered, length):
    """The fraction that `bedtools annotate` prints for `covered` of `length` positions, as the float64 pandas reads back: the
    float32 quotient, written with '%f' (six decimals) and parsed.  float32 * 10^6 is exact in float64, so rounding there to an
    integer (ties to even, like printf) and dividing by 10^6 gives the same double as the text.  length 0 -> NaN."""
    with np.errstate(divide='ignore', invalid='ignore'):
        f = np.asarray(covered).astype(np.float32) / np.asarray(length).astype(np.float32)
    return np.round(f.astype(np.float64), 6)


def select_alignment_by_bed(*, align_list, bed, max_overlap=100, can_equal_to_max=True, min_overlap=0, can_equal_to_min=True, temp_dir_name=None,
                            device=None):
    """The reference's select_alignment_by_bed with its keyword arguments (temp_dir_name is accepted and ignored): the rows of
    align_list whose target interval [sequence_from, sequence_to) is covered by `bed` to a fraction x with
    min_overlap / 100 <[=] x <[=] max_overlap / 100.  A BED row and an alignment match iff assembly_id and sequence_id are both
    equal (a BED without assembly_id has ''); strand plays no part.  x: overlap_fraction of the exact covered base pairs; an
    alignment of length 0 has x = NaN and is never selected; sequence_to < sequence_from raises ValueError.  bed None or empty:
    align_list itself iff the range admits 0, otherwise none of it.
    -> the selected rows in input order, columns and index as in align_list.  device: as in covered_bp_by_assembly."""
    if bed is None or bed.shape[0] == 0:
        if min_overlap == 0 and can_equal_to_min and (max_overlap != 0 or can_equal_to_max):
            return align_list
        return align_list.iloc[0:0]
    if align_list.shape[0] == 0:
        return align_list
    if device is None:
        device = True
    q_start, q_end = align_list['sequence_from'].to_numpy(dtype=np.int64), align_list['sequence_to'].to_numpy(dtype=np.int64)
    if (q_end < q_start).any():
        raise ValueError(f'row {int(np.flatnonzero(q_end < q_start)[0])}: sequence_to < sequence_from')
    b_asm, b_seq = _bed_ids(bed)
    n_bed = len(b_asm)
    code, n_pairs = _pair_codes(np.concatenate([b_asm, _str_objects(align_list['assembly_id'])]),
                                np.concatenate([b_seq, _str_objects(align_list['sequence_id'])]))
    covered = (device_cover_by_bed if device else host_cover_by_bed)(code[:n_bed], bed['start'].to_numpy(dtype=np.int64), bed['end'].to_numpy(dtype=np.int64),
                                                                     code[n_bed:], q_start, q_end, n_pairs)
    x = overlap_fraction(covered, q_end - q_start)
    hi, lo = max_overlap / 100, min_overlap / 100
    with np.errstate(invalid='ignore'):
        keep = ((x <= hi) if can_equal_to_max else (x < hi)) & ((x >= lo) if can_equal_to_min else (x > lo))
    return align_list[keep]


def noise_removal(*, align_list, noise_bed, non_zero_assembly_ids, max_align_noise_overlap, device=None):
    """step_noise_removal (megapath_nano.py:2257-2278): the alignments that noise_bed covers to at most max_align_noise_overlap
    percent, of the assemblies in non_zero_assembly_ids (ids, or a DataFrame with an assembly_id column; an id twice raises
    ValueError, as the reference's m:1 merge does), in input order.  -> align_list, num_align_before, num_align_after"""
    ids = non_zero_assembly_ids['assembly_id'] if isinstance(non_zero_assembly_ids, pandas.DataFrame) else non_zero_assembly_ids
    ids = [str(i) for i in ids]
    if len(set(ids)) != len(ids):
        raise ValueError('non_zero_assembly_ids: an assembly_id occurs twice')
    out = select_alignment_by_bed(align_list=align_list, bed=noise_bed, max_overlap=max_align_noise_overlap, device=device)
    out = out[out['assembly_id'].astype(str).isin(ids).to_numpy()]
    return out, align_list.shape[0], out.shape[0]


def closing_spike_filter(*, align_list, best_align_list, best_align_list_with_short_alignment, noise_bed, assembly_length, max_align_noise_overlap,
                         expected_max_depth_stdev=9, assembly_tax=None, device=None):
    """step_closing_spike_filter (megapath_nano.py:2353-2408).  The two best-alignment tables are inputs (the reference draws
    them with align_list_to_best_align_list): spikes are sought in best_align_list_with_short_alignment, their BED joins
    noise_bed, and every read whose row of best_align_list is covered by the joint BED to MORE than max_align_noise_overlap
    percent leaves align_list with all its alignments.
    -> align_list, noise_bed (the joint one), closing_spike_noise_bed, noise_stat: DataFrame(assembly_id, closing_spike_span_bp,
    closing_spike_span_percent), num_read_before (rows of best_align_list), num_read_after (distinct reads left)"""
    spike_bed, noise_stat = spike_noise(best_align_list_with_short_alignment, assembly_length, expected_max_depth_stdev, assembly_tax, device=device)
    noise_stat = noise_stat.rename(columns={'spike_span_bp': 'closing_spike_span_bp', 'spike_span_percent': 'closing_spike_span_percent'})
    noise_bed_out = merge_bed_with_assembly_id([noise_bed, spike_bed], device=device)
    gone = select_alignment_by_bed(align_list=best_align_list, bed=noise_bed_out, min_overlap=max_align_noise_overlap, can_equal_to_min=False,
                                   device=device)['read_id']
    out = align_list[~align_list['read_id'].isin(gone).to_numpy()]
    return out, noise_bed_out, spike_bed, noise_stat, best_align_list.shape[0], int(out['read_id'].nunique())


# ---- the best alignment of every read -----------------------------------------------------------------------------------------
BEST_TILE = 2048   # MPN_BEST_TILE of include/mpn_abundance.h: the rows one block of the device's segmented scans covers (the tests
#                    put their sizes around its multiples; tests/test_best_align.py checks that the two numbers agree)
_NO_SCORE = np.iinfo(np.int64).min


def _best_args(read, assembly, score, tiebreak, n_reads, n_assemblies):
    read, assembly = np.ascontiguousarray(read, dtype=np.int32), np.ascontiguousarray(assembly, dtype=np.int32)
    score, tiebreak = np.ascontiguousarray(score, dtype=np.int64), np.ascontiguousarray(tiebreak, dtype=np.float64)
    if not (len(read) == len(assembly) == len(score) == len(tiebreak)):
        raise ValueError('read, assembly, score and tiebreak have one entry per row')
    return read, assembly, score, tiebreak, int(n_reads), int(n_assemblies)


def device_best_candidates(read, assembly, score, tiebreak, n_reads, n_assemblies):
    """mpn_best_candidates.  Row i: read[i] in [0, n_reads), assembly[i] in [0, n_assemblies), score[i] (int64 above -2^63),
    tiebreak[i] (finite).  -> cand_row int64[m], cand_read int32[m], read_count int64[n_reads], read_first int64[n_reads]: per
    (read, assembly) the row with the largest (score, tiebreak), the last in input order among equal ones; of those the ones with
    their read's largest score, ordered by (read, assembly); per read their number and the position of the first."""
    read, assembly, score, tiebreak, n_reads, n_assemblies = _best_args(read, assembly, score, tiebreak, n_reads, n_assemblies)
    n = len(read)
    cand_row, cand_read, n_cand = np.empty(max(n, 1), np.int64), np.empty(max(n, 1), np.int32), ct.c_int64(0)
    count, first = np.zeros(max(n_reads, 1), np.int64), np.zeros(max(n_reads, 1), np.int64)
    _ffi.check(_lib().mpn_best_candidates(n, read.ctypes.data, assembly.ctypes.data, score.ctypes.data, tiebreak.ctypes.data, n_reads, n_assemblies,
                                          cand_row.ctypes.data, cand_read.ctypes.data, ct.byref(n_cand), count.ctypes.data, first.ctypes.data),
               'mpn_best_candidates')
    m = n_cand.value
    return cand_row[:m].copy(), cand_read[:m].copy(), count[:n_reads], first[:n_reads]


def host_best_candidates(read, assembly, score, tiebreak, n_reads, n_assemblies):
    """numpy statement of mpn_best_candidates (same arguments, same result)."""
    read, assembly, score, tiebreak, n_reads, n_assemblies = _best_args(read, assembly, score, tiebreak, n_reads, n_assemblies)
    n = len(read)
    bad = (read < 0) | (read >= n_reads) | (assembly < 0) | (assembly >= n_assemblies) | (score == _NO_SCORE) | ~np.isfinite(tiebreak)
    if bad.any():
        raise ValueError(f'record {int(np.flatnonzero(bad)[0])} outside the domain')
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(n_reads, np.int64), np.zeros(n_reads, np.int64)
    order = np.lexsort((np.arange(n), tiebreak, score, assembly, read))    # the input order decides among equal rows; -0.0 == 0.0
    r, a = read[order], assembly[order]
    last = np.ones(n, dtype=bool)
    last[:-1] = (r[1:] != r[:-1]) | (a[1:] != a[:-1])
    kept = order[last]                                                     # ordered by (read, assembly)
    k_read, k_score = read[kept], score[kept]
    head = np.ones(len(kept), dtype=bool)
    head[1:] = k_read[1:] != k_read[:-1]
    read_max = np.full(n_reads, _NO_SCORE, dtype=np.int64)
    read_max[k_read[head]] = np.maximum.reduceat(k_score, np.flatnonzero(head))
    cand = k_score == read_max[k_read]
    count = np.bincount(k_read[cand], minlength=n_reads).astype(np.int64)
    first = np.cumsum(count) - count
    return kept[cand].astype(np.int64), k_read[cand].astype(np.int32), count, first


def _pick_args(read, weight, tiebreak, draw, n_reads):
    read, weight = np.ascontiguousarray(read, dtype=np.int32), np.ascontiguousarray(weight, dtype=np.int64)
    tiebreak, draw = np.ascontiguousarray(tiebreak, dtype=np.float64), np.ascontiguousarray(draw, dtype=np.float64)
    if not (len(read) == len(weight) == len(tiebreak) == len(draw)):
        raise ValueError('read, weight, tiebreak and draw have one entry per candidate')
    return read, weight, tiebreak, draw, int(n_reads)


def device_pick_weighted(read, weight, tiebreak, draw, n_reads):
    """mpn_pick_weighted.  Candidate j: read[j] in [0, n_reads), non-decreasing; weight[j] >= 0, sums per read below 2^53;
    tiebreak[j] and draw[j] finite.  -> new_tiebreak float64[m], winner int64[n_reads]: a read with one candidate keeps that
    candidate's tiebreak; in the others new = draw * (1.0 if the read's summed weight s <= 0 else weight / s) in float64; winner[r] =
    the candidate of read r with the largest new tiebreak, the last among equal ones, -1 for a read without candidates."""
    read, weight, tiebreak, draw, n_reads = _pick_args(read, weight, tiebreak, draw, n_reads)
    m = len(read)
    new, winner = np.empty(max(m, 1), np.float64), np.full(max(n_reads, 1), -1, np.int64)
    _ffi.check(_lib().mpn_pick_weighted(m, read.ctypes.data, weight.ctypes.data, tiebreak.ctypes.data, draw.ctypes.data, n_reads, new.ctypes.data,
                                        winner.ctypes.data), 'mpn_pick_weighted')
    return new[:m], winner[:n_reads]


def host_pick_weighted(read, weight, tiebreak, draw, n_reads):
    """numpy statement of mpn_pick_weighted (same arguments, same result)."""
    read, weight, tiebreak, draw, n_reads = _pick_args(read, weight, tiebreak, draw, n_reads)
    m = len(read)
    total = np.zeros(n_reads, dtype=np.int64)
    bad = (read < 0) | (read >= n_reads) | (weight < 0) | (weight >= 2 ** 53) | ~np.isfinite(tiebreak) | ~np.isfinite(draw)
    bad[1:] |= read[1:] < read[:-1]
    if not bad.any():
        np.add.at(total, read, weight)
        bad |= total[read] >= 2 ** 53
    if bad.any():
        raise ValueError(f'candidate {int(np.flatnonzero(bad)[0])} outside the domain')
    count = np.bincount(read, minlength=n_reads)
    s = total[read]
    with np.errstate(divide='ignore', invalid='ignore'):
        relative = np.where(s <= 0, 1.0, weight.astype(np.float64) / s.astype(np.float64))
    new = np.where(count[read] == 1, tiebreak, draw * relative)
    winner = np.full(n_reads, -1, dtype=np.int64)
    order = np.lexsort((np.arange(m), new, read))
    last = np.ones(m, dtype=bool)
    last[:-1] = read[order][1:] != read[order][:-1]
    winner[read[order[last]]] = order[last]
    return new, winner


def _second_args(read, assembly, score, n_reads, excluded):
    read, assembly = np.ascontiguousarray(read, dtype=np.int32), np.ascontiguousarray(assembly, dtype=np.int32)
    score, excluded = np.ascontiguousarray(score, dtype=np.int64), np.ascontiguousarray(excluded, dtype=np.int32)
    if not (len(read) == len(assembly) == len(score)) or len(excluded) != int(n_reads):
        raise ValueError('read, assembly and score have one entry per row, excluded one per read')
    return read, assembly, score, int(n_reads), excluded


def device_second_best_by_read(read, assembly, score, n_reads, excluded):
    """mpn_second_best_by_read -> int64[n_reads]: the largest score[i] over the rows of read r with assembly[i] != excluded[r]
    (-1: nothing is excluded), 0 for a read without such a row.  assembly >= 0, score above -2^63."""
    read, assembly, score, n_reads, excluded = _second_args(read, assembly, score, n_reads, excluded)
    second = np.zeros(max(n_reads, 1), np.int64)
    _ffi.check(_lib().mpn_second_best_by_read(len(read), read.ctypes.data, assembly.ctypes.data, score.ctypes.data, n_reads, excluded.ctypes.data,
                                              second.ctypes.data), 'mpn_second_best_by_read')
    return second[:n_reads]


def host_second_best_by_read(read, assembly, score, n_reads, excluded):
    """numpy statement of mpn_second_best_by_read (same arguments, same result)."""
    read, assembly, score, n_reads, excluded = _second_args(read, assembly, score, n_reads, excluded)
    bad = (read < 0) | (read >= n_reads) | (assembly < 0) | (score == _NO_SCORE)
    if bad.any() or (excluded < -1).any():
        raise ValueError('a record outside the domain')
    second = np.full(n_reads, _NO_SCORE, dtype=np.int64)
    on = assembly != excluded[read]
    np.maximum.at(second, read[on], score[on])
    second[second == _NO_SCORE] = 0
    return second


def align_list_to_best_align_list(*, align_list, assembly_length, assembly_tax=None, noise_bed=None, rng=None, device=None):
    """The reference's align_list_to_best_align_list: one row per read, its best alignment.  align_list: the Align() table with
    read_id and assembly_id as strings; assembly_length / assembly_tax / noise_bed: as in align_stat_by_assembly_id (they stand for
    the reference's assembly_metadata).  Per (read, assembly) the row with the largest (alignment_score, tiebreaker) is kept, the
    last in table order among equal ones; the kept rows with their read's largest score are its candidates.  A read with one
    candidate keeps it and its tiebreaker.  For the others, assembly_abundance = adjusted_total_aligned_bp of
    align_stat_by_assembly_id over the one-candidate reads' rows (0 for an assembly that has none), and every candidate, in the order
    of (read_id, assembly_id), gets the tiebreaker rng() * (abundance of its assembly / summed abundance of the read's candidates; 1
    where that sum is 0); the largest wins, the last one among equal ones.
    rng: a callable without arguments, default random.random; called once per candidate of a read with several, in that order, and
    never otherwise.  -> the winning rows with their index labels and columns, ordered by read_id, alignment_score_tiebreaker
    replaced in the drawn reads.  An empty table comes back empty, without a draw.  device: as in covered_bp_by_assembly."""
    if align_list.shape[0] == 0:
        return align_list.copy()
    if device is None:
        device = True
    if rng is None:
        rng = random.random
    reads, rc = _codes(align_list['read_id'])              # np.unique orders str like pandas' sort_values: the order of the draws
    asms, ac = _codes(align_list['assembly_id'])
    tiebreak = align_list['alignment_score_tiebreaker'].to_numpy(dtype=np.float64)
    cand_row, cand_read, count, _ = (device_best_candidates if device else host_best_candidates)(
        rc, ac, align_list['alignment_score'].to_numpy(dtype=np.int64), tiebreak, len(reads), len(asms))
    alone = count[cand_read] == 1
    weight = np.zeros(len(cand_row), dtype=np.int64)
    if alone.any() and not alone.all():
        stat = align_stat_by_assembly_id(align_list.iloc[cand_row[alone]], assembly_length, assembly_tax, noise_bed=noise_bed, device=device)
        abundance = np.zeros(len(asms), dtype=np.int64)
        abundance[pandas.Index(asms).get_indexer(stat['assembly_id'].to_numpy())] = stat['adjusted_total_aligned_bp'].to_numpy(dtype=np.int64)
        weight = abundance[ac[cand_row]]
    draw = np.zeros(len(cand_row), dtype=np.float64)
    draw[~alone] = [rng() for _ in range(int((~alone).sum()))]
    new, winner = (device_pick_weighted if device else host_pick_weighted)(cand_read, weight, tiebreak[cand_row], draw, len(reads))
    out = align_list.iloc[cand_row[winner]].copy()
    out['alignment_score_tiebreaker'] = new[winner]
    return out


def short_alignment_removal(*, align_list, min_align_length, assembly_length, assembly_tax=None, rng=None, device=None):
    """step_short_alignment_removal (megapath_nano.py:2302-2321): every read whose best alignment (align_list_to_best_align_list,
    without a noise BED) spans fewer than min_align_length target positions leaves with all its alignments.
    -> align_list (input order), num_read_before (reads), num_read_after"""
    best = align_list_to_best_align_list(align_list=align_list, assembly_length=assembly_length, assembly_tax=assembly_tax, rng=rng, device=device)
    gone = best['read_id'][((best['sequence_to'] - best['sequence_from']) < min_align_length).to_numpy()]
    out = align_list[~align_list['read_id'].isin(gone).to_numpy()]
    return out, best.shape[0], best.shape[0] - gone.shape[0]


def unique_alignment(*, align_list, best_align_list, human_best_align_list=None, decoy_best_align_list=None, unique_align_threshold, device=None):
    """step_unique_alignment (megapath_nano.py:2561-2590): the rows of best_align_list (one per read; ValueError otherwise) whose
    score stands clear of the read's second best -- the largest alignment_score among the read's rows of align_list on OTHER
    assemblies than the best row's and its rows in the human and decoy tables (read_id, alignment_score), 0 if there is none:
    kept iff float64(alignment_score) * (unique_align_threshold / 100) > second best.
    -> best_align_list with the column second_best_alignment_score, num_read_before, num_read_after"""
    if device is None:
        device = True
    if best_align_list['read_id'].duplicated().any():
        raise ValueError('best_align_list: a read_id occurs twice')
    extra = [t for t in (human_best_align_list, decoy_best_align_list) if t is not None and t.shape[0] > 0]
    n_al, n_best = align_list.shape[0], best_align_list.shape[0]
    reads, rc = _codes(pandas.concat([t['read_id'] for t in [align_list, best_align_list] + extra], ignore_index=True))
    asms, ac = _codes(pandas.concat([align_list['assembly_id'], best_align_list['assembly_id']], ignore_index=True))
    excluded = np.full(len(reads), -1, dtype=np.int32)
    excluded[rc[n_al:n_al + n_best]] = ac[n_al:]
    # the human and decoy rows count whatever their assembly: they go under a code of their own
    row_read = np.concatenate([rc[:n_al], rc[n_al + n_best:]])
    row_asm = np.concatenate([ac[:n_al], np.full(len(rc) - n_al - n_best, len(asms), dtype=ac.dtype)])
    row_score = np.concatenate([t['alignment_score'].to_numpy(dtype=np.int64) for t in [align_list] + extra])
    second = (device_second_best_by_read if device else host_second_best_by_read)(row_read, row_asm, row_score, len(reads), excluded)
    out = best_align_list.copy()
    out['second_best_alignment_score'] = second[rc[n_al:n_al + n_best]]
    keep = out['alignment_score'].to_numpy(dtype=np.float64) * (unique_align_threshold / 100) > out['second_best_alignment_score'].to_numpy(dtype=np.float64)
    out = out[keep].copy()
    return out, n_best, out.shape[0]


def closing_spike_step(*, align_list, align_list_with_short_alignment, noise_bed, assembly_length, max_align_noise_overlap, expected_max_depth_stdev=9,
                       assembly_tax=None, rng=None, device=None):
    """The whole step_closing_spike_filter (megapath_nano.py:2330-2422): the best table of align_list is drawn first, that of
    align_list_with_short_alignment second, as the reference draws them, and both go to closing_spike_filter.  -> its result"""
    kw = dict(assembly_length=assembly_length, assembly_tax=assembly_tax, rng=rng, device=device)
    best = align_list_to_best_align_list(align_list=align_list, **kw)
    best_with_short = align_list_to_best_align_list(align_list=align_list_with_short_alignment, **kw)
    return closing_spike_filter(align_list=align_list, best_align_list=best, best_align_list_with_short_alignment=best_with_short, noise_bed=noise_bed,
                                assembly_length=assembly_length, max_align_noise_overlap=max_align_noise_overlap,
                                expected_max_depth_stdev=expected_max_depth_stdev, assembly_tax=assembly_tax, device=device)


def combine_with_human_and_decoy(*, align_list, human_and_decoy_best_align_list):
    """step_combine_with_human_and_decoy (megapath_nano.py:2432-2441): the rows of align_list that score above their read's row of
    human_and_decoy_best_align_list (one row per read; a read it lacks has 0 there), followed by that table's own rows; the columns
    in sorted order (pandas.concat(sort=True))."""
    other = human_and_decoy_best_align_list
    if other['read_id'].duplicated().any():
        raise ValueError('human_and_decoy_best_align_list: a read_id occurs twice')
    best = pandas.Series(other['alignment_score'].to_numpy(), index=other['read_id'].to_numpy())
    bar = align_list['read_id'].map(best).fillna(0).to_numpy()
    return pandas.concat([align_list[align_list['alignment_score'].to_numpy() > bar], other], axis=0, sort=True)


# ---- good alignments, grouped sums, the per-sequence statistic, assembly selection ---------------------------------------------
_SCORE_LIMIT = 2 ** 53   # |score| below it: the conversion to float64 is exact
_VALUE_LIMIT = 2 ** 32   # |value| below it: 2^31 of them sum inside int64
SUM_COLS = 6             # the columns one mpn_sum_by_key call takes


def _threshold_arg(threshold):
    """-> use_threshold, threshold as a Python float (None: no threshold)"""
    return (0, 0.0) if threshold is None else (1, float(threshold))


def device_good_rows(read, unit, score, tiebreak, n_reads, n_units, threshold=None):
    """mpn_good_rows.  Row i: read[i] in [0, n_reads), unit[i] in [0, n_units), |score[i]| < 2^53, tiebreak[i] finite.
    -> good_row int64[m], read_best int64[n_reads]: per (read, unit) the row with the largest (score, tiebreak) is kept, the last in
    input order among equal ones; read_best[r] = the largest kept score of read r (0 without rows); good_row = the kept rows with
    float64(score) >= float64(read_best) * threshold (threshold None: every kept row), ordered by (read, unit)."""
    read, unit, score, tiebreak, n_reads, n_units = _best_args(read, unit, score, tiebreak, n_reads, n_units)
    use, threshold = _threshold_arg(threshold)
    n = len(read)
    good, n_good, best = np.empty(max(n, 1), np.int64), ct.c_int64(0), np.zeros(max(n_reads, 1), np.int64)
    _ffi.check(_lib().mpn_good_rows(n, read.ctypes.data, unit.ctypes.data, score.ctypes.data, tiebreak.ctypes.data, n_reads, n_units, use, threshold,
                                    good.ctypes.data, ct.byref(n_good), best.ctypes.data), 'mpn_good_rows')
    return good[:n_good.value].copy(), best[:n_reads]


def host_good_rows(read, unit, score, tiebreak, n_reads, n_units, threshold=None):
    """numpy statement of mpn_good_rows (same arguments, same result)."""
    read, unit, score, tiebreak, n_reads, n_units = _best_args(read, unit, score, tiebreak, n_reads, n_units)
    use, threshold = _threshold_arg(threshold)
    if not math.isfinite(threshold):
        raise ValueError('the threshold is not finite')
    n = len(read)
    bad = (read < 0) | (read >= n_reads) | (unit < 0) | (unit >= n_units) | (score <= -_SCORE_LIMIT) | (score >= _SCORE_LIMIT) | ~np.isfinite(tiebreak)
    if bad.any():
        raise ValueError(f'record {int(np.flatnonzero(bad)[0])} outside the domain')
    read_best = np.zeros(n_reads, dtype=np.int64)
    if n == 0:
        return np.zeros(0, np.int64), read_best
    order = np.lexsort((np.arange(n), tiebreak, score, unit, read))        # the input order decides among equal rows; -0.0 == 0.0
    r, u = read[order], unit[order]
    last = np.ones(n, dtype=bool)
    last[:-1] = (r[1:] != r[:-1]) | (u[1:] != u[:-1])
    kept = order[last]                                                     # ordered by (read, unit)
    k_read, k_score = read[kept], score[kept]
    head = np.ones(len(kept), dtype=bool)
    head[1:] = k_read[1:] != k_read[:-1]
    read_best[k_read[head]] = np.maximum.reduceat(k_score, np.flatnonzero(head))
    if use:
        kept = kept[k_score.astype(np.float64) >= read_best[k_read].astype(np.float64) * np.float64(threshold)]   # one float64 product
    return kept.astype(np.int64), read_best


def _sum_args(key, n_keys, cols):
    key = np.ascontiguousarray(key, dtype=np.int32)
    cols = [np.asarray(c, dtype=np.int64) for c in cols]
    if any(c.shape != key.shape for c in cols):
        raise ValueError('every column has one value per row')
    flat = np.ascontiguousarray(np.concatenate(cols)) if cols else np.zeros(0, np.int64)
    return key, int(n_keys), len(cols), flat


def device_sum_by_key(key, n_keys, cols):
    """mpn_sum_by_key.  key[i] in [0, n_keys); cols: 1 to 6 arrays of one value per row, |value| < 2^32.
    -> count int64[n_keys], sums int64[len(cols), n_keys]: the rows and the column sums per key, 0 for a key without rows."""
    key, n_keys, n_cols, flat = _sum_args(key, n_keys, cols)
    count, sums = np.zeros(max(n_keys, 1), np.int64), np.zeros(max(n_cols * n_keys, 1), np.int64)
    _ffi.check(_lib().mpn_sum_by_key(len(key), key.ctypes.data, n_keys, n_cols, flat.ctypes.data, count.ctypes.data, sums.ctypes.data), 'mpn_sum_by_key')
    return count[:n_keys], sums[:n_cols * n_keys].reshape(n_cols, n_keys)


def host_sum_by_key(key, n_keys, cols):
    """numpy statement of mpn_sum_by_key (same arguments, same result).  np.bincount adds in float64, so every value goes in as
    v >> 16 and v & 0xffff: over fewer than 2^31 rows both sums stay below 2^53 and are exact."""
    key, n_keys, n_cols, flat = _sum_args(key, n_keys, cols)
    if not 1 <= n_cols <= SUM_COLS:
        raise ValueError(f'1 to {SUM_COLS} columns')
    bad = (key < 0) | (key >= n_keys)
    if bad.any():
        raise ValueError(f'record {int(np.flatnonzero(bad)[0])} outside the domain')
    vals = flat.reshape(n_cols, len(key))
    if ((vals <= -_VALUE_LIMIT) | (vals >= _VALUE_LIMIT)).any():
        raise ValueError('a value outside the domain')
    sums = np.zeros((n_cols, n_keys), dtype=np.int64)
    for c in range(n_cols):
        high = np.bincount(key, weights=(vals[c] >> 16).astype(np.float64), minlength=n_keys).astype(np.int64)
        low = np.bincount(key, weights=(vals[c] & 0xffff).astype(np.float64), minlength=n_keys).astype(np.int64)
        sums[c] = (high << 16) + low
    return np.bincount(key, minlength=n_keys).astype(np.int64)[:n_keys], sums


def _best_rows(align_list, unit_col, threshold, device):
    """positions of the good rows of align_list (mpn_good_rows; unit_col None: the single unit 0), ordered by (read_id, unit)"""
    reads, rc = _codes(align_list['read_id'])
    if unit_col is None:
        n_units, uc = 1, np.zeros(len(rc), dtype=np.int32)
    else:
        units, uc = _codes(align_list[unit_col])
        n_units = len(units)
    run = device_good_rows if device else host_good_rows
    return run(rc, uc, align_list['alignment_score'].to_numpy(dtype=np.int64), align_list['alignment_score_tiebreaker'].to_numpy(dtype=np.float64),
               len(reads), n_units, threshold)[0]


def good_align_list(*, align_list, good_align_threshold, device=None):
    """The reference's good_align_list (megapath_nano.py:642-663): per (read_id, assembly_id) the row with the largest
    (alignment_score, tiebreaker), the last in table order among equal ones; of those the rows with
    alignment_score >= (their read's largest kept score) * (good_align_threshold / 100), the product in float64.
    -> those rows with their index labels and columns, ordered by (read_id, assembly_id).  An empty table comes back empty.
    device: as in covered_bp_by_assembly."""
    if align_list.shape[0] == 0:
        return align_list.copy()
    if device is None:
        device = True
    return align_list.iloc[_best_rows(align_list, 'assembly_id', good_align_threshold / 100, device)]


def best_align_per_read(align_list, device=None):
    """`sort_values(['read_id', 'alignment_score', 'alignment_score_tiebreaker']).drop_duplicates('read_id', keep='last')` of the
    reference (megapath_nano.py:1287, :1459): one row per read, the one with the largest (alignment_score, tiebreaker), the last in
    table order among equal ones, ordered by read_id, index labels and columns kept.  device: as in covered_bp_by_assembly."""
    if align_list.shape[0] == 0:
        return align_list.copy()
    if device is None:
        device = True
    return align_list.iloc[_best_rows(align_list, None, None, device)]


def _key_sums(device):
    run = device_sum_by_key if device else host_sum_by_key

    def sums(code, n, cols):
        count, s = run(code, n, cols)
        return count, list(s)
    return sums


def _align_stat_by_assembly_id_exact(align_list, assembly_length, assembly_tax, device):
    """align_stat_by_assembly_id with the best rows from mpn_good_rows and the integer sums from mpn_sum_by_key (device) or from
    their host statements: the same table wherever align_stat_by_assembly_id's float64 sums are exact (below 2^53)."""
    best = align_list.iloc[_best_rows(align_list, 'assembly_id', None, device)]
    return _stat_of_best_rows(best, assembly_length, assembly_tax, None, device, _key_sums(device))


_SEQUENCE_STAT_COLUMNS = ['assembly_id', 'sequence_id', 'total_number_of_read', 'total_read_bp', 'total_aligned_bp', 'match', 'edit_dist', 'alignment_score',
                          'alignment_score_tiebreaker', 'sequence_length', 'covered_bp', 'noise_span_bp', 'average_read_length', 'average_depth',
                          'covered_percent', 'noise_span_percent', 'adjusted_covered_percent', 'average_identity', 'average_edit_dist',
                          'average_alignment_score', 'adjusted_average_depth', 'adjusted_total_aligned_bp']


def align_stat_by_sequence_id(align_list, sequence_length, noise_bed=None, device=None):
    """The reference's align_list_to_align_stat_by_sequence_id (megapath_nano.py:585-639).  align_list: the Align() table;
    sequence_length: DataFrame(sequence_id, sequence_length), a sequence it lacks has length 0; noise_bed (optional):
    DataFrame(sequence_id, start, end[, assembly_id]), matched on sequence_id alone (`bedtools subtract` sees that column only).
    Per (read_id, sequence_id) the row with the largest (alignment_score, tiebreaker) is kept; the sums of summary_stat_1 per
    (assembly_id, sequence_id); covered_bp = the union length of the kept rows' target intervals on the sequence minus what the
    noise BED covers there; noise_span_bp = the summed length of the noise intervals of the sequence; the columns of summary_stat_2
    over sequence_length.  -> DataFrame, one row per sequence, ordered by the bytes of assembly_id + ',' + sequence_id.
    A sequence_id under two assemblies raises ValueError (the reference's validate='1:1' merge raises there).
    device: as in covered_bp_by_assembly."""
    if align_list.shape[0] == 0:
        return pandas.DataFrame({c: np.zeros(0, dtype=object if c.endswith('_id') else np.float64 if 'average' in c or 'percent' in c or 'tiebreaker' in c
                                             else np.int64) for c in _SEQUENCE_STAT_COLUMNS})
    if device is None:
        device = True
    best = align_list.iloc[_best_rows(align_list, 'sequence_id', None, device)]
    asm = best['assembly_id'].to_numpy(dtype=object).astype(str)
    seqs, sc = _codes(best['sequence_id'])
    n = len(seqs)
    asm_of = np.empty(n, dtype=asm.dtype)
    asm_of[sc] = asm
    if not np.array_equal(asm_of[sc], asm):
        raise ValueError(f'sequence_id {seqs[sc[np.flatnonzero(asm_of[sc] != asm)[0]]]} lies under two assemblies')
    order = np.argsort(np.char.add(np.char.add(asm_of, ','), seqs), kind='stable')    # the order of groupby(assembly_id + ',' + sequence_id)
    rank = np.empty(n, dtype=np.int32)
    rank[order] = np.arange(n, dtype=np.int32)
    key = rank[sc]
    out = pandas.DataFrame({'assembly_id': asm_of[order], 'sequence_id': seqs[order], **_summary_stat_1(best, key, n, _key_sums(device))})
    length = dict(zip(sequence_length['sequence_id'].astype(str), sequence_length['sequence_length']))
    out['sequence_length'] = np.array([int(length.get(s, 0)) for s in out['sequence_id']], dtype=np.int64)
    cover = device_cover_by_group if device else host_cover_by_group
    start, end = best['sequence_from'].to_numpy(dtype=np.int64), best['sequence_to'].to_numpy(dtype=np.int64)
    out['noise_span_bp'] = 0
    if noise_bed is None or noise_bed.shape[0] == 0:
        covered = cover(key, key, start, end, n)
    else:
        # |A \ N| = |A u N| - |N| per sequence, over the noise intervals of the sequences that carry alignments
        where = pandas.Index(out['sequence_id']).get_indexer(noise_bed['sequence_id'].astype(str))
        hit = where >= 0
        n_key = where[hit].astype(np.int32)
        n_start, n_end = noise_bed['start'].to_numpy(dtype=np.int64)[hit], noise_bed['end'].to_numpy(dtype=np.int64)[hit]
        both_key = np.concatenate([key, n_key])
        covered = cover(both_key, both_key, np.concatenate([start, n_start]), np.concatenate([end, n_end]), n) - cover(n_key, n_key, n_start, n_end, n)
        # bed_to_covered_bp_by_sequence_id(noise_bed): the plain sum of the noise intervals' lengths per sequence
        out['noise_span_bp'] = np.bincount(n_key, weights=(n_end - n_start).astype(np.float64), minlength=n).astype(np.int64)
    out.insert(out.columns.get_loc('noise_span_bp'), 'covered_bp', np.asarray(covered, dtype=np.int64))
    return _summary_stat_2(out, 'sequence_length')


class AssemblySelection:
    """What assembly_selection returns: the attributes of the reference's assembly_selection.O and the two counts it logs."""
    __slots__ = ('align_list', 'best_align_list', 'good_align_list', 'align_stat', 'assembly_list', 'species_align_stat',
                 'num_species_reached_min_average_depth', 'num_species_not_reached')


def _species_pick(stat):
    return stat.sort_values(['species_tax_id', 'adjusted_average_depth', 'alignment_score_tiebreaker']).drop_duplicates(subset=['species_tax_id'], keep='last')


def assembly_selection(*, species_align_list, assembly_align_list, species_list, read_id_species_id, assembly_ID_min_average_depth, good_align_threshold,
                       assembly_length, assembly_tax, device=None):
    """step_assembly_selection (megapath_nano.py:1400-1476).  species_align_list / assembly_align_list: the Align() tables against
    the species-ID and the assembly-ID genome sets, each with a species_tax_id column; species_list: DataFrame with species_tax_id,
    one row per species; read_id_species_id: DataFrame(read_id, species_tax_id), one row per read; assembly_length / assembly_tax:
    as in align_stat_by_assembly_id (they stand for the reference's assembly_metadata).
    The statistic per assembly of species_align_list picks one assembly per species -- the largest (adjusted_average_depth, summed
    tiebreaker), the last among equal ones -- and the species of species_list whose pick reaches assembly_ID_min_average_depth keep
    their rows of assembly_align_list; species_align_list keeps the rows on the species its read was placed in.  Of the two together
    (`concat(sort=True)`): the best row per read, the good rows (good_align_list), the statistic per assembly of the good rows and,
    from it, one assembly per species.  The per-species pick runs over one row per assembly and stays in pandas.
    -> AssemblySelection.  device: as in covered_bp_by_assembly; the best rows come from mpn_good_rows and the integer sums from
    mpn_sum_by_key (or their host statements), and the summed tiebreaker is np.bincount over the listed rows either way."""
    if device is None:
        device = True

    def stat(table):
        return _align_stat_by_assembly_id_exact(table, assembly_length, assembly_tax, device)
    out = AssemblySelection()
    species_stat = _species_pick(stat(species_align_list))
    species_stat = species_stat.merge(right=species_list[['species_tax_id']].set_index('species_tax_id'), how='inner', left_on='species_tax_id',
                                      right_index=True, suffixes=['', '_y'], validate='1:1')
    reached = species_stat[species_stat['adjusted_average_depth'].to_numpy() >= assembly_ID_min_average_depth][['species_tax_id']]
    not_reached = species_list.merge(right=reached.assign(reached_min_average_depth=1).set_index('species_tax_id'), how='left', left_on='species_tax_id',
                                     right_index=True, suffixes=['', '_y'], validate='1:1').fillna(0).query('reached_min_average_depth == 0')
    from_assembly = assembly_align_list.merge(right=reached.set_index('species_tax_id'), how='inner', left_on='species_tax_id', right_index=True,
                                              suffixes=['', '_y'], validate='m:1')
    from_species = species_align_list.merge(right=read_id_species_id.rename(columns={'species_tax_id': 'read_species_tax_id'}).set_index('read_id'),
                                            how='inner', left_on='read_id', right_index=True, suffixes=['', '_y'], validate='m:1')
    from_species = from_species[(from_species['species_tax_id'] == from_species['read_species_tax_id']).to_numpy()].drop(['read_species_tax_id'], axis=1)
    out.species_align_stat = species_stat
    out.align_list = pandas.concat([from_assembly, from_species], axis=0, sort=True)
    out.best_align_list = best_align_per_read(out.align_list, device=device)
    out.good_align_list = good_align_list(align_list=out.align_list, good_align_threshold=good_align_threshold, device=device)
    out.align_stat = stat(out.good_align_list)
    out.assembly_list = _species_pick(out.align_stat).copy()
    out.num_species_reached_min_average_depth = int(reached.shape[0])
    out.num_species_not_reached = int(not_reached.shape[0])
    return out
