"""Amplicon realigner: host-side mirror of the reference's ctypes use of `realigner`
(/root/reference/bin/realignment/realign_illumina_reads.py:32,40-43,579-629) over libmpn.so.

    realign_reads(...)   one window through the reference's own C entry points (realign_reads / free_memory)
    realign_batch([...]) many windows in one call (mpn_realign_batch): one launch per stage over all of them
    place_batch([...])   the placement stage of realign_batch on its own (mpn_realign_place_batch), for the parity tests

and of its use of `debruijn_graph` (realign_illumina_reads.py:543-566), the producer of the realigner's haplotypes:

    get_consensus(...)     one window through the reference's C entry point (get_consensus / free_consensus)
    consensus_batch([...]) many windows in one call (mpn_dbg_consensus_batch): one workgroup per window
    realign_windows([...]) consensus, then realign_batch on the windows it leaves: the body of the script's window loop

Both return, per read, (position, cigar_string) exactly as the reference's `realigner_p.contents` would hold them
(a match run is written 'X'; reads the realigner leaves alone come back with their input position and CIGAR).
"""
import ctypes as ct

from . import _ffi

MAX_REGION_READS = 1000   # realign_illumina_reads.py:38 max_region_reads_num, realigner.h:44-45


class StructPointer(ct.Structure):   # realign_illumina_reads.py:40-43
    _fields_ = [('position', ct.c_int * MAX_REGION_READS), ('cigar_string', ct.c_char_p * MAX_REGION_READS)]


class Window(ct.Structure):          # include/mpn_realign.h mpn_realign_window
    _fields_ = [('n_reads', ct.c_int32), ('seqs', ct.POINTER(ct.c_char_p)), ('positions', ct.POINTER(ct.c_int32)),
                ('cigars', ct.POINTER(ct.c_char_p)), ('reference', ct.c_char_p), ('n_haps', ct.c_int32),
                ('haplotypes', ct.POINTER(ct.c_char_p)), ('ref_start', ct.c_int32), ('ref_prefix', ct.c_int32),
                ('ref_suffix', ct.c_int32)]


def _b(s):
    return s if isinstance(s, bytes) else s.encode()


def realign_reads(seqs, positions, cigars, reference, haplotypes, ref_start, ref_prefix, ref_suffix):
    lib = _ffi.lib()
    n = len(seqs)
    if n > MAX_REGION_READS:
        raise ValueError('at most %d reads per window' % MAX_REGION_READS)
    seq_list = (ct.c_char_p * n)(*[_b(s) for s in seqs])
    pos_list = (ct.c_int * n)(*positions)
    cig_list = (ct.c_char_p * n)(*[_b(c) for c in cigars])
    lib.realign_reads.restype = ct.POINTER(StructPointer)
    lib.realign_reads.argtypes = [ct.c_char_p * n, ct.c_int * n, ct.c_char_p * n, ct.c_char_p, ct.c_char_p, ct.c_int, ct.c_int,
                                  ct.c_int, ct.c_int]
    p = lib.realign_reads(seq_list, pos_list, cig_list, _b(reference), b' '.join(_b(h) for h in haplotypes), ref_start,
                          ref_prefix, ref_suffix, n)
    if not p:
        raise _ffi.MpnError('realign_reads failed: ' + _ffi.last_error())
    out = [(int(p.contents.position[i]), p.contents.cigar_string[i].decode()) for i in range(n)]
    lib.free_memory.restype = None
    lib.free_memory.argtypes = [ct.POINTER(StructPointer), ct.c_int]
    lib.free_memory(p, n)
    return out


def _window_array(windows):
    """-> (mpn_realign_window array, the ctypes arrays it points into, reads in all)"""
    arr = (Window * max(len(windows), 1))()
    keep = []
    total = 0
    for k, w in enumerate(windows):
        n, nh = len(w['seqs']), len(w['haplotypes'])
        seqs = (ct.c_char_p * max(n, 1))(*[_b(s) for s in w['seqs']])
        cigs = (ct.c_char_p * max(n, 1))(*[_b(c) for c in w['cigars']])
        pos = (ct.c_int32 * max(n, 1))(*w['positions'])
        haps = (ct.c_char_p * max(nh, 1))(*[_b(h) for h in w['haplotypes']])
        ref = None if w['reference'] is None else _b(w['reference'])
        keep.append((seqs, cigs, pos, haps, ref))
        arr[k] = Window(n, seqs, pos, cigs, ref, nh, haps, w['ref_start'], w['ref_prefix'], w['ref_suffix'])
        total += n
    return arr, keep, total


class Hit(ct.Structure):             # include/mpn_realign.h mpn_realign_hit
    _fields_ = [(k, ct.c_int32) for k in ('window', 'hap', 'read', 'start', 'mm', 't', 'p')]


def place_call(windows, list_cap=0, grid_cap=0, hit_cap=None):
    """mpn_realign_place_batch as it is: -> (return code, dict of the output arrays).  The arrays are filled with marks first
    (bytes of 0x55), so that a caller sees whether a refused call wrote to them."""
    lib = _ffi.lib()
    arr, keep, _ = _window_array(windows)   # keep: alive until the call has returned
    n_haps = sum(len(w['haplotypes']) for w in windows)
    n_pairs = sum(len(w['haplotypes']) * len(w['seqs']) for w in windows)
    n_kmer = sum(max(0, len(h) - 31) for w in windows for h in w['haplotypes'])
    if hit_cap is None:
        hit_cap = sum(max(0, len(h) - len(s) + 1) for w in windows for h in w['haplotypes'] for s in w['seqs'])
    out = dict(hits=(Hit * max(hit_cap, 1))(), n_hits=ct.c_int64(), kmer=(ct.c_uint8 * max(n_kmer, 1))(),
               dropped=(ct.c_uint8 * max(n_haps, 1))(), hap_score=(ct.c_int32 * max(n_haps, 1))(),
               position=(ct.c_int32 * max(n_pairs, 1))(), score=(ct.c_int32 * max(n_pairs, 1))(), launches=ct.c_int32())
    for v in out.values():
        ct.memset(ct.byref(v), 0x55, ct.sizeof(v))
    P = ct.c_void_p
    lib.mpn_realign_place_batch.restype = ct.c_int
    lib.mpn_realign_place_batch.argtypes = [ct.c_int32, ct.POINTER(Window), ct.c_int64, ct.c_int32, ct.c_int64, P, P, P, P, P, P, P, P]
    rc = lib.mpn_realign_place_batch(len(windows), arr, list_cap, grid_cap, hit_cap, ct.byref(out['hits']), ct.byref(out['n_hits']),
                                     ct.byref(out['kmer']), ct.byref(out['dropped']), ct.byref(out['hap_score']),
                                     ct.byref(out['position']), ct.byref(out['score']), ct.byref(out['launches']))
    return rc, out


def place_batch(windows, list_cap=0, grid_cap=0):
    """The placement stage on its own (mpn_realign_place_batch): the kernel's hits and k-mer bitmaps and the per-haplotype
    bookkeeping, as realign_batch has them before any Smith-Waterman step.  windows as for realign_batch; list_cap / grid_cap: the
    first launch's hit-list capacity and the largest grid, 0 for the realigner's own.  -> (one dict per window, kernel launches):
        hits        [(hap, read, start, mm, t, p)] in the reference's order of evaluation (haplotype, t, read, p)
        kmer        per haplotype: bytes, 1 at the positions 0 .. HL - 32 that hold a 32-mer of any read
        dropped, score          per haplotype
        position, read_score    per haplotype, per read (-1 / 0: not placed)"""
    rc, o = place_call(windows, list_cap, grid_cap)
    _ffi.check(rc, 'mpn_realign_place_batch')
    res = [dict(hits=[], kmer=[], dropped=[], score=[], position=[], read_score=[]) for _ in windows]
    for k in range(o['n_hits'].value):
        h = o['hits'][k]
        res[h.window]['hits'].append((h.hap, h.read, h.start, h.mm, h.t, h.p))
    kmer = bytes(o['kmer'])
    gh = kp = pp = 0
    for w, r in zip(windows, res):
        n = len(w['seqs'])
        for hap in w['haplotypes']:
            r['kmer'].append(kmer[kp:kp + len(hap) - 31])
            r['dropped'].append(bool(o['dropped'][gh]))
            r['score'].append(int(o['hap_score'][gh]))
            r['position'].append([int(x) for x in o['position'][pp:pp + n]])
            r['read_score'].append([int(x) for x in o['score'][pp:pp + n]])
            kp += len(hap) - 31
            pp += n
            gh += 1
    return res, int(o['launches'].value)


def realign_batch(windows):
    """windows: dicts with the keyword arguments of realign_reads -> one list of (position, cigar) per window."""
    lib = _ffi.lib()
    nw = len(windows)
    if nw == 0:
        return []
    arr, keep, total = _window_array(windows)
    out_pos = (ct.c_int32 * max(total, 1))()
    out_cig = (ct.c_char_p * max(total, 1))()
    lib.mpn_realign_batch.restype = ct.c_int
    lib.mpn_realign_batch.argtypes = [ct.c_int32, ct.POINTER(Window), ct.POINTER(ct.c_int32), ct.POINTER(ct.c_char_p)]
    _ffi.check(lib.mpn_realign_batch(nw, arr, out_pos, out_cig), 'mpn_realign_batch')
    res, i = [], 0
    for w in windows:
        n = len(w['seqs'])
        res.append([(int(out_pos[i + j]), out_cig[i + j].decode()) for j in range(n)])
        i += n
    lib.mpn_realign_free_cigars.restype = None
    lib.mpn_realign_free_cigars.argtypes = [ct.POINTER(ct.c_char_p), ct.c_int64]
    lib.mpn_realign_free_cigars(out_cig, total)
    return res


# ---- de Bruijn graph consensus (include/mpn_dbg.h) ----------------------------------------
MAX_CONSENSUS = 500       # debruijn_graph.h: char *consensus[500]
SCRIPT_CONSENSUS = 200    # realign_illumina_reads.py: DBGPointer's `c_char_p * 200` -- the script sees the first 200 of the list
DBG_OK, DBG_NO_K, DBG_PATH_CAP, DBG_TABLE_FULL, DBG_HAP_FULL = range(5)


class DbgStrArr(ct.Structure):       # include/mpn_dbg.h mpn_dbg_str_arr
    _fields_ = [('consensus_size', ct.c_int), ('consensus', ct.c_char_p * MAX_CONSENSUS)]


class DbgWindow(ct.Structure):       # include/mpn_dbg.h mpn_dbg_window
    _fields_ = [('reference', ct.c_char_p), ('n_reads', ct.c_int32), ('reads', ct.POINTER(ct.c_char_p)),
                ('bad', ct.POINTER(ct.c_char_p))]     # (byte masks, passed as bytes objects)


class DbgResult(ct.Structure):       # include/mpn_dbg.h mpn_dbg_result
    _fields_ = [('status', ct.c_int32), ('k', ct.c_int32), ('n_haps', ct.c_int32), ('haps', ct.POINTER(ct.c_char_p))]


def get_consensus(ref, reads, bad_positions):
    """One window as the script passes it: reads joined with ',', per read its low-quality positions joined with ' ' (an iterable of
    ints, or the string itself) -> the sorted candidate haplotypes."""
    lib = _ffi.lib()
    lists = [b if isinstance(b, (str, bytes)) else ' '.join(str(int(x)) for x in b) for b in bad_positions]
    lib.get_consensus.restype = ct.POINTER(DbgStrArr)
    lib.get_consensus.argtypes = [ct.c_char_p, ct.c_char_p, ct.c_char_p, ct.c_int]
    p = lib.get_consensus(_b(ref), b','.join(_b(r) for r in reads), b','.join(_b(x) for x in lists), len(reads))
    if not p:
        raise _ffi.MpnError('get_consensus failed: ' + _ffi.last_error())
    n = p.contents.consensus_size
    out = [p.contents.consensus[i].decode() for i in range(n)]
    lib.free_consensus.restype = None
    lib.free_consensus.argtypes = [ct.POINTER(DbgStrArr), ct.c_int]
    lib.free_consensus(p, n)
    return out


def _dbg_window_array(windows):
    """-> (mpn_dbg_window array, the objects it points into)"""
    arr = (DbgWindow * max(len(windows), 1))()
    keep = []
    for i, w in enumerate(windows):
        n = len(w['reads'])
        reads = (ct.c_char_p * max(n, 1))(*[_b(r) for r in w['reads']])
        bad = None
        if w.get('bad') is not None:
            masks = []
            for r, pos in zip(w['reads'], w['bad']):
                m = None
                if pos:
                    m = bytearray(len(r) + 1)
                    for x in pos:
                        if 0 <= x < len(r):
                            m[x] = 1
                    m = bytes(m)
                masks.append(m)
            bad = (ct.c_char_p * max(n, 1))(*masks)
        ref = None if w['ref'] is None else _b(w['ref'])
        keep.append((reads, bad, ref))
        arr[i] = DbgWindow(ref, n, reads, bad)
    return arr, keep


def consensus_call(windows, table_cap=0, grid_cap=0, marshalled=None):
    """mpn_dbg_consensus_batch as it is.  windows: dicts with `ref`, `reads` and optionally `bad` (per read: None, or an iterable of
    low-quality positions).  marshalled: what _dbg_window_array(windows) gave, for a caller that times the two apart.
    -> (return code, [(status, k, haplotypes)], windows done again with larger tables)"""
    lib = _ffi.lib()
    nw = len(windows)
    arr, keep = marshalled or _dbg_window_array(windows)   # keep: alive until the call has returned
    res = (DbgResult * max(nw, 1))()
    redone = ct.c_int32(0)
    lib.mpn_dbg_consensus_batch.restype = ct.c_int
    lib.mpn_dbg_consensus_batch.argtypes = [ct.c_int32, ct.POINTER(DbgWindow), ct.c_int64, ct.c_int32, ct.POINTER(DbgResult),
                                            ct.POINTER(ct.c_int32)]
    rc = lib.mpn_dbg_consensus_batch(nw, arr, table_cap, grid_cap, res, ct.byref(redone))
    if rc != 0:
        return rc, [], 0
    out = [(r.status, r.k, [h.decode() for h in r.haps[:r.n_haps]]) for r in res[:nw]]
    lib.mpn_dbg_free_results.restype = None
    lib.mpn_dbg_free_results.argtypes = [ct.POINTER(DbgResult), ct.c_int32]
    lib.mpn_dbg_free_results(res, nw)
    return rc, out, int(redone.value)


def consensus_batch(windows, table_cap=0, grid_cap=0):
    """Many windows in one call -> [(haplotypes, k)], k = 0 where no k serves.  A window whose graph passes the workspace budget
    raises: nothing is returned cut short."""
    rc, out, _ = consensus_call(windows, table_cap, grid_cap)
    _ffi.check(rc, 'mpn_dbg_consensus_batch')
    for i, (status, _, _) in enumerate(out):
        if status in (DBG_TABLE_FULL, DBG_HAP_FULL):
            raise _ffi.MpnError('mpn_dbg_consensus_batch: the graph of window %d passes the workspace budget' % i)
    return [(haps, k) for _, k, haps in out]


def consensus_device_ms():
    lib = _ffi.lib()
    lib.mpn_dbg_last_device_ms.restype = None
    lib.mpn_dbg_last_device_ms.argtypes = [ct.POINTER(ct.c_double)]
    return _ffi.device_ms(lib.mpn_dbg_last_device_ms, 1)[0]


def realign_windows(windows):
    """The body of the script's window loop (realign_illumina_reads.py:543-629) for a batch.  A window is a dict:
        ref                   the window's own reference bases
        graph_reads, graph_bad  the reads that build its graph and, per read, their low-quality positions (or None)
        ref_prefix, ref_suffix  the reference bases on either side that the realigner aligns into (strings)
        seqs, positions, cigars, ref_start   the reads to realign, as realign_reads takes them
    Consensus per window; the first 200 of the list, as the script's binding slices it; a window with no consensus, with the
    reference alone, or with no reads to realign is skipped (None); the others go through realign_batch with the haplotypes
    ref_prefix + consensus + ref_suffix.  -> per window None or [(position, cigar)]."""
    cons = consensus_batch([dict(ref=w['ref'], reads=w['graph_reads'], bad=w.get('graph_bad')) for w in windows])
    todo, where = [], []
    for i, (w, (haps, _)) in enumerate(zip(windows, cons)):
        haps = haps[:SCRIPT_CONSENSUS]
        if not haps or haps == [w['ref']] or not w['seqs']:
            continue
        n = min(MAX_REGION_READS, len(w['seqs']))
        todo.append(dict(seqs=[s.upper() for s in w['seqs'][:n]], positions=list(w['positions'][:n]), cigars=list(w['cigars'][:n]),
                         reference=w['ref_prefix'] + w['ref'] + w['ref_suffix'],
                         haplotypes=[w['ref_prefix'] + h + w['ref_suffix'] for h in haps], ref_start=w['ref_start'],
                         ref_prefix=len(w['ref_prefix']), ref_suffix=len(w['ref_suffix'])))
        where.append(i)
    out = [None] * len(windows)
    for i, r in zip(where, realign_batch(todo)):
        out[i] = r
    return out
