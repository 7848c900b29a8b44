"""ctypes bindings for oracle/libmm2_oracle.so (TEST INFRASTRUCTURE ONLY; parity unpinned, see mm2_oracle.h)."""
import ctypes as ct
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


class MM128(ct.Structure):
    _fields_ = [('x', ct.c_uint64), ('y', ct.c_uint64)]


class Opt(ct.Structure):
    _fields_ = [('mid_occ_frac', ct.c_float), ('mid_occ', ct.c_int32), ('max_gap', ct.c_int32), ('bw', ct.c_int32),
                ('max_chain_skip', ct.c_int32), ('max_chain_iter', ct.c_int32), ('min_cnt', ct.c_int32),
                ('min_chain_score', ct.c_int32), ('mask_level', ct.c_float), ('pri_ratio', ct.c_float),
                ('best_n', ct.c_int32), ('max_join_long', ct.c_int32), ('max_join_short', ct.c_int32),
                ('min_join_flank_sc', ct.c_int32), ('min_join_flank_ratio', ct.c_float), ('a', ct.c_int32),
                ('b', ct.c_int32), ('q', ct.c_int32), ('e', ct.c_int32), ('q2', ct.c_int32), ('e2', ct.c_int32),
                ('sc_ambi', ct.c_int32), ('zdrop', ct.c_int32), ('zdrop_inv', ct.c_int32), ('end_bonus', ct.c_int32),
                ('min_dp_max', ct.c_int32), ('min_ksw_len', ct.c_int32), ('max_clip_ratio', ct.c_float),
                ('max_sw_mat', ct.c_int64), ('with_cigar', ct.c_int32), ('seed', ct.c_uint32)]


class Reg(ct.Structure):
    _fields_ = [(n, ct.c_int32) for n in ('id', 'cnt', 'rid', 'score', 'qs', 'qe', 'rs', 're', 'parent', 'subsc', 'as_',
                                          'mlen', 'blen', 'n_sub', 'score0')] + \
               [(n, ct.c_uint32) for n in ('mapq', 'split', 'rev', 'inv', 'sam_pri', 'split_inv', 'hash')] + \
               [(n, ct.c_int32) for n in ('has_p', 'dp_score', 'dp_max', 'dp_max2', 'n_ambi', 'n_cigar')] + \
               [('cigar', ct.POINTER(ct.c_uint32))]


class Ez(ct.Structure):
    _fields_ = [(n, ct.c_int32) for n in ('max', 'zdropped', 'max_q', 'max_t', 'mqe', 'mqe_t', 'mte', 'mte_q', 'score',
                                          'reach_end', 'n_cigar')] + [('cigar', ct.POINTER(ct.c_uint32))]


def lib():
    global _lib
    if _lib is None:
        L = ct.CDLL(os.path.join(HERE, 'libmm2_oracle.so'))
        L.mmo_opt_init.argtypes = [ct.POINTER(Opt)]
        L.mmo_idx_build.argtypes = [ct.c_int32, ct.POINTER(ct.c_char_p), ct.POINTER(ct.c_char_p), ct.c_void_p,
                                    ct.c_int, ct.c_int]
        L.mmo_idx_build.restype = ct.c_void_p
        L.mmo_idx_destroy.argtypes = [ct.c_void_p]
        L.mmo_idx_cal_max_occ.argtypes = [ct.c_void_p, ct.c_float]
        L.mmo_idx_cal_max_occ.restype = ct.c_int32
        L.mmo_free.argtypes = [ct.c_void_p]
        L.mmo_sketch.argtypes = [ct.c_char_p, ct.c_int32, ct.c_int, ct.c_int, ct.c_uint32, ct.POINTER(ct.c_void_p)]
        L.mmo_sketch.restype = ct.c_int64
        L.mmo_collect_anchors.argtypes = [ct.c_void_p, ct.c_int32, ct.c_void_p, ct.c_int64, ct.c_int32,
                                          ct.POINTER(ct.c_void_p), ct.POINTER(ct.c_int32)]
        L.mmo_collect_anchors.restype = ct.c_int64
        L.mmo_chain.argtypes = [ct.POINTER(Opt), ct.c_int64, ct.c_void_p, ct.POINTER(ct.c_int32),
                                ct.POINTER(ct.c_void_p), ct.POINTER(ct.c_void_p)]
        L.mmo_chain.restype = ct.c_int64
        L.mmo_map_read.argtypes = [ct.c_void_p, ct.POINTER(Opt), ct.c_char_p, ct.c_char_p, ct.c_int32,
                                   ct.POINTER(ct.c_int32), ct.POINTER(ct.c_int32)]
        L.mmo_map_read.restype = ct.POINTER(Reg)
        L.mmo_free_regs.argtypes = [ct.POINTER(Reg), ct.c_int32]
        L.mmo_write_paf.argtypes = [ct.c_void_p, ct.POINTER(Opt), ct.c_char_p, ct.c_int32, ct.POINTER(Reg), ct.c_int32,
                                    ct.c_int32, ct.c_char_p, ct.c_int64]
        L.mmo_write_paf.restype = ct.c_int64
        L.mmo_write_sam.argtypes = [ct.c_void_p, ct.POINTER(Opt), ct.c_char_p, ct.c_int32, ct.c_char_p, ct.POINTER(Reg), ct.c_int32,
                                    ct.c_int32, ct.c_char_p, ct.c_int64]
        L.mmo_write_sam.restype = ct.c_int64
        L.mmo_write_sam_q.argtypes = [ct.c_void_p, ct.POINTER(Opt), ct.c_char_p, ct.c_int32, ct.c_char_p, ct.c_char_p, ct.POINTER(Reg),
                                      ct.c_int32, ct.c_int32, ct.c_char_p, ct.c_int64]
        L.mmo_write_sam_q.restype = ct.c_int64
        L.mmo_idx_concat_names.argtypes = [ct.c_int32, ct.POINTER(ct.c_void_p)]
        L.mmo_idx_concat_names.restype = ct.c_void_p
        L.mmo_map_read_split.argtypes = [ct.c_int32, ct.POINTER(ct.c_void_p), ct.POINTER(Opt), ct.c_char_p, ct.c_char_p, ct.c_int32,
                                         ct.POINTER(ct.c_int32), ct.POINTER(ct.c_int32)]
        L.mmo_map_read_split.restype = ct.POINTER(Reg)
        L.mmo_extd2.argtypes = [ct.c_int, ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_int8, ct.c_int8, ct.c_int8, ct.c_int8,
                                ct.c_int8, ct.c_int8, ct.c_int8, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.POINTER(Ez)]
        L.mmo_fix_update.argtypes = [ct.c_void_p, ct.c_int32, ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p]
        L.mmo_fix_update.restype = None
        L.mmo_hits_from_chains.argtypes = [ct.POINTER(Opt), ct.c_int, ct.c_char_p, ct.c_int32, ct.c_int32, ct.c_void_p, ct.c_void_p,
                                           ct.POINTER(ct.c_int32), ct.POINTER(ct.c_int32)]
        L.mmo_hits_from_chains.restype = ct.POINTER(Reg)
        L.mmo_plan_hit.argtypes = [ct.POINTER(Opt), ct.c_int, ct.c_int32, ct.c_int32, ct.c_int32, ct.c_int32, ct.c_int32, ct.c_int32, ct.c_int32,
                                   ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_int32]
        L.mmo_plan_hit.restype = ct.c_int32
        L.mmo_stitch_hit.argtypes = [ct.POINTER(Opt), ct.c_int, ct.c_int32, ct.c_int32, ct.c_int32, ct.c_int32, ct.c_int32, ct.c_int32, ct.c_int32,
                                     ct.c_void_p, ct.c_int32, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p]
        L.mmo_stitch_hit.restype = ct.c_int32
        _lib = L
    return _lib


def default_opt(**kw):
    o = Opt()
    lib().mmo_opt_init(ct.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class Index:
    def __init__(self, genomes, k=15, w=10):
        """genomes: list of (name, uint8 ASCII numpy array or bytes)"""
        L = lib()
        n = len(genomes)
        self.names = [g[0] for g in genomes]
        self._seqs = [bytes(g[1]) if not isinstance(g[1], bytes) else g[1] for g in genomes]
        names = (ct.c_char_p * n)(*[x.encode() for x in self.names])
        seqs = (ct.c_char_p * n)(*self._seqs)
        lens = np.array([len(s) for s in self._seqs], dtype=np.int32)
        self.lens = lens
        self.h = L.mmo_idx_build(n, names, seqs, lens.ctypes.data, k, w)
        self.k, self.w = k, w

    def mid_occ(self, f=2e-4):
        return lib().mmo_idx_cal_max_occ(self.h, f)

    def close(self):
        if self.h:
            lib().mmo_idx_destroy(self.h)
            self.h = None


def _take128(ptr, n):
    if n == 0 or not ptr:
        return np.zeros((0, 2), dtype=np.uint64)
    arr = np.ctypeslib.as_array(ct.cast(ptr, ct.POINTER(ct.c_uint64)), shape=(n, 2)).copy()
    lib().mmo_free(ptr)
    return arr


def sketch(seq, w=10, k=15, rid=0):
    seq = bytes(seq)
    out = ct.c_void_p()
    n = lib().mmo_sketch(seq, len(seq), w, k, rid, ct.byref(out))
    return _take128(out, n)


def collect_anchors(idx, max_occ, mv, qlen):
    mv = np.ascontiguousarray(mv, dtype=np.uint64)
    out = ct.c_void_p()
    rep = ct.c_int32()
    n = lib().mmo_collect_anchors(idx.h, max_occ, mv.ctypes.data, len(mv), qlen, ct.byref(out), ct.byref(rep))
    return _take128(out, n), rep.value


def chain(opt, a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    n_u = ct.c_int32()
    u = ct.c_void_p()
    b = ct.c_void_p()
    n_b = lib().mmo_chain(ct.byref(opt), len(a), a.ctypes.data, ct.byref(n_u), ct.byref(u), ct.byref(b))
    if n_u.value == 0:
        return np.zeros(0, dtype=np.uint64), np.zeros((0, 2), dtype=np.uint64)
    uu = np.ctypeslib.as_array(ct.cast(u, ct.POINTER(ct.c_uint64)), shape=(n_u.value,)).copy()
    lib().mmo_free(u)
    return uu, _take128(b, n_b)


def map_read_sam(idx, opt, name, seq, qual=None):
    """-> SAM records of one read (minimap2 -a), unmapped reads included; qual: the read's quality string or None"""
    L = lib()
    seq = bytes(seq)
    n = ct.c_int32()
    rep = ct.c_int32()
    regs = L.mmo_map_read(idx.h, ct.byref(opt), name.encode(), seq, len(seq), ct.byref(n), ct.byref(rep))
    cap = (4096 + 2 * len(seq)) * max(n.value, 1) + sum(regs[i].n_cigar for i in range(n.value)) * 12 + 4096
    buf = ct.create_string_buffer(cap)
    nb = L.mmo_write_sam_q(idx.h, ct.byref(opt), name.encode(), len(seq), seq, bytes(qual) if qual is not None else None, regs, n.value,
                           rep.value, buf, cap)
    assert nb >= 0
    if n.value > 0:
        L.mmo_free_regs(regs, n.value)
    return buf.raw[:nb].decode()


class SplitIndex:
    """Index parts (minimap2 -I) + the concatenated name table the writers need."""

    def __init__(self, parts):
        self.parts = list(parts)
        self.arr = (ct.c_void_p * len(self.parts))(*[p.h for p in self.parts])
        self.names_h = lib().mmo_idx_concat_names(len(self.parts), self.arr)

    def map_read(self, opt, name, seq, sam=False, qual=None):
        """-> PAF lines (or SAM records) of one read mapped against every part and merged (--split-prefix)"""
        L = lib()
        seq = bytes(seq)
        n = ct.c_int32()
        rep = ct.c_int32()
        regs = L.mmo_map_read_split(len(self.parts), self.arr, ct.byref(opt), name.encode(), seq, len(seq), ct.byref(n), ct.byref(rep))
        cap = (4096 + 2 * len(seq)) * max(n.value, 1) + sum(regs[i].n_cigar for i in range(n.value)) * 12 + 4096
        buf = ct.create_string_buffer(cap)
        if sam:
            nb = L.mmo_write_sam_q(self.names_h, ct.byref(opt), name.encode(), len(seq), seq, bytes(qual) if qual is not None else None,
                                   regs, n.value, rep.value, buf, cap)
        else:
            nb = L.mmo_write_paf(self.names_h, ct.byref(opt), name.encode(), len(seq), regs, n.value, rep.value, buf, cap) if n.value else 0
        assert nb >= 0
        if n.value > 0:
            L.mmo_free_regs(regs, n.value)
        return buf.raw[:nb].decode()

    def close(self):
        if self.names_h:
            lib().mmo_idx_destroy(self.names_h)
            self.names_h = None


def map_read(idx, opt, name, seq):
    """-> (list of reg dicts, rep_len, paf text)"""
    L = lib()
    seq = bytes(seq)
    n = ct.c_int32()
    rep = ct.c_int32()
    regs = L.mmo_map_read(idx.h, ct.byref(opt), name.encode(), seq, len(seq), ct.byref(n), ct.byref(rep))
    out = []
    paf = ''
    if n.value > 0:
        cap = 4096 * n.value + sum(regs[i].n_cigar for i in range(n.value)) * 12 + 4096
        buf = ct.create_string_buffer(cap)
        nb = L.mmo_write_paf(idx.h, ct.byref(opt), name.encode(), len(seq), regs, n.value, rep.value, buf, cap)
        assert nb >= 0
        paf = buf.raw[:nb].decode()
        for i in range(n.value):
            r = regs[i]
            d = {f: getattr(r, f) for f, _ in Reg._fields_ if f != 'cigar'}
            d['cigar'] = [int(r.cigar[k]) for k in range(r.n_cigar)]
            out.append(d)
        L.mmo_free_regs(regs, n.value)
    return out, rep.value, paf


def extd2(query, target, sc_mch=2, sc_mis=-4, sc_n=-1, q=4, e=2, q2=24, e2=1, w=751, zdrop=400, end_bonus=-1, flag=0):
    query = np.ascontiguousarray(query, dtype=np.uint8)
    target = np.ascontiguousarray(target, dtype=np.uint8)
    ez = Ez()
    lib().mmo_extd2(len(query), query.ctypes.data, len(target), target.ctypes.data, sc_mch, sc_mis, sc_n, q, e, q2, e2,
                    w, zdrop, end_bonus, flag, ct.byref(ez))
    d = {f: getattr(ez, f) for f, _ in Ez._fields_ if f != 'cigar'}
    d['cigar'] = [int(ez.cigar[k]) for k in range(ez.n_cigar)]
    if ez.cigar:
        lib().mmo_free(ez.cigar)
    return d


def fix_update(cigar, q, t, a=2, b=4, sc_ambi=1, q_=4, e=2):
    """fix_cigar + update_extra of the oracle on one alignment: cigar words len << 4 | op, q / t 0..4 codes in alignment orientation
    -> dict(n_cigar, qshift, tshift, blen, mlen, n_ambi, dp_max, cigar)"""
    cig = np.ascontiguousarray(list(cigar) + [0], dtype=np.uint32)
    qq = np.ascontiguousarray(np.concatenate([np.asarray(q, dtype=np.uint8), np.zeros(8, np.uint8)]))
    tt = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.uint8), np.zeros(8, np.uint8)]))
    out = np.zeros(8, dtype=np.int32)
    lib().mmo_fix_update(cig.ctypes.data, len(cigar), qq.ctypes.data, tt.ctypes.data, a, b, sc_ambi, q_, e, out.ctypes.data)
    d = {k: int(out[j]) for j, k in enumerate(('n_cigar', 'qshift', 'tshift', 'blen', 'mlen', 'n_ambi', 'dp_max'))}
    d['cigar'] = cig[:d['n_cigar']].tolist()
    return d


def hits_from_chains(opt, k, name, qlen, u, a):
    """gen_regs -> set_parent -> select_sub -> join_long of the oracle on one read's chains: u uint64[n_u] (score << 32 | cnt), a uint64
    [n, 2] their anchors back to back, chains in the order of their first anchors -> (list of reg dicts, squeezed anchors uint64 [n_a, 2])"""
    u = np.ascontiguousarray(u, dtype=np.uint64)
    a = np.array(a, dtype=np.uint64).reshape(-1, 2)
    a = np.ascontiguousarray(np.concatenate([a, np.zeros((1, 2), np.uint64)]))
    n, n_a = ct.c_int32(), ct.c_int32()
    regs = lib().mmo_hits_from_chains(ct.byref(opt), k, name.encode() if name is not None else None, qlen, len(u), u.ctypes.data, a.ctypes.data,
                                      ct.byref(n), ct.byref(n_a))
    out = [{f: getattr(regs[i], f) for f, _ in Reg._fields_ if f != 'cigar'} for i in range(n.value)]
    if regs:
        lib().mmo_free(regs)
    return out, a[:n_a.value].copy()


PLAN_HIT_KEYS = ('as1', 'cnt1', 'qs', 'rs', 'qe', 're', 'qs0', 'qe0', 'rid', 'rev')
PLAN_WIN_KEYS = ('qs', 'qlen', 'ts', 'tlen', 'reversed', 'w', 'zdrop', 'end_bonus', 'flag', 'anchor', 'refused')


def plan_hit(opt, k, tlen, qlen, as_, cnt, mlen, split_inv, a):
    """the planning half of the oracle's align1 on the hit a[as_ : as_ + cnt] of one read's squeezed anchors a (uint64 [n_a, 2], changed
    in place: SEED_IGNORE marks) -> (dict of PLAN_HIT_KEYS, list of window dicts of PLAN_WIN_KEYS)"""
    assert a.dtype == np.uint64 and a.flags['C_CONTIGUOUS'] and a.ndim == 2 and a.shape[1] == 2
    out = np.zeros(10, dtype=np.int32)
    win = np.zeros((cnt + 2, 12), dtype=np.int32)
    n = lib().mmo_plan_hit(ct.byref(opt), k, tlen, qlen, as_, cnt, mlen, split_inv, len(a), a.ctypes.data, out.ctypes.data, win.ctypes.data,
                           len(win))
    assert n >= 0
    return ({key: int(v) for key, v in zip(PLAN_HIT_KEYS, out)},
            [{key: int(v) for key, v in zip(PLAN_WIN_KEYS, row)} for row in win[:n]])


STITCH_WIN_KEYS = ('kind', 'qs', 'ts', 'max', 'zdropped', 'max_q', 'max_t', 'mqe_t', 'score', 'reach_end', 'n_cigar', 'zcode')
STITCH_OUT_KEYS = ('n_ops', 'dp_score', 'rs1', 're1', 'qs1', 'qe1', 'has_p', 'dropped', 'drop_fill', 'drop_max_t', 'drop_max_q', 'split_n',
                   'r2_cnt', 'r2_as', 'r2_split_inv', 'mlen', 'blen', 'r2_mlen', 'r2_blen', 'consumed')


def stitch_hit(opt, k, tlen, qlen, as_, cnt, mlen, split_inv, a, wins, ops):
    """the second half of the oracle's align1 on the hit a[as_ : as_ + cnt] of one read's squeezed anchors a (uint64 [n_a, 2], SEED_IGNORE
    marks set in place), with recorded window results: wins = rows of STITCH_WIN_KEYS, ops = the windows' CIGAR ops back to back
    -> (dict of STITCH_OUT_KEYS, the appended CIGAR as a list of ints)"""
    assert a.dtype == np.uint64 and a.flags['C_CONTIGUOUS'] and a.ndim == 2 and a.shape[1] == 2
    win = np.ascontiguousarray(wins, dtype=np.int32).reshape(-1, 12)
    ops = np.ascontiguousarray(ops, dtype=np.uint32)
    assert int(win[:, 10].sum()) == len(ops)
    out = np.zeros(20, dtype=np.int32)
    cig = np.zeros(len(ops) + 1, dtype=np.uint32)
    rc = lib().mmo_stitch_hit(ct.byref(opt), k, tlen, qlen, as_, cnt, mlen, split_inv, len(a), a.ctypes.data, len(win), win.ctypes.data,
                              ops.ctypes.data, out.ctypes.data, cig.ctypes.data)
    assert rc == 0, 'the windows are not those align1 reaches'
    res = {key: int(v) for key, v in zip(STITCH_OUT_KEYS, out)}
    return res, [int(v) for v in cig[:res['n_ops']]]
