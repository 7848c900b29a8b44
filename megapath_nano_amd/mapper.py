"""ctypes wrapper over include/mpn_map.h: index build, stage entry points and the batch mapper."""
import ctypes as ct
import os

import numpy as np

from . import _ffi


class MapOpt(ct.Structure):
    _fields_ = [('k', ct.c_int32), ('w', ct.c_int32), ('mid_occ_frac', ct.c_float), ('mid_occ', ct.c_int32),
                ('max_gap', ct.c_int32), ('bw', ct.c_int32), ('max_chain_skip', ct.c_int32), ('max_chain_iter', ct.c_int32),
                ('min_cnt', ct.c_int32), ('min_chain_score', ct.c_int32), ('mask_level', ct.c_float),
                ('pri_ratio', ct.c_float), ('best_n', ct.c_int32), ('max_join_long', ct.c_int32),
                ('max_join_short', ct.c_int32), ('min_join_flank_sc', ct.c_int32), ('min_join_flank_ratio', ct.c_float),
                ('a', ct.c_int32), ('b', ct.c_int32), ('q', ct.c_int32), ('e', ct.c_int32), ('q2', ct.c_int32),
                ('e2', ct.c_int32), ('sc_ambi', ct.c_int32), ('zdrop', ct.c_int32), ('zdrop_inv', ct.c_int32),
                ('end_bonus', ct.c_int32), ('min_dp_max', ct.c_int32), ('min_ksw_len', ct.c_int32),
                ('max_clip_ratio', ct.c_float), ('max_sw_mat', ct.c_int64), ('with_cigar', ct.c_int32),
                ('seed', ct.c_uint32), ('host_threads', ct.c_int32), ('out_sam', ct.c_int32), ('out_tags', ct.c_int32)]


# MapOpt.out_tags bits (include/mpn_map.h MPN_TAG_*)
TAG_CS, TAG_CS_LONG, TAG_MD, TAG_EQX = 1, 2, 4, 8


COL_NAMES = ('read_idx', 'qs', 'qe', 'rev', 'rid', 'rs', 're', 'mlen', 'blen', 'mapq', 'nm', 'as_', 'primary')


class AlnCols(ct.Structure):
    _fields_ = [('cap', ct.c_int64), ('n_rows', ct.c_int64)] + [(n, ct.c_void_p) for n in COL_NAMES]


_bound = False


def _bind():
    global _bound
    lib = _ffi.lib()
    if not _bound:
        P = ct.c_void_p
        lib.mpn_map_opt_init.argtypes = [ct.POINTER(MapOpt)]
        lib.mpn_map_opt_init.restype = None
        lib.mpn_index_build.argtypes = [ct.c_int32, ct.POINTER(ct.c_char_p), ct.POINTER(ct.c_char_p), P, ct.c_int32, ct.c_int32]
        lib.mpn_index_build.restype = P
        lib.mpn_index_build_device.argtypes = [ct.c_int32, ct.POINTER(ct.c_char_p), P, P, P, ct.c_int32, ct.c_int32]
        lib.mpn_index_build_device.restype = P
        lib.mpn_index_destroy.argtypes = [P]
        lib.mpn_index_destroy.restype = None
        lib.mpn_index_n_minimizers.argtypes = [P]
        lib.mpn_index_n_minimizers.restype = ct.c_int64
        lib.mpn_index_n_keys.argtypes = [P]
        lib.mpn_index_n_keys.restype = ct.c_int64
        lib.mpn_index_mid_occ.argtypes = [P, ct.c_float]
        lib.mpn_index_mid_occ.restype = ct.c_int32
        lib.mpn_index_fetch_seq.argtypes = [P, ct.c_int32, ct.c_int64, ct.c_int64, ct.c_char_p]
        lib.mpn_index_fetch_seq.restype = ct.c_int64
        lib.mpn_index_export.argtypes = [P, P, P, P]
        lib.mpn_index_export.restype = ct.c_int
        lib.mpn_sam_header.argtypes = [P, ct.c_char_p, ct.c_char_p, ct.c_int64]
        lib.mpn_sam_header.restype = ct.c_int64
        lib.mpn_index_save.argtypes = [P, ct.c_char_p]
        lib.mpn_index_save.restype = ct.c_int
        lib.mpn_index_load.argtypes = [ct.c_char_p]
        lib.mpn_index_load.restype = P
        lib.mpn_index_save_append.argtypes = [P, ct.c_char_p]
        lib.mpn_index_save_append.restype = ct.c_int
        lib.mpn_index_load_at.argtypes = [ct.c_char_p, ct.c_int64, ct.POINTER(ct.c_int64)]
        lib.mpn_index_load_at.restype = P
        for fn in ('mpn_index_n_seq', 'mpn_index_k', 'mpn_index_w'):
            getattr(lib, fn).argtypes = [P]
            getattr(lib, fn).restype = ct.c_int32
        lib.mpn_index_seq_len.argtypes = [P, ct.c_int32]
        lib.mpn_index_seq_len.restype = ct.c_int32
        lib.mpn_index_seq_name.argtypes = [P, ct.c_int32, ct.c_char_p, ct.c_int32]
        lib.mpn_index_seq_name.restype = ct.c_int32
        lib.mpn_sketch_batch.argtypes = [ct.c_int32, P, P, P, ct.c_int32, ct.c_int32, P, P, ct.c_int64]
        lib.mpn_sketch_batch.restype = ct.c_int64
        lib.mpn_seed_chain_batch.argtypes = [P, ct.POINTER(MapOpt), ct.c_int32, P, P, P, P, P, P, P, ct.c_int64, P, P, ct.c_int64]
        lib.mpn_seed_chain_batch.restype = ct.c_int
        if True:
            lib.mpn_map_batch.argtypes = [P, ct.POINTER(MapOpt), ct.c_int32, ct.POINTER(ct.c_char_p), P, P, P, P, ct.c_int64]
            lib.mpn_map_batch.restype = ct.c_int64
        lib.mpn_map_batch_ex.argtypes = [P, ct.POINTER(MapOpt), ct.c_int32, ct.POINTER(ct.c_char_p), P, P, P, P, P, P, P,
                                         ct.c_int64, ct.POINTER(AlnCols)]
        lib.mpn_map_batch_ex.restype = ct.c_int64
        lib.mpn_map_batch_q.argtypes = [P, ct.POINTER(MapOpt), ct.c_int32, ct.POINTER(ct.c_char_p), P, P, P, P, P, P, P, P,
                                        ct.c_int64, ct.POINTER(AlnCols)]
        lib.mpn_map_batch_q.restype = ct.c_int64
        lib.mpn_hits_create.argtypes = [ct.c_int32]
        lib.mpn_hits_create.restype = P
        lib.mpn_hits_destroy.argtypes = [P]
        lib.mpn_hits_destroy.restype = None
        for fn in ('mpn_hits_n_seq', 'mpn_hits_n_parts'):
            getattr(lib, fn).argtypes = [P]
            getattr(lib, fn).restype = ct.c_int32
        lib.mpn_hits_seq_len.argtypes = [P, ct.c_int32]
        lib.mpn_hits_seq_len.restype = ct.c_int32
        lib.mpn_hits_seq_name.argtypes = [P, ct.c_int32, ct.c_char_p, ct.c_int32]
        lib.mpn_hits_seq_name.restype = ct.c_int32
        lib.mpn_hits_sam_header.argtypes = [P, ct.c_char_p, ct.c_char_p, ct.c_int64]
        lib.mpn_hits_sam_header.restype = ct.c_int64
        lib.mpn_map_batch_part.argtypes = [P, ct.POINTER(MapOpt), ct.c_int32, ct.POINTER(ct.c_char_p), P, P, P, P, P, P, P]
        lib.mpn_map_batch_part.restype = ct.c_int
        lib.mpn_map_batch_parts.argtypes = [ct.POINTER(ct.c_void_p), ct.c_int32, ct.POINTER(MapOpt), ct.c_int32, ct.POINTER(ct.c_char_p), P, P, P, P, P, P, P]
        lib.mpn_map_batch_parts.restype = ct.c_int
        lib.mpn_hits_set_text.argtypes = [P, ct.c_int32]
        lib.mpn_hits_set_text.restype = None
        lib.mpn_hits_export.argtypes = [P, ct.c_int32, ct.c_int32, P, ct.c_int64]
        lib.mpn_hits_export.restype = ct.c_int64
        lib.mpn_hits_import.argtypes = [P, P, ct.c_int64, ct.c_int32, ct.c_int32, ct.POINTER(ct.c_char_p), P]
        lib.mpn_hits_import.restype = ct.c_int
        lib.mpn_index_part_info.argtypes = [ct.c_char_p, ct.c_int64, ct.POINTER(ct.c_int64), ct.POINTER(ct.c_int64)]
        lib.mpn_index_part_info.restype = ct.c_int32
        lib.mpn_hits_finish.argtypes = [P, ct.POINTER(MapOpt), ct.c_int32, ct.POINTER(ct.c_char_p), P, P, P, P, P, ct.c_int64,
                                        ct.POINTER(AlnCols)]
        lib.mpn_hits_finish.restype = ct.c_int64
        lib.mpn_map_fetch_sam.argtypes = [ct.c_char_p, ct.c_int64]
        lib.mpn_map_fetch_sam.restype = ct.c_int64
        lib.mpn_map_fetch_cols.argtypes = [ct.POINTER(AlnCols)]
        lib.mpn_map_fetch_cols.restype = ct.c_int64
        lib.mpn_map_fetch_text.argtypes = [ct.c_char_p, ct.c_int64]
        lib.mpn_map_fetch_text.restype = ct.c_int64
        lib.mpn_ext_dp_batch.argtypes = [ct.POINTER(MapOpt), ct.c_int32, P, P, P, P, P, P, P, P, P, P, ct.c_int32, P, P, ct.c_int64, P]
        lib.mpn_ext_dp_batch.restype = ct.c_int
        lib.mpn_aln_tags_batch.argtypes = [ct.c_int32, P, P, P, P, P, P, P, P, P, P, P, P, P, ct.c_int32, P, ct.c_int64, P, P, ct.c_int64, P,
                                           P, ct.c_int64, P]
        lib.mpn_aln_tags_batch.restype = ct.c_int
        lib.mpn_aln_finish_batch.argtypes = [ct.POINTER(MapOpt), ct.c_int32, P, P, P, P, P, P, P, P, P, P, P, P, P, ct.c_int32, P, P]
        lib.mpn_aln_finish_batch.restype = ct.c_int
        lib.mpn_hit_select_batch.argtypes = [ct.POINTER(MapOpt), ct.c_int32, ct.c_int32, P, ct.POINTER(ct.c_char_p), P, P, P, P, P, P, P, P, P, P,
                                             ct.c_int32, ct.c_int32, ct.c_int32, P, P, P, P]
        lib.mpn_hit_select_batch.restype = ct.c_int
        lib.mpn_ext_plan_batch.argtypes = [ct.POINTER(MapOpt), ct.c_int32, ct.c_int32, P, ct.c_int32, P, P, P, P, P, P, P, P, ct.c_int32, P, ct.c_int64,
                                           P, P, P]
        lib.mpn_ext_plan_batch.restype = ct.c_int
        lib.mpn_stitch_batch.argtypes = [ct.c_int32, P, P, ct.c_int32, P, ct.c_int64, P, P, ct.c_int64, P, ct.c_int32, ct.c_int32, P, ct.c_int64, P, P,
                                         P, P]
        lib.mpn_stitch_batch.restype = ct.c_int
        lib.mpn_chain_batch.argtypes = [ct.POINTER(MapOpt), ct.c_int32, P, P, ct.c_int32, ct.c_int32, ct.c_int32, P, P, P, P, ct.c_int64, P, ct.c_int64]
        lib.mpn_chain_batch.restype = ct.c_int
        lib.mpn_seed_anchors_batch.argtypes = [ct.c_int32, ct.c_int32, P, ct.c_int64, P, P, P, ct.POINTER(MapOpt), ct.c_int32, P, P, P, ct.c_int64,
                                               ct.c_int32, ct.c_int32, P, P, P, P, P, ct.c_int64, P]
        lib.mpn_seed_anchors_batch.restype = ct.c_int
        lib.mpn_map_last_stats.argtypes = [P]
        lib.mpn_map_last_stats.restype = None
        lib.mpn_reads_split_plan.argtypes = [ct.c_int32, P, ct.c_int64, P, P, ct.c_int32, ct.c_int64, P, P, P, P, P, P]
        lib.mpn_reads_split_plan.restype = ct.c_int
        lib.mpn_reads_split_gather.argtypes = [ct.c_int32, P, P, ct.c_int64, P, P, ct.c_int32, ct.c_int64, P, P, ct.c_int64, P, P, ct.c_int64, P, P]
        lib.mpn_reads_split_gather.restype = ct.c_int
        lib.mpn_reads_split_last_ns.argtypes = [ct.c_int32]
        lib.mpn_reads_split_last_ns.restype = ct.c_int64
        lib.mpn_map_last_stats_ex.argtypes = [P, ct.c_int32]
        lib.mpn_map_last_stats_ex.restype = ct.c_int32
        _bound = True
    return lib


def default_opt(**kw):
    o = MapOpt()
    _bind().mpn_map_opt_init(ct.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def pack_seqs(seqs):
    """list of bytes / uint8 arrays -> (concatenated uint8 buffer, offsets int64, lengths int32)"""
    lens = np.array([len(s) for s in seqs], dtype=np.int32)
    off = np.zeros(len(seqs), dtype=np.int64)
    if len(seqs) > 1:
        off[1:] = np.cumsum(lens[:-1].astype(np.int64))
    total = int(lens.astype(np.int64).sum())
    buf = np.zeros(total + 16, dtype=np.uint8)
    for s, o in zip(seqs, off):
        a = np.frombuffer(s, dtype=np.uint8) if isinstance(s, (bytes, bytearray)) else np.asarray(s, dtype=np.uint8)
        buf[o:o + len(a)] = a
    return buf, off, lens


class Index:
    """Target sequences + minimizer index resident in HBM (mpn_index_build), or loaded from a file written by save()."""

    MAGIC = b'MPNIDX01'

    def __init__(self, genomes, k=15, w=10):
        lib = _bind()
        n = len(genomes)
        self.names = [g[0] for g in genomes]
        seqs_b = [bytes(g[1]) if not isinstance(g[1], bytes) else g[1] for g in genomes]  # alive for the call only
        self.lens = np.array([len(s) for s in seqs_b], dtype=np.int32)
        names = (ct.c_char_p * n)(*[x.encode() for x in self.names])
        seqs = (ct.c_char_p * n)(*seqs_b)
        self.k, self.w = k, w
        self.h = lib.mpn_index_build(n, names, seqs, self.lens.ctypes.data, k, w)
        if not self.h:
            raise _ffi.MpnError('mpn_index_build failed: ' + _ffi.hint(_ffi.last_error()))

    @classmethod
    def from_device(cls, names, d_seqs_ptr, lens, k=15, w=10):
        """Index of targets that are resident in HBM as concatenated ASCII (device pointer; target i at sum(lens[:i]))."""
        lib = _bind()
        self = cls.__new__(cls)
        n = len(names)
        self.names = list(names)
        self.lens = np.ascontiguousarray(lens, dtype=np.int32)
        off = np.zeros(n + 1, dtype=np.int64)
        off[1:] = np.cumsum(self.lens.astype(np.int64))
        cn = (ct.c_char_p * n)(*[x.encode() for x in self.names])
        self.k, self.w = k, w
        self.h = lib.mpn_index_build_device(n, cn, d_seqs_ptr, off.ctypes.data, self.lens.ctypes.data, k, w)
        if not self.h:
            raise _ffi.MpnError('mpn_index_build_device failed: ' + _ffi.hint(_ffi.last_error()))
        return self

    def sam_header(self, cmdline=None):
        cap = 64 * len(self.names) + sum(len(n) for n in self.names) + 4096 + (len(cmdline) if cmdline else 0)
        buf = ct.create_string_buffer(cap)
        r = _bind().mpn_sam_header(self.h, cmdline.encode() if cmdline else None, buf, cap)
        if r < 0:
            raise _ffi.MpnError(f'mpn_sam_header rc={r}')
        return buf.raw[:r].decode()

    def save(self, path, append=False):
        """Persistent form (minimap2 `-d FILE`): load() gives back an index that maps identically.  append=True adds this
        index as a further PART of the target set the file holds (minimap2 dumps all parts of a -I split into the one file)."""
        lib = _bind()
        _ffi.check((lib.mpn_index_save_append if append else lib.mpn_index_save)(self.h, os.fsencode(path)), 'mpn_index_save')

    @classmethod
    def load(cls, path):
        """The (first) index part of a saved file."""
        idx, _ = cls.load_at(path, 0)
        return idx

    @classmethod
    def iter_parts(cls, path):
        """The index parts of a saved file, one at a time (the caller closes each before asking for the next)."""
        off = 0
        while off >= 0:
            idx, off = cls.load_at(path, off)
            yield idx

    @classmethod
    def load_at(cls, path, offset):
        """-> (the part that starts at byte `offset`, offset of the next part or -1)"""
        lib = _bind()
        nxt = ct.c_int64(-1)
        h = lib.mpn_index_load_at(os.fsencode(path), int(offset), ct.byref(nxt))
        if not h:
            raise _ffi.MpnError('mpn_index_load failed: ' + _ffi.last_error())
        self = cls._from_handle(h)
        return self, int(nxt.value)

    @classmethod
    def part_info(cls, path):
        """Every part of a saved file without loading any: -> list of (offset, n_seq, bases), in file (= target) order."""
        lib = _bind()
        out, off = [], 0
        while off >= 0:
            bases, nxt = ct.c_int64(0), ct.c_int64(-1)
            n = lib.mpn_index_part_info(os.fsencode(path), int(off), ct.byref(bases), ct.byref(nxt))
            if n < 0:
                raise _ffi.MpnError('mpn_index_part_info failed: ' + _ffi.last_error())
            out.append((off, int(n), int(bases.value)))
            off = int(nxt.value)
        return out

    @classmethod
    def _from_handle(cls, h):
        lib = _bind()
        self = cls.__new__(cls)
        self.h = h
        n = lib.mpn_index_n_seq(h)
        buf = ct.create_string_buffer(1 << 16)
        self.names, lens = [], []
        for i in range(n):
            lib.mpn_index_seq_name(h, i, buf, len(buf))
            self.names.append(buf.value.decode())
            lens.append(lib.mpn_index_seq_len(h, i))
        self.lens = np.array(lens, dtype=np.int32)
        self.k, self.w = lib.mpn_index_k(h), lib.mpn_index_w(h)
        return self

    @classmethod
    def is_index_file(cls, path):
        try:
            with open(path, 'rb') as f:
                return f.read(8) == cls.MAGIC
        except OSError:
            return False

    @property
    def n_minimizers(self):
        return _bind().mpn_index_n_minimizers(self.h)

    @property
    def n_keys(self):
        return _bind().mpn_index_n_keys(self.h)

    def mid_occ(self, f=2e-4):
        return _bind().mpn_index_mid_occ(self.h, f)

    def fetch_seq(self, i, start, length):
        """bases [start, start+length) of target i as bytes, decoded from the packed targets in HBM"""
        buf = ct.create_string_buffer(int(length) + 1)
        r = _bind().mpn_index_fetch_seq(self.h, int(i), int(start), int(length), buf)
        if r < 0:
            raise _ffi.MpnError(f'mpn_index_fetch_seq rc={r}: {_ffi.last_error()}')
        return buf.raw[:r]

    def export(self):
        keys = np.zeros(self.n_keys, dtype=np.uint64)
        key_off = np.zeros(self.n_keys + 1, dtype=np.int64)
        pos = np.zeros(self.n_minimizers, dtype=np.uint64)
        _ffi.check(_bind().mpn_index_export(self.h, keys.ctypes.data, key_off.ctypes.data, pos.ctypes.data), 'mpn_index_export')
        return keys, key_off, pos

    def close(self):
        if self.h:
            _bind().mpn_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sketch_batch(seqs, k=15, w=10):
    """-> list of (n_i, 2) uint64 arrays, one per sequence"""
    lib = _bind()
    buf, off, lens = pack_seqs(seqs)
    n = len(seqs)
    mz_off = np.zeros(n + 1, dtype=np.int64)
    cap = int(lens.astype(np.int64).sum()) + 16
    mz = np.zeros((cap, 2), dtype=np.uint64)
    r = lib.mpn_sketch_batch(n, buf.ctypes.data, off.ctypes.data, lens.ctypes.data, k, w, mz_off.ctypes.data, mz.ctypes.data, cap)
    if r < 0:
        raise _ffi.MpnError(f'mpn_sketch_batch rc={r}: {_ffi.last_error()}')
    return [mz[mz_off[i]:mz_off[i + 1]].copy() for i in range(n)]


def seed_chain_batch(idx, opt, seqs):
    """-> list of dict(n_anchor, rep_len, u (uint64[n_chain]), b ((n,2) uint64)) per read"""
    lib = _bind()
    buf, off, lens = pack_seqs(seqs)
    n = len(seqs)
    n_anchor = np.zeros(n, dtype=np.int64)
    rep_len = np.zeros(n, dtype=np.int32)
    chain_off = np.zeros(n + 1, dtype=np.int64)
    anchor_off = np.zeros(n + 1, dtype=np.int64)
    u_cap, b_cap = 1 << 16, 1 << 20
    while True:
        u = np.zeros(u_cap, dtype=np.uint64)
        b = np.zeros((b_cap, 2), dtype=np.uint64)
        rc = lib.mpn_seed_chain_batch(idx.h, ct.byref(opt), n, buf.ctypes.data, off.ctypes.data, lens.ctypes.data,
                                      n_anchor.ctypes.data, rep_len.ctypes.data, chain_off.ctypes.data, u.ctypes.data, u_cap,
                                      anchor_off.ctypes.data, b.ctypes.data, b_cap)
        if rc == -3:
            u_cap, b_cap = max(u_cap, int(chain_off[n]) + 1), max(b_cap, int(anchor_off[n]) + 1)
            continue
        _ffi.check(rc, 'mpn_seed_chain_batch')
        break
    return [dict(n_anchor=int(n_anchor[i]), rep_len=int(rep_len[i]), u=u[chain_off[i]:chain_off[i + 1]].copy(),
                 b=b[anchor_off[i]:anchor_off[i + 1]].copy()) for i in range(n)]


CHAIN_REC_KEYS = ('fx', 'fy', 'lx', 'ly', 'mlen', 'blen')


def chain_batch(opt, anchor_off, anchors, chain_item=0, bt_par_min=0, grid_cap=0):
    """The chaining stage on arbitrary sorted anchors (mpn_chain_batch).  anchor_off[n + 1] into anchors uint64 [total, 2] (x, y), every
    read's anchors in ascending (x, y) order.  chain_item, bt_par_min: 0 = the mapper's values (MPN_CHAIN_ITEM, MPN_BT_PAR_MIN);
    grid_cap: 0 = the mapper's grids, else at most that many blocks per launch.  -> list of dict(n_chain, n_chained, u (uint64[n_chain]),
    b ((n_chained, 2) uint64), recs (int64 [n_chain, 6] in CHAIN_REC_KEYS order, x / y words bit for bit)) per read, chains in the order
    of seed_chain_batch."""
    lib = _bind()
    anchor_off = np.ascontiguousarray(anchor_off, dtype=np.int64)
    anchors = np.ascontiguousarray(anchors, dtype=np.uint64).reshape(-1, 2)
    n = len(anchor_off) - 1
    assert n >= 0 and (n == 0 or len(anchors) >= int(anchor_off[-1]))
    n_chain = np.zeros(n + 1, dtype=np.int32)
    n_chained = np.zeros(n + 1, dtype=np.int64)
    u_cap, b_cap = len(anchors) // 4 + 16, len(anchors) + 16
    while True:
        u = np.zeros(u_cap, dtype=np.uint64)
        recs = np.zeros((u_cap, 6), dtype=np.int64)
        b = np.zeros((b_cap, 2), dtype=np.uint64)
        rc = lib.mpn_chain_batch(ct.byref(opt), n, anchor_off.ctypes.data, anchors.ctypes.data, int(chain_item), int(bt_par_min), int(grid_cap),
                                 n_chain.ctypes.data, n_chained.ctypes.data, u.ctypes.data, recs.ctypes.data, u_cap, b.ctypes.data, b_cap)
        if rc == -3:
            u_cap, b_cap = max(u_cap, int(n_chain.sum()) + 1), max(b_cap, int(n_chained.sum()) + 1)
            continue
        _ffi.check(rc, 'mpn_chain_batch')
        break
    c_off = np.concatenate([[0], np.cumsum(n_chain[:n].astype(np.int64))])
    b_off = np.concatenate([[0], np.cumsum(n_chained[:n])])
    return [dict(n_chain=int(n_chain[i]), n_chained=int(n_chained[i]), u=u[c_off[i]:c_off[i + 1]].copy(), b=b[b_off[i]:b_off[i + 1]].copy(),
                 recs=recs[c_off[i]:c_off[i + 1]].copy()) for i in range(n)]


def seed_anchors_batch(k, lens, keys, key_off, pos, opt, mz_off, mz, seq_len, flt_round2=0, flt_wgs=0, grid_cap=0, cap=None):
    """The seed half of the stage on a made index and made minimizers (mpn_seed_anchors_batch): hit lookup, stray-hit filter, emission
    and sort.  lens: the targets' lengths; keys, key_off, pos: the index as Index.export() gives it; mz_off[n + 1] into mz uint64
    [total, 2] in the sketch's layout; seq_len[n].  Of opt mid_occ (explicit), min_cnt and max_gap are read.  flt_round2, flt_wgs,
    grid_cap: 0 = the mapper's values.  cap: room for that many anchors (None: grown as needed; else MpnError -3 if too small, with
    the partial result as its .partial).  -> (list of dict(n_anchor, rep_len, span_sum, a ((n, 2) uint64)) per read,
    dict(n_list=(3 counts), walked=hits the filter walked))."""
    lib = _bind()
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    key_off = np.ascontiguousarray(key_off, dtype=np.int64)
    pos = np.ascontiguousarray(pos, dtype=np.uint64)
    mz_off = np.ascontiguousarray(mz_off, dtype=np.int64)
    mz = np.ascontiguousarray(mz, dtype=np.uint64).reshape(-1, 2)
    seq_len = np.ascontiguousarray(seq_len, dtype=np.int32)
    n = len(mz_off) - 1
    assert n >= 0 and len(seq_len) == n and len(key_off) == len(keys) + 1
    n_anchor = np.zeros(n + 1, dtype=np.int64)
    rep_len = np.zeros(n + 1, dtype=np.int32)
    span_sum = np.zeros(n + 1, dtype=np.int64)
    anchor_off = np.zeros(n + 1, dtype=np.int64)
    counts = np.zeros(4, dtype=np.int64)
    a_cap = (1 << 16) if cap is None else int(cap)
    while True:
        a = np.zeros((max(a_cap, 1), 2), dtype=np.uint64)
        rc = lib.mpn_seed_anchors_batch(int(k), len(lens), lens.ctypes.data, len(keys), keys.ctypes.data, key_off.ctypes.data, pos.ctypes.data,
                                        ct.byref(opt), n, mz_off.ctypes.data, mz.ctypes.data, seq_len.ctypes.data, int(flt_round2), int(flt_wgs),
                                        int(grid_cap), n_anchor.ctypes.data, rep_len.ctypes.data, span_sum.ctypes.data, anchor_off.ctypes.data,
                                        a.ctypes.data, a_cap, counts.ctypes.data)
        if rc == -3 and cap is None:
            a_cap = int(anchor_off[n]) + 1
            continue
        if rc == -3:
            e = _ffi.MpnError('mpn_seed_anchors_batch rc=-3: room for %d anchors, %d needed' % (a_cap, int(anchor_off[n])))
            e.partial = dict(n_anchor=n_anchor[:n].copy(), anchor_off=anchor_off.copy())
            raise e
        _ffi.check(rc, 'mpn_seed_anchors_batch')
        break
    reads = [dict(n_anchor=int(n_anchor[i]), rep_len=int(rep_len[i]), span_sum=int(span_sum[i]), a=a[anchor_off[i]:anchor_off[i + 1]].copy())
             for i in range(n)]
    return reads, dict(n_list=tuple(int(v) for v in counts[:3]), walked=int(counts[3]))


def map_batch(idx, opt, names, seqs):
    """-> PAF text of the whole batch (reads in input order)"""
    packed = PackedReads(names, seqs)
    return map_batch_ex(idx, opt, packed, want_paf=True, want_cols=False)[0]


class PackedReads:
    """Reads packed for mpn_map_batch_ex; optionally also resident in HBM (torch uint8/int64/int32 tensors)."""

    def __init__(self, names, seqs, device=None, quals=None):
        """quals: per read a quality string of the read's length, or None (then the SAM QUAL column is '*')"""
        self.n = len(seqs)
        self.names = list(names)
        self.buf, self.off, self.lens = pack_seqs(seqs)
        self.qbuf = None
        if quals is not None and any(q is not None for q in quals):
            # reads without qualities in a batch that has some: the '*' cannot be mixed per read, they get '!' (Phred 0)
            self.qbuf = pack_seqs([q if q is not None else b'!' * int(l) for q, l in zip(quals, self.lens)])[0]
        self._finish(device)

    @classmethod
    def from_arrays(cls, names, buf, off, lens, dev=None, qbuf=None):
        """buf: concatenated ASCII (uint8, padded to a 4-byte multiple past the last base), off int64, lens int32 (host
        numpy); dev: the same three as torch tensors already resident in HBM, or None; qbuf: qualities laid out like buf, or None."""
        self = cls.__new__(cls)
        self.n = len(lens)
        self.names = list(names)
        self.buf = np.ascontiguousarray(buf, dtype=np.uint8)
        self.off = np.ascontiguousarray(off, dtype=np.int64)
        self.lens = np.ascontiguousarray(lens, dtype=np.int32)
        self.qbuf = None if qbuf is None else np.ascontiguousarray(qbuf, dtype=np.uint8)
        self._finish(None)
        self.dev = dev
        return self

    def _finish(self, device):
        self.cnames = (ct.c_char_p * self.n)(*[x.encode() for x in self.names])
        self.bases = int(self.lens.astype(np.int64).sum())
        self.dev = None
        if device is not None:
            import torch
            self.dev = (torch.from_numpy(self.buf).to(device), torch.from_numpy(self.off).to(device),
                        torch.from_numpy(self.lens).to(device))
            torch.cuda.synchronize(device)

    def seq(self, i):
        return self.buf[self.off[i]:self.off[i] + self.lens[i]]

    def sub(self, lo, hi):
        """Reads [lo, hi) as a PackedReads of their own: names, bases, qualities and (when this batch has one) the device copy,
        repacked from offset 0 like a batch of just these reads."""
        lo, hi = int(lo), int(hi)
        assert 0 <= lo <= hi <= self.n, (lo, hi, self.n)
        a = int(self.off[lo]) if hi > lo else 0
        b = int(self.off[hi - 1] + self.lens[hi - 1]) if hi > lo else 0
        out = self.__class__.__new__(self.__class__)
        out.n = hi - lo
        out.names = self.names[lo:hi]
        out.buf = np.zeros(b - a + 16, dtype=np.uint8)
        out.buf[:b - a] = self.buf[a:b]
        out.off = (self.off[lo:hi] - a).astype(np.int64)
        out.lens = self.lens[lo:hi].copy()
        out.qbuf = None
        if getattr(self, 'qbuf', None) is not None:
            out.qbuf = np.zeros(b - a + 16, dtype=np.uint8)
            out.qbuf[:b - a] = self.qbuf[a:b]
        out._finish(self.dev[0].device if self.dev is not None else None)
        return out


# ---- regrouping a batch by (read, group) pairs: include/mpn_reads.h ---------------------------------------------------------------
SPLIT_ALIGN = 16
PLAN_KEYS = ('n_out', 'out_read', 'group_first', 'out_off', 'group_byte', 'out_bytes')


def _split_args(lens, mem_read, mem_group):
    c = lambda v, t: np.ascontiguousarray(v, dtype=t)  # noqa: E731
    lens, mem_read, mem_group = c(lens, np.int32), c(mem_read, np.int32), c(mem_group, np.int32)
    if mem_read.shape != mem_group.shape or mem_read.ndim != 1:
        raise ValueError('mem_read and mem_group: two 1-d arrays of one length')
    return lens, mem_read, mem_group


def host_split_plan(lens, mem_read, mem_group, n_groups):
    """The plan of a split as a numpy statement (what mpn_reads_split_plan computes on the device) -> dict of PLAN_KEYS."""
    lens, mem_read, mem_group = _split_args(lens, mem_read, mem_group)
    n, n_groups = len(lens), int(n_groups)
    if (lens < 0).any() or ((mem_read < 0) | (mem_read >= n)).any() or ((mem_group < 0) | (mem_group >= n_groups)).any():
        raise ValueError('split: a negative length, or a pair outside [0, n) x [0, n_groups)')
    key = np.unique(mem_group.astype(np.int64) << 32 | mem_read.astype(np.int64))     # sorted by (group, read), a pair once
    out_group, out_read = (key >> 32).astype(np.int64), (key & 0xffffffff).astype(np.int32)
    group_first = np.searchsorted(out_group, np.arange(n_groups + 1)).astype(np.int64)
    out_len = lens[out_read].astype(np.int64)
    g_bytes = np.bincount(out_group, weights=None if not len(key) else out_len, minlength=n_groups).astype(np.int64) if n_groups else np.zeros(0, np.int64)
    group_byte = np.zeros(n_groups + 1, dtype=np.int64)
    group_byte[1:] = np.cumsum((g_bytes + SPLIT_ALIGN - 1) // SPLIT_ALIGN * SPLIT_ALIGN)
    before = np.cumsum(out_len) - out_len                                               # bytes of all earlier output reads
    out_off = group_byte[out_group] + before - (before[group_first[out_group]] if len(key) else 0)
    return dict(n_out=len(key), out_read=out_read, group_first=group_first, out_off=out_off.astype(np.int64), group_byte=group_byte,
                out_bytes=int(group_byte[n_groups]) + SPLIT_ALIGN)


def host_split_gather(plan, buf, off, lens, qbuf=None):
    """-> (bases uint8[out_bytes], qualities or None): the reads of the plan copied into place, every other byte 0"""
    outs = []
    for src in (buf, qbuf):
        if src is None:
            outs.append(None)
            continue
        o = np.zeros(plan['out_bytes'], dtype=np.uint8)
        for r, d in zip(plan['out_read'], plan['out_off']):
            o[d:d + lens[r]] = src[off[r]:off[r] + lens[r]]
        outs.append(o)
    return outs[0], outs[1]


def host_split_reads(buf, off, lens, mem_read, mem_group, n_groups, qbuf=None):
    """Reads regrouped by (read, group) pairs with nanosplit's semantics, on the host -> the plan's dict plus 'seqs' and 'quals'."""
    plan = host_split_plan(lens, mem_read, mem_group, n_groups)
    plan['seqs'], plan['quals'] = host_split_gather(plan, buf, off, lens, qbuf)
    return plan


def device_split_plan(lens, mem_read, mem_group, n_groups, out_cap=None):
    """mpn_reads_split_plan -> dict of PLAN_KEYS"""
    lib = _bind()
    lens, mem_read, mem_group = _split_args(lens, mem_read, mem_group)
    n, m, n_groups = len(lens), len(mem_read), int(n_groups)
    cap = m if out_cap is None else int(out_cap)
    out_read, out_off = np.zeros(max(cap, 1), dtype=np.int32), np.zeros(max(cap, 1), dtype=np.int64)
    group_first, group_byte = np.zeros(max(n_groups, 0) + 1, dtype=np.int64), np.zeros(max(n_groups, 0) + 1, dtype=np.int64)
    n_out, out_bytes = ct.c_int64(0), ct.c_int64(0)
    _ffi.check(lib.mpn_reads_split_plan(n, lens.ctypes.data, m, mem_read.ctypes.data, mem_group.ctypes.data, n_groups, cap, ct.addressof(n_out),
                                        out_read.ctypes.data, group_first.ctypes.data, out_off.ctypes.data, group_byte.ctypes.data,
                                        ct.addressof(out_bytes)), 'mpn_reads_split_plan')
    k = int(n_out.value)
    return dict(n_out=k, out_read=out_read[:k], group_first=group_first, out_off=out_off[:k], group_byte=group_byte, out_bytes=int(out_bytes.value))


def device_split_gather(plan, buf, off, lens, d_out, qbuf=None, d_qout=None, dev_src=None, want_host=True):
    """mpn_reads_split_gather into the caller's device buffers d_out / d_qout (torch uint8 tensors of at least out_bytes).
    buf / qbuf: host sources; dev_src = (bases, qualities or None) as torch uint8 tensors: the same sources resident in HBM, read
    instead.  -> (host copy of the bases or None, host copy of the qualities or None)"""
    lib = _bind()
    off, lens = np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(lens, dtype=np.int32)
    src_bytes = int((off + lens).max()) if len(lens) else 0
    if dev_src is not None:
        if int(dev_src[0].numel()) < src_bytes or (qbuf is not None and int(dev_src[1].numel()) < src_bytes):
            raise ValueError(f'split: the reads end at byte {src_bytes}, beyond their device buffer')
        s_ptr, q_ptr = dev_src[0].data_ptr(), (dev_src[1].data_ptr() if qbuf is not None else None)
    else:
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        qbuf = None if qbuf is None else np.ascontiguousarray(qbuf, dtype=np.uint8)
        if len(buf) < src_bytes or (qbuf is not None and len(qbuf) < src_bytes):
            raise ValueError(f'split: the reads end at byte {src_bytes}, beyond their buffer')
        s_ptr, q_ptr = buf.ctypes.data, (qbuf.ctypes.data if qbuf is not None else None)
    with_q = qbuf is not None
    out_bytes = int(plan['out_bytes'])
    h_out = np.empty(out_bytes, dtype=np.uint8) if want_host else None
    h_qout = np.empty(out_bytes, dtype=np.uint8) if want_host and with_q else None
    out_read, out_off = np.ascontiguousarray(plan['out_read'], dtype=np.int32), np.ascontiguousarray(plan['out_off'], dtype=np.int64)
    cap = int(d_out.numel()) if not with_q else min(int(d_out.numel()), int(d_qout.numel()))
    _ffi.check(lib.mpn_reads_split_gather(len(lens), s_ptr, q_ptr, src_bytes, off.ctypes.data, lens.ctypes.data, 1 if dev_src is not None else 0,
                                          int(plan['n_out']), out_read.ctypes.data, out_off.ctypes.data, out_bytes, d_out.data_ptr(),
                                          d_qout.data_ptr() if with_q else None, cap, h_out.ctypes.data if want_host else None,
                                          h_qout.ctypes.data if h_qout is not None else None), 'mpn_reads_split_gather')
    return h_out, h_qout


def split_last_ns():
    """Device time of this thread's last plan and gather call (HIP events), ns -> (plan, gather)"""
    lib = _bind()
    return int(lib.mpn_reads_split_last_ns(0)), int(lib.mpn_reads_split_last_ns(1))


def device_split_reads(buf, off, lens, mem_read, mem_group, n_groups, qbuf=None, dev_src=None, device='cuda'):
    """The device form of host_split_reads: the same dict, plus 'd_seqs' / 'd_quals' (torch uint8 tensors of out_bytes in HBM)."""
    import torch
    plan = device_split_plan(lens, mem_read, mem_group, n_groups)
    plan['d_seqs'] = torch.empty(plan['out_bytes'], dtype=torch.uint8, device=device)
    plan['d_quals'] = torch.empty(plan['out_bytes'], dtype=torch.uint8, device=device) if qbuf is not None else None
    plan['seqs'], plan['quals'] = device_split_gather(plan, buf, off, lens, plan['d_seqs'], qbuf, plan['d_quals'], dev_src)
    return plan


class ReadSplit:
    """The groups of split_reads(): one output buffer (host, and in HBM when the source batch is resident), a view per group."""

    def __init__(self, packed, res, n_groups):
        self.packed, self.res, self.n_groups = packed, res, int(n_groups)
        self._d_off = self._d_len = None
        if res.get('d_seqs') is not None:
            import torch
            dev = res['d_seqs'].device
            # every read's offset inside its own group's block, and its length, resident once for all group views
            g_of = np.repeat(np.arange(self.n_groups), np.diff(res['group_first']))
            self._d_off = torch.from_numpy(res['out_off'] - res['group_byte'][g_of]).to(dev)
            self._d_len = torch.from_numpy(np.ascontiguousarray(packed.lens[res['out_read']])).to(dev)

    def n_reads(self, g):
        return int(self.res['group_first'][g + 1] - self.res['group_first'][g])

    def group(self, g):
        """-> PackedReads of group g: views of the one output buffer, no copy"""
        r = self.res
        lo, hi, b0 = int(r['group_first'][g]), int(r['group_first'][g + 1]), int(r['group_byte'][g])
        reads = r['out_read'][lo:hi]
        dev = None
        if self._d_off is not None:
            dev = (r['d_seqs'][b0:], self._d_off[lo:hi], self._d_len[lo:hi])
        return PackedReads.from_arrays([self.packed.names[i] for i in reads], r['seqs'][b0:], r['out_off'][lo:hi] - b0, self.packed.lens[reads], dev=dev,
                                       qbuf=None if r['quals'] is None else r['quals'][b0:])


def split_reads(packed, read_idx, group, n_groups, device=None):
    """Regroup a PackedReads by (read, group) pairs (nanosplit's semantics: a pair once, input order inside a group) -> ReadSplit.
    device: None = on the GPU when the batch is resident there (packed.dev), True / False to choose."""
    on_dev = packed.dev is not None if device is None else bool(device)
    if not on_dev:
        return ReadSplit(packed, host_split_reads(packed.buf, packed.off, packed.lens, read_idx, group, n_groups, packed.qbuf), n_groups)
    import torch
    dev_src, where = None, 'cuda'
    if packed.dev is not None:
        where = packed.dev[0].device
        # the bases stay where they are; the qualities of a batch are not resident, they go up once for the gather
        dev_src = (packed.dev[0], None if packed.qbuf is None else torch.from_numpy(packed.qbuf).to(where))
    return ReadSplit(packed, device_split_reads(packed.buf, packed.off, packed.lens, read_idx, group, n_groups, packed.qbuf, dev_src, where), n_groups)


_rows_per_read = 2.0  # running estimate used to size the column arrays (a short guess costs a copy, not a second mapping)


def _emit(call, opt, packed, want_paf, want_cols):
    """Shared buffer handling of mpn_map_batch_q / mpn_hits_finish: call(text_buf, text_cap, cols_ref) -> rc.
    -> (text or None, SAM text or None (opt.out_sam == 2), column dict or None)"""
    global _rows_per_read
    lib = _bind()
    n = packed.n
    per_base = 3 if opt.out_sam == 1 else 0.5
    if opt.with_cigar:   # the difference strings of ~10 % error reads, per text (out_sam == 2 keeps the SAM in the library)
        per_base += (2.5 if opt.out_tags & TAG_CS_LONG else 1 if opt.out_tags & TAG_CS else 0) + (0.5 if opt.out_tags & TAG_MD else 0) + \
            (0.25 if opt.out_tags & TAG_EQX else 0)
    paf_cap = int(packed.bases * per_base) + 512 * n + 4096 if want_paf else 0
    rows_cap = max(64, int(n * _rows_per_read * 1.25) + 16)

    def make_cols(cap):
        cols, arrs = AlnCols(), {}
        cols.cap = cap
        for c in COL_NAMES:
            arrs[c] = np.empty(cap, dtype=np.int32)
            setattr(cols, c, arrs[c].ctypes.data)
        return cols, arrs

    out = ct.create_string_buffer(paf_cap) if want_paf else None
    cols, arrs = make_cols(rows_cap) if want_cols else (None, None)
    r = call(out, paf_cap, ct.byref(cols) if want_cols else None)
    if r == -3:  # the library kept what did not fit: fetch it, do not map again
        if want_cols and cols.n_rows > rows_cap:
            cols, arrs = make_cols(int(cols.n_rows))
            if lib.mpn_map_fetch_cols(ct.byref(cols)) < 0:
                raise _ffi.MpnError('mpn_map_fetch_cols: ' + _ffi.last_error())
        need = lib.mpn_map_fetch_text(None, 0) if want_paf else -1
        if need > 0:
            out = ct.create_string_buffer(need)
            r = lib.mpn_map_fetch_text(out, need)
            if r < 0:
                raise _ffi.MpnError('mpn_map_fetch_text: ' + _ffi.last_error())
        elif want_paf:
            r = len(out.value)
    elif r < 0:
        raise _ffi.MpnError(f'mapping call rc={r}: {_ffi.last_error()}')
    text = out.raw[:r].decode() if want_paf else None
    sam = None
    if opt.out_sam == 2:
        need = lib.mpn_map_fetch_sam(None, 0)
        if need < 0:
            raise _ffi.MpnError('mpn_map_fetch_sam: ' + _ffi.last_error())
        sbuf = ct.create_string_buffer(need)
        k = lib.mpn_map_fetch_sam(sbuf, need)
        sam = sbuf.raw[:k].decode()
    if want_cols:
        nr = int(cols.n_rows)
        _rows_per_read = max(_rows_per_read, nr / max(n, 1))
        arrs = {k: v[:nr] for k, v in arrs.items()}
    return text, sam, (arrs if want_cols else None)


def _dev_ptrs(packed, use_device):
    return [0, 0, 0] if (packed.dev is None or not use_device) else [t.data_ptr() for t in packed.dev]


def map_batch_full(idx, opt, packed, want_paf=False, want_cols=True, use_device=True):
    """-> (text (PAF; SAM if opt.out_sam == 1) or None, SAM text if opt.out_sam == 2 else None, column dict or None)"""
    lib = _bind()
    d = _dev_ptrs(packed, use_device)
    q = packed.qbuf.ctypes.data if getattr(packed, 'qbuf', None) is not None else None

    def call(out, cap, cols):
        return lib.mpn_map_batch_q(idx.h, ct.byref(opt), packed.n, packed.cnames, packed.buf.ctypes.data, q, packed.off.ctypes.data,
                                   packed.lens.ctypes.data, d[0], d[1], d[2], out, cap, cols)
    return _emit(call, opt, packed, want_paf, want_cols)


def map_batch_ex(idx, opt, packed, want_paf=False, want_cols=True, use_device=True):
    """-> (paf text or None, dict of int32 column arrays or None)"""
    text, _, cols = map_batch_full(idx, opt, packed, want_paf, want_cols, use_device)
    return text, cols


class Hits:
    """Hits of one batch of reads accumulated over the parts of a split index (minimap2 -I), merged by finish()
    the way minimap2 --split-prefix merges its per-part dumps."""

    def __init__(self, packed, want_text=True):
        self.packed = packed
        self.h = _bind().mpn_hits_create(packed.n)
        if not self.h:
            raise _ffi.MpnError('mpn_hits_create: ' + _ffi.last_error())
        if not want_text:   # columns only at finish(): the CIGARs of the parts' hits never leave the GPU
            _bind().mpn_hits_set_text(self.h, 0)

    def add_part(self, idx, opt, use_device=True):
        p = self.packed
        d = _dev_ptrs(p, use_device)
        _ffi.check(_bind().mpn_map_batch_part(idx.h, ct.byref(opt), p.n, p.cnames, p.buf.ctypes.data, p.off.ctypes.data, p.lens.ctypes.data,
                                              d[0], d[1], d[2], self.h), 'mpn_map_batch_part')

    def add_parts(self, parts, opt, use_device=True):
        """Several RESIDENT index parts in one call: reads uploaded once, (sub-batch, part) pairs in one pipeline."""
        p = self.packed
        d = _dev_ptrs(p, use_device)
        arr = (ct.c_void_p * len(parts))(*[i.h for i in parts])
        _ffi.check(_bind().mpn_map_batch_parts(arr, len(parts), ct.byref(opt), p.n, p.cnames, p.buf.ctypes.data, p.off.ctypes.data,
                                               p.lens.ctypes.data, d[0], d[1], d[2], self.h), 'mpn_map_batch_parts')

    def finish(self, opt, want_paf=False, want_cols=True):
        """-> (text, SAM text or None, columns); column `rid` indexes targets()"""
        lib = _bind()
        p = self.packed
        q = p.qbuf.ctypes.data if getattr(p, 'qbuf', None) is not None else None

        def call(out, cap, cols):
            return lib.mpn_hits_finish(self.h, ct.byref(opt), p.n, p.cnames, p.buf.ctypes.data, q, p.off.ctypes.data, p.lens.ctypes.data,
                                       out, cap, cols)
        return _emit(call, opt, p, want_paf, want_cols)

    def export(self, lo, hi):
        """The accumulated hits of reads [lo, hi) (before finish()) as one byte block for import_block() -> np.ndarray[uint8]"""
        lib = _bind()
        need = lib.mpn_hits_export(self.h, int(lo), int(hi), None, 0)
        if need < 0:
            raise _ffi.MpnError('mpn_hits_export: ' + _ffi.last_error())
        buf = np.empty(need, dtype=np.uint8)
        r = lib.mpn_hits_export(self.h, int(lo), int(hi), buf.ctypes.data, need)
        if r != need:
            raise _ffi.MpnError(f'mpn_hits_export rc={r}: {_ffi.last_error()}')
        return buf

    def import_block(self, buf, n_parts, names, lens):
        """Append a block of export() the way add_parts() would have appended the exporter's n_parts parts, whose targets are
        (names, lens).  Blocks are imported in part order."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        n = len(names)
        if len(lens) != n:
            raise ValueError(f'{n} target names but {len(lens)} lengths')
        cn = (ct.c_char_p * n)(*[x.encode() for x in names])
        _ffi.check(_bind().mpn_hits_import(self.h, buf.ctypes.data, len(buf), int(n_parts), n, cn, lens.ctypes.data), 'mpn_hits_import')

    def targets(self):
        lib = _bind()
        n = lib.mpn_hits_n_seq(self.h)
        buf = ct.create_string_buffer(1 << 16)
        names, lens = [], np.zeros(n, dtype=np.int32)
        for i in range(n):
            lib.mpn_hits_seq_name(self.h, i, buf, len(buf))
            names.append(buf.value.decode())
            lens[i] = lib.mpn_hits_seq_len(self.h, i)
        return names, lens

    def sam_header(self, cmdline=None):
        lib = _bind()
        names, _ = self.targets()
        cap = 64 * len(names) + sum(len(x) for x in names) + 4096 + (len(cmdline) if cmdline else 0)
        buf = ct.create_string_buffer(cap)
        r = lib.mpn_hits_sam_header(self.h, cmdline.encode() if cmdline else None, buf, cap)
        if r < 0:
            raise _ffi.MpnError(f'mpn_hits_sam_header rc={r}')
        return buf.raw[:r].decode()

    def close(self):
        if self.h:
            _bind().mpn_hits_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pack_pairs(queries, targets):
    """(query, target) pairs of 0..4 codes -> (qbuf, qoff, qlen, tbuf, toff, tlen) as the stage entries take them"""
    return pack_seqs([np.asarray(q, dtype=np.uint8) for q in queries]) + pack_seqs([np.asarray(t, dtype=np.uint8) for t in targets])


def _pack_alns(n, q_ivals, revs, t_starts, cigars):
    """the alignments of n pairs -> (qs, qe, rev, ts, cig, coff, ncig): the CIGARs one after the other, one spare op behind them"""
    qs = np.ascontiguousarray([iv[0] for iv in q_ivals], dtype=np.int32)
    qe = np.ascontiguousarray([iv[1] for iv in q_ivals], dtype=np.int32)
    rev = np.ascontiguousarray(np.broadcast_to(np.asarray(revs, dtype=np.int32), (n,)))
    ts = np.ascontiguousarray(np.broadcast_to(np.asarray(t_starts, dtype=np.int32), (n,)))
    ncig = np.array([len(c) for c in cigars], dtype=np.int32)
    coff = np.zeros(n, dtype=np.int64)
    if n > 1:
        coff[1:] = np.cumsum(ncig[:-1].astype(np.int64))
    cig = np.zeros(int(ncig.astype(np.int64).sum()) + 1, dtype=np.uint32)
    for c, o in zip(cigars, coff):
        cig[o:o + len(c)] = np.asarray(c, dtype=np.uint32)
    return qs, qe, rev, ts, cig, coff, ncig


def ext_dp_batch(opt, queries, targets, w, zdrop, end_bonus, flag, force_kernel=0):
    """DP stage on (query, target) pairs of 0..4 codes -> list of dicts (max, zdropped, max_q, max_t, mqe, mqe_t, score, reach_end, n_cigar, cigar).

    force_kernel: 0 dispatch as the mapper does; 1 LDS-state workgroup kernel with one wave per window; 3 the same with 256, 512
    or 1024 threads by band width; 4 systolic strip kernel where eligible, else as 5; 5 band-in-registers kernel where the band
    fits 1024 slots; 6 tiled strips where eligible.  Other windows go to the workgroup kernel, sized as under 0."""
    lib = _bind()
    n = len(queries)
    qbuf, qoff, qlen, tbuf, toff, tlen = _pack_pairs(queries, targets)
    arr = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.int32), (n,)))  # noqa: E731
    w, zdrop, end_bonus, flag = arr(w), arr(zdrop), arr(end_bonus), arr(flag)
    out = np.zeros((n, 9), dtype=np.int32)
    cap = int(qlen.astype(np.int64).sum() + tlen.astype(np.int64).sum()) + 4 * n
    pool = np.zeros(cap, dtype=np.uint32)
    coff = np.zeros(n, dtype=np.int64)
    rc = lib.mpn_ext_dp_batch(ct.byref(opt), n, qbuf.ctypes.data, qoff.ctypes.data, qlen.ctypes.data, tbuf.ctypes.data,
                              toff.ctypes.data, tlen.ctypes.data, w.ctypes.data, zdrop.ctypes.data, end_bonus.ctypes.data,
                              flag.ctypes.data, force_kernel, out.ctypes.data, pool.ctypes.data, cap, coff.ctypes.data)
    _ffi.check(rc, 'mpn_ext_dp_batch')
    keys = ('max', 'zdropped', 'max_q', 'max_t', 'mqe', 'mqe_t', 'score', 'reach_end', 'n_cigar')
    res = []
    for i in range(n):
        d = {k: int(out[i, j]) for j, k in enumerate(keys)}
        d['cigar'] = [int(x) for x in pool[coff[i]:coff[i] + d['n_cigar']]]
        res.append(d)
    return res


def aln_tags_batch(queries, q_ivals, revs, targets, t_starts, cigars, out_tags, caps=None):
    """The difference-string kernel on arbitrary alignments (mpn_aln_tags_batch).  queries / targets: 0..4 code arrays (reads in
    read orientation); q_ivals: (qs, qe) per pair in read coordinates; revs: strand per pair; t_starts: first target base;
    cigars: lists of len << 4 | op (M 0, I 1, D 2); out_tags: TAG_* bits; caps: (cs bytes, MD bytes, =/X ops) or None for bounds
    that always fit.  -> list of dict(cs=str or None, md=str or None, eqx=list or None), outputs that were not asked for None."""
    lib = _bind()
    n = len(queries)
    qbuf, qoff, qlen, tbuf, toff, tlen = _pack_pairs(queries, targets)
    qs, qe, rev, ts, cig, coff, ncig = _pack_alns(n, q_ivals, revs, t_starts, cigars)
    cols = sum(int(x) >> 4 for c in cigars for x in c)
    ops = int(ncig.astype(np.int64).sum())
    want_cs, want_md, want_eqx = bool(out_tags & (TAG_CS | TAG_CS_LONG)), bool(out_tags & TAG_MD), bool(out_tags & TAG_EQX)
    cs_cap, md_cap, eqx_cap = caps if caps is not None else (3 * cols + 2 * ops + 16, 2 * cols + 2 * ops + 16 * n + 16, cols + ops + 16)
    cs = np.zeros(cs_cap if want_cs else 1, dtype=np.uint8)
    md = np.zeros(md_cap if want_md else 1, dtype=np.uint8)
    eqx = np.zeros(eqx_cap if want_eqx else 1, dtype=np.uint32)
    cs_off, md_off, eqx_off = (np.zeros(n + 1, dtype=np.int64) for _ in range(3))
    rc = lib.mpn_aln_tags_batch(n, qbuf.ctypes.data, qoff.ctypes.data, qlen.ctypes.data, qs.ctypes.data, qe.ctypes.data, rev.ctypes.data,
                                tbuf.ctypes.data, toff.ctypes.data, tlen.ctypes.data, ts.ctypes.data, cig.ctypes.data, coff.ctypes.data,
                                ncig.ctypes.data, int(out_tags), cs.ctypes.data, cs_cap if want_cs else 0, cs_off.ctypes.data,
                                md.ctypes.data, md_cap if want_md else 0, md_off.ctypes.data, eqx.ctypes.data, eqx_cap if want_eqx else 0,
                                eqx_off.ctypes.data)
    _ffi.check(rc, 'mpn_aln_tags_batch')
    res = []
    for i in range(n):
        res.append(dict(cs=cs[cs_off[i]:cs_off[i + 1]].tobytes().decode() if want_cs else None,
                        md=md[md_off[i]:md_off[i + 1]].tobytes().decode() if want_md else None,
                        eqx=[int(x) for x in eqx[eqx_off[i]:eqx_off[i + 1]]] if want_eqx else None))
    return res



def aln_finish_batch(opt, queries, q_ivals, revs, targets, t_starts, cigars, force_class=0):
    """The CIGAR finishing kernel on arbitrary alignments (mpn_aln_finish_batch); arguments as for aln_tags_batch, ops of length
    0 allowed, scoring from opt.  force_class: 0 the launch class as the mapper chooses it, 1..3 the 16 / 32 / 64 KB LDS class, 4
    global scratch.  -> list of dict(n_cigar, qshift, tshift, blen, mlen, n_ambi, dp_max, cigar)."""
    lib = _bind()
    n = len(queries)
    qbuf, qoff, qlen, tbuf, toff, tlen = _pack_pairs(queries, targets)
    qs, qe, rev, ts, cig, coff, ncig = _pack_alns(n, q_ivals, revs, t_starts, cigars)
    out = np.zeros((n, 8), dtype=np.int32)
    fixed = np.zeros_like(cig)
    rc = lib.mpn_aln_finish_batch(ct.byref(opt), n, qbuf.ctypes.data, qoff.ctypes.data, qlen.ctypes.data, qs.ctypes.data, qe.ctypes.data,
                                  rev.ctypes.data, tbuf.ctypes.data, toff.ctypes.data, tlen.ctypes.data, ts.ctypes.data, cig.ctypes.data,
                                  coff.ctypes.data, ncig.ctypes.data, int(force_class), out.ctypes.data, fixed.ctypes.data)
    _ffi.check(rc, 'mpn_aln_finish_batch')
    keys = ('n_cigar', 'qshift', 'tshift', 'blen', 'mlen', 'n_ambi', 'dp_max')
    res = []
    for i in range(n):
        d = {k: int(out[i, j]) for j, k in enumerate(keys)}
        d['cigar'] = fixed[coff[i]:coff[i] + d['n_cigar']].tolist()
        res.append(d)
    return res


HIT_KEYS = ('fx', 'fy', 'lx', 'ly', 'score', 'score0', 'cnt', 'as', 'parent', 'subsc', 'n_sub', 'mlen', 'blen', 'hash', 'sam_pri')


def hit_select_batch(opt, k, q_len, names, chain_off, u, recs, anchor_off, anchors, path=0, max_chains=0, grid_cap=0):
    """The hit stage on arbitrary chains (mpn_hit_select_batch).  CSR over reads: chain_off[n + 1], anchor_off[n + 1]; per chain in
    pool order u (score << 32 | cnt) and recs = (fx, fy, lx, ly, mlen, blen) arrays; anchors: uint64 [total, 2] (x, y).  path: 0 the
    mapper's dispatch, 1 the large kernel instantiation for all, 2 the host functions; max_chains 0 = 384; grid_cap 0 = the mapper's
    grids.  -> (n_regs int32[n], n_a int32[n], hits int64 [sum n_regs, 15] in HIT_KEYS order (fx..ly and hash as unsigned bit
    patterns), squeezed anchors uint64 [sum n_a, 2] or None without opt.with_cigar)."""
    lib = _bind()
    n = len(q_len)
    c = lambda v, t: np.ascontiguousarray(v, dtype=t)  # noqa: E731
    q_len, chain_off, anchor_off, u = c(q_len, np.int32), c(chain_off, np.int64), c(anchor_off, np.int64), c(u, np.uint64)
    fx, fy, lx, ly = (c(r, np.uint64) for r in recs[:4])
    mlen, blen = c(recs[4], np.int32), c(recs[5], np.int32)
    anchors = c(anchors, np.uint64).reshape(-1, 2)
    assert len(chain_off) == n + 1 and len(anchor_off) == n + 1 and len(names) == n
    n_chains, n_anch = int(chain_off[-1]) if n else 0, int(anchor_off[-1]) if n else 0
    assert all(len(x) == n_chains for x in (u, fx, fy, lx, ly, mlen, blen)) and len(anchors) == n_anch
    cnames = (ct.c_char_p * max(1, n))(*[(nm.encode() if isinstance(nm, str) else nm) for nm in names])
    n_regs, n_a = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    hits = np.zeros((n_chains + 1, 15), dtype=np.int64)
    sq = np.zeros((n_anch + 1, 2), dtype=np.uint64)
    rc = lib.mpn_hit_select_batch(ct.byref(opt), int(k), n, q_len.ctypes.data, cnames, chain_off.ctypes.data, u.ctypes.data, fx.ctypes.data,
                                  fy.ctypes.data, lx.ctypes.data, ly.ctypes.data, mlen.ctypes.data, blen.ctypes.data, anchor_off.ctypes.data,
                                  anchors.ctypes.data, int(path), int(max_chains), int(grid_cap), n_regs.ctypes.data, n_a.ctypes.data,
                                  hits.ctypes.data, sq.ctypes.data)
    _ffi.check(rc, 'mpn_hit_select_batch')
    return n_regs, n_a, hits[:int(n_regs.sum())], (sq[:int(n_a.sum())] if opt.with_cigar else None)


PLAN_HIT_KEYS = ('n_jobs', 'as1', 'cnt1', 'qs', 'rs', 'qe', 're', 'qs0', 'qe0', 'rid', 'rev')
PLAN_WIN_KEYS = ('read', 'rid', 'rev', 'qs', 'qlen', 'ts', 'tlen', 'reversed', 'w', 'zdrop', 'end_bonus', 'flag', 'anchor')


def ext_plan_batch(opt, k, t_len, q_len, anchor_off, anchors, hit_off, h_as, h_cnt, h_mlen, h_split_inv, grid_cap=0):
    """The extension planning stage on arbitrary hits (mpn_ext_plan_batch).  t_len: target lengths.  CSR over reads: anchor_off[n + 1]
    into anchors uint64 [total, 2] (x, y; flag bits 40..42 of y allowed), hit_off[n + 1] into the per-hit arrays h_as, h_cnt, h_mlen,
    h_split_inv.  grid_cap 0 = the mapper's grid, else at most that many blocks.  -> (hits int32 [n_hits, 11] in PLAN_HIT_KEYS order, windows
    int32 [sum n_jobs, 13] in PLAN_WIN_KEYS order, hit after hit in input order, anchors uint64 [total, 2] as the kernel left them)."""
    lib = _bind()
    n = len(q_len)
    c = lambda v, t: np.ascontiguousarray(v, dtype=t)  # noqa: E731
    t_len, q_len, anchor_off, hit_off = c(t_len, np.int32), c(q_len, np.int32), c(anchor_off, np.int64), c(hit_off, np.int64)
    h_as, h_cnt, h_mlen, h_split_inv = (c(v, np.int32) for v in (h_as, h_cnt, h_mlen, h_split_inv))
    anchors = c(anchors, np.uint64).reshape(-1, 2)
    assert len(anchor_off) == n + 1 and len(hit_off) == n + 1
    n_anch, n_hits = (int(anchor_off[-1]), int(hit_off[-1])) if n else (0, 0)
    assert len(anchors) == n_anch and all(len(v) == n_hits for v in (h_as, h_cnt, h_mlen, h_split_inv))
    win_cap = int(np.maximum(h_cnt.astype(np.int64), 0).sum()) + n_hits
    hits = np.zeros((n_hits + 1, 11), dtype=np.int32)
    wins = np.zeros((win_cap + 1, 13), dtype=np.int32)
    left = np.zeros((n_anch + 1, 2), dtype=np.uint64)
    n_win = ct.c_int64(0)
    rc = lib.mpn_ext_plan_batch(ct.byref(opt), int(k), len(t_len), t_len.ctypes.data, n, q_len.ctypes.data, anchor_off.ctypes.data,
                                anchors.ctypes.data, hit_off.ctypes.data, h_as.ctypes.data, h_cnt.ctypes.data, h_mlen.ctypes.data,
                                h_split_inv.ctypes.data, int(grid_cap), hits.ctypes.data, win_cap, ct.addressof(n_win), wins.ctypes.data,
                                left.ctypes.data)
    _ffi.check(rc, 'mpn_ext_plan_batch')
    return hits[:n_hits], wins[:n_win.value], left[:n_anch]


STITCH_HIT_KEYS = ('read', 'rid', 'rev', 'as', 'cnt', 'as1', 'cnt1', 'qs', 'rs', 'qe', 're', 'qs0', 'qe0', 'first_win', 'n_win')
STITCH_WIN_KEYS = ('flag', 'reversed', 'qs', 'ts', 'anchor', 'max', 'zdropped', 'max_q', 'max_t', 'mqe_t', 'score', 'reach_end', 'n_cigar')
STITCH_OUT_KEYS = ('cig_off', 'n_ops', 'dp_score', 'rs1', 're1', 'qs1', 'qe1', 'has_p', 'dropped', 'drop_fill', 'drop_max_t', 'drop_max_q',
                   'split_n', 'split_inv', 'split_rec')
STITCH_FIN_KEYS = ('cig_off', 'code_off', 'n_cigar', 'read', 'rid', 'rev', 'qs1', 'rs1', 'qspan', 'tspan')
STITCH_SPLIT_KEYS = ('fx', 'fy', 'lx_left', 'ly_left', 'mlen_l', 'blen_l', 'mlen_r', 'blen_r')


def stitch_batch(anchor_off, anchors, hits, wins, cig_pos, compact, min_cnt, grid_cap=0):
    """The stitching stage on arbitrary hits, windows and window results (mpn_stitch_batch).  anchor_off[n + 1] into anchors uint64
    [total, 2]; hits int32 [n_hits, 15] in STITCH_HIT_KEYS order; wins int32 [n_win, 13] in STITCH_WIN_KEYS order with cig_pos int64
    [n_win] into compact uint32.  grid_cap 0 = the mapper's grid, else at most that many blocks.  -> (out int64 [n_hits, 25]: STITCH_OUT_KEYS
    then STITCH_FIN_KEYS, pool uint32 [the cursor's final value], splits int64 [n_splits, 8] in STITCH_SPLIT_KEYS order, x / y words bit for
    bit)."""
    lib = _bind()
    c = lambda v, t: np.ascontiguousarray(v, dtype=t)  # noqa: E731
    anchor_off, cig_pos, compact = c(anchor_off, np.int64), c(cig_pos, np.int64), c(compact, np.uint32)
    anchors, hits, wins = c(anchors, np.uint64).reshape(-1, 2), c(hits, np.int32).reshape(-1, 15), c(wins, np.int32).reshape(-1, 13)
    n = len(anchor_off) - 1
    assert n >= 0 and len(anchors) == (int(anchor_off[-1]) if n else 0) and len(cig_pos) == len(wins)
    n_hits = len(hits)
    pool_cap = int(np.maximum(wins[:, 12].astype(np.int64), 0).sum())
    out = np.zeros((n_hits + 1, 25), dtype=np.int64)
    pool = np.zeros(pool_cap + 1, dtype=np.uint32)
    splits = np.zeros((n_hits + 1, 8), dtype=np.int64)
    used, n_splits = ct.c_int64(0), ct.c_int64(0)
    rc = lib.mpn_stitch_batch(n, anchor_off.ctypes.data, anchors.ctypes.data, n_hits, hits.ctypes.data, len(wins), wins.ctypes.data,
                              cig_pos.ctypes.data, len(compact), compact.ctypes.data, int(min_cnt), int(grid_cap), out.ctypes.data, pool_cap,
                              pool.ctypes.data, ct.addressof(used), splits.ctypes.data, ct.addressof(n_splits))
    _ffi.check(rc, 'mpn_stitch_batch')
    return out[:n_hits], pool[:used.value], splits[:n_splits.value]


STAT_NAMES = {0: 'bases', 1: 'minimizers', 2: 'anchors', 3: 'chains', 4: 'dp_jobs', 5: 'dp_cells', 6: 'alignments',
              7: 'dp_rounds', 8: 'second_pass_jobs', 10: 'ev_sketch_ns', 11: 'ev_seed_ns', 12: 'ev_sort_ns',
              13: 'ev_chain_dp_ns', 14: 'ev_chain_bt_ns', 15: 'ev_ext_dp_ns', 25: 'ev_ext_bt_ns', 26: 'ev_ext_ztest_ns',
              16: 'wall_h2d_ns', 17: 'wall_seed_chain_ns', 18: 'wall_d2h_chains_ns', 19: 'wall_host_hits_ns',
              20: 'wall_host_plan_ns', 21: 'wall_ext_stage_ns', 22: 'wall_host_stitch_ns', 23: 'wall_host_final_ns',
              24: 'wall_total_ns', 27: 'wall_ext_host_prep_ns', 28: 'wall_ext_enqueue_ns', 29: 'wall_ext_gpu_wait_ns',
              30: 'wall_ext_finish_ns', 9: 'ev_ext_strip_ns', 31: 'strip_cells', 32: 'sub_batches',
              33: 'k_sketch_count_ns', 34: 'k_sketch_fill_ns', 35: 'k_seed_lookup_ns', 36: 'k_seed_fill_ns',
              37: 'k_chain_dp_ns', 38: 'k_strip16_ns', 39: 'k_strip32_ns', 40: 'k_strip64_ns', 41: 'strip16_cells',
              42: 'strip32_cells', 43: 'strip64_cells', 44: 'sort_records_moved', 45: 'anchors_kept', 46: 'k_compact_ns', 47: 'k_sort_msd_ns', 48: 'k_sort_chunk_ns', 49: 'k_sort_radix_ns',
              50: 'k_seed_filter_ns', 51: 'anchors_emitted', 52: 'k_finish_ns', 53: 'cigar_ops', 54: 'k_stitch_ns', 55: 'k_plan_ns', 56: 'k_layout_ns', 57: 'k_xstrip_ns', 58: 'xstrip_cells', 59: 'anchors_squeezed', 60: 'workers_shed', 61: 'workers', 62: 'k_hit_select_ns', 63: 'reads_hits_on_host',
              64: 'tile_windows', 65: 'wall_lease_wait_ns', 66: 'ext_groups_side_leased', 67: 'ext_groups_side_own',
              68: 'tile_windows_1w_s16', 69: 'tile_windows_s4_nw8', 70: 'tile_windows_s8_nw4', 71: 'tile_windows_s4_nw16',
              72: 'tile_wait_giveups',
              # ev_ext_walk_long_ns: traceback + z-drop test of the tile and side lists where they run on the worker's own
              # stream (MPN_KERNEL_EVENTS on: two more events per extension group); ev_ext_dp_ns held this time before and no
              # longer does.  Where the side / tile work got leased streams the span is ~0 and their walks are in no slot.
              73: 'walk_wave_windows', 74: 'ev_ext_walk_long_ns',
              75: 'walk_wave_failed',   # gap fills the wave z-drop test failed (second pass or inversion probe)
              76: 'k_tags_ns'}          # aln_tags_wave_kernel: cs / MD / =X strings (0 unless out_tags asks for them in a text call)


def last_stats():
    n = max(STAT_NAMES) + 1
    s = np.zeros(n, dtype=np.int64)
    _bind().mpn_map_last_stats_ex(s.ctypes.data, n)
    return {name: int(s[i]) for i, name in STAT_NAMES.items()}
