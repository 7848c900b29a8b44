"""Plain restatement of the seed half of the mapper (hit collection, the stray-hit filter's rules, the order of the anchor sort) for
test_seed_ref.py and test_seed_stage_gpu.py.  Nothing here follows the kernels' structure: collect is minimap2's mm_collect_matches
with its loops, needed is the compaction's rule, bin_rule the filter as its comment states it.  sketch_rule is the one function that
restates constants of the implementation (see there).  The *_np forms are the same functions without Python loops over hits; the
CPU test pins them to the loops.

An index is a MadeIndex: k, lens[n_seq], keys[n_keys] ascending, key_off[n_keys + 1], pos[] as rid << 32 | position << 1 | strand.
Minimizers are (n, 2) uint64 arrays in the sketch's layout: x = hash << 8 | span, y = read << 32 | last_pos << 1 | strand.
Anchors are (n, 2) uint64 arrays: x = strand << 63 | rid << 32 | target position, y = flags << 40 | span << 32 | read position."""
import numpy as np

U64 = np.uint64
TANDEM = 1 << 42
EMPTY = np.zeros((0, 2), dtype=U64)


class MadeIndex:
    def __init__(self, k, lens, table):
        """table: {hash: [position words]} (the words ascending inside a key)"""
        self.k = int(k)
        self.lens = np.asarray(lens, dtype=np.int32)
        hs = sorted(table)
        self.keys = np.array(hs, dtype=U64)
        cnt = [len(table[h]) for h in hs]
        self.key_off = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)]).astype(np.int64)
        self.pos = np.array([w for h in hs for w in table[h]], dtype=U64) if sum(cnt) else np.zeros(0, dtype=U64)

    @classmethod
    def from_arrays(cls, k, lens, keys, key_off, pos):
        self = cls.__new__(cls)
        self.k, self.lens = int(k), np.asarray(lens, dtype=np.int32)
        self.keys, self.key_off, self.pos = np.asarray(keys, dtype=U64), np.asarray(key_off, dtype=np.int64), np.asarray(pos, dtype=U64)
        return self

    def get(self, h):
        """the position words of hash h (mm_idx_get)"""
        i = int(np.searchsorted(self.keys, U64(h)))
        if i == len(self.keys) or int(self.keys[i]) != int(h):
            return self.pos[:0]
        return self.pos[self.key_off[i]:self.key_off[i + 1]]


def word(rid, p, strand=0):
    return rid << 32 | p << 1 | strand


def minimizer(h, span, last_pos, strand=0, read=0):
    return (h << 8 | span, read << 32 | last_pos << 1 | strand)


def sort_anchors(a):
    """by (x, low 32 bits of y): the order of minimap2's radix_sort_128x on anchors whose read positions are below 2^32"""
    a = np.asarray(a, dtype=U64).reshape(-1, 2)
    return a[np.lexsort((a[:, 1] & U64(0xffffffff), a[:, 0]))]


def collect(index, mz, qlen, mid_occ):
    """mm_collect_matches -> (anchors sorted, n_anchor, rep_len, span_sum)"""
    mz = [(int(x), int(y)) for x, y in np.asarray(mz, dtype=U64).reshape(-1, 2)]
    out, rep_st, rep_en, rep_len, span_sum = [], 0, 0, 0, 0
    for i, (mx, my) in enumerate(mz):
        q_pos, q_span = my & 0xffffffff, mx & 0xff
        cr = index.get(mx >> 8)
        if len(cr) >= mid_occ:
            en = (q_pos >> 1) + 1
            st = en - q_span
            if st > rep_en:
                rep_len += rep_en - rep_st
                rep_st, rep_en = st, en
            else:
                rep_en = en
            continue
        tandem = (i > 0 and mz[i - 1][0] >> 8 == mx >> 8) or (i + 1 < len(mz) and mz[i + 1][0] >> 8 == mx >> 8)
        for r in cr:
            r = int(r)
            rpos = (r & 0xffffffff) >> 1
            if (r & 1) == (q_pos & 1):
                x, y = (r >> 32 << 32) | rpos, q_span << 32 | q_pos >> 1
            else:
                x, y = 1 << 63 | (r >> 32 << 32) | rpos, q_span << 32 | ((qlen - ((q_pos >> 1) + 1 - q_span) - 1) & 0xffffffff)
            out.append((x, y | TANDEM if tandem else y))
            span_sum += q_span
    rep_len += rep_en - rep_st
    a = sort_anchors(np.array(out, dtype=U64)) if out else EMPTY
    return a, len(out), rep_len, span_sum


def collect_np(index, mz, qlen, mid_occ):
    """collect without a Python loop over the hits (the loop over the repetitive minimizers stays: it is the definition of rep_len)"""
    mz = np.asarray(mz, dtype=U64).reshape(-1, 2)
    n = len(mz)
    if n == 0:
        return EMPTY, 0, 0, 0
    h = mz[:, 0] >> U64(8)
    span = (mz[:, 0] & U64(0xff)).astype(np.int64)
    q_pos = (mz[:, 1] & U64(0xffffffff)).astype(np.int64)
    ki = np.searchsorted(index.keys, h)
    found = ki < len(index.keys)
    found[found] = index.keys[ki[found]] == h[found]
    kf = np.where(found, ki, 0)
    start = np.where(found, index.key_off[kf], 0) if len(index.keys) else np.zeros(n, np.int64)
    t = np.where(found, index.key_off[kf + 1] - index.key_off[kf], 0) if len(index.keys) else np.zeros(n, np.int64)
    rep = t >= mid_occ
    rep_st = rep_en = rep_len = 0
    for en, sp in zip(((q_pos[rep] >> 1) + 1).tolist(), span[rep].tolist()):
        if en - sp > rep_en:
            rep_len += rep_en - rep_st
            rep_st, rep_en = en - sp, en
        else:
            rep_en = en
    rep_len += rep_en - rep_st
    t = np.where(rep, 0, t)
    total = int(t.sum())
    if total == 0:
        return EMPTY, 0, rep_len, 0
    same = h[1:] == h[:-1]
    tandem = np.zeros(n, dtype=bool)
    tandem[1:] |= same
    tandem[:-1] |= same
    own = np.repeat(np.arange(n), t)
    first = np.cumsum(t) - t
    r = index.pos[start[own] + (np.arange(total) - first[own])]
    rpos = (r & U64(0xffffffff)) >> U64(1)
    qp, sp = q_pos[own], span[own]
    fwd = (r & U64(1)).astype(np.int64) == (qp & 1)
    x = (r >> U64(32) << U64(32)) | rpos | np.where(fwd, U64(0), U64(1 << 63))
    qy = np.where(fwd, qp >> 1, (qlen - ((qp >> 1) + 1 - sp) - 1) & 0xffffffff)
    y = sp.astype(U64) << U64(32) | qy.astype(U64) | np.where(tandem[own], U64(TANDEM), U64(0))
    return sort_anchors(np.stack([x, y], axis=1)), total, rep_len, int((t * span).sum())


def segment_starts(x, max_gap):
    """sorted x of one read -> bool per anchor: it starts a segment (its x exceeds its predecessor's by more than max_gap; the first does)"""
    st = np.ones(len(x), dtype=bool)
    st[1:] = x[1:] - x[:-1] > U64(max_gap)
    return st


def needed(anchors, max_gap, min_cnt):
    """what the compaction keeps: bool per sorted anchor, members of segments of at least clamp(min_cnt, 1, 64) anchors"""
    x = np.asarray(anchors, dtype=U64).reshape(-1, 2)[:, 0]
    if len(x) == 0:
        return np.zeros(0, dtype=bool)
    seg = np.cumsum(segment_starts(x, max_gap)) - 1
    return np.bincount(seg)[seg] >= min(max(min_cnt, 1), 64)


def filter_bins(max_gap, min_cnt):
    """-> (T, shift): the count a bin must reach, and the bin width 2^shift the host derives: the smallest power of two, at least 2,
    that is >= 2 (T - 1) max(max_gap, 1)"""
    T = min(max(min_cnt, 1), 3)
    sh = 1
    while sh < 32 and (1 << sh) < 2 * (T - 1) * max(max_gap, 1):
        sh += 1
    return T, sh


def _groups(anchors, max_gap, min_cnt):
    x = np.asarray(anchors, dtype=U64).reshape(-1, 2)[:, 0]
    T, sh = filter_bins(max_gap, min_cnt)
    hi = x >> U64(32)                                    # strand and target: hits on another strand or target never count together
    rpos = x & U64(0xffffffff)
    return hi, rpos >> U64(sh), (rpos + U64(1 << (sh - 1))) >> U64(sh), T


def bin_rule(anchors, max_gap, min_cnt):
    """the filter as stated, with exact counts: a hit passes if its A bin (pos / W) or its B bin ((pos + W / 2) / W) holds at least T
    hits of the same read, strand and target"""
    hi, ba, bb, T = _groups(anchors, max_gap, min_cnt)
    if len(hi) == 0:
        return np.zeros(0, dtype=bool)

    def count(b):
        _, inv, cnt = np.unique(hi << U64(32) | b, return_inverse=True, return_counts=True)
        return cnt[inv.reshape(-1)]
    return (count(ba) >= T) | (count(bb) >= T)


# ---- the filter as it is.  This function alone restates constants of the implementation (csrc/map_kernels.h: FLT_SLOTS, the
# multipliers and shifts of flt_slots, the B family's xor, the three-level counters): change them there and here together. --------
FLT_SLOTS = 81920


def _slots(hi, b):
    M = 0xffffffff
    hi, b = hi.astype(np.uint64) & U64(M), b.astype(np.uint64) & U64(M)
    k = ((hi * U64(0x9E3779B1)) & U64(M)) ^ ((((b + U64(0x7F4A7C15)) & U64(M)) * U64(0x85EBCA77)) & U64(M))
    k ^= k >> U64(15)
    k = (k * U64(0x2C1B3C6D)) & U64(M)
    k ^= k >> U64(12)
    s1 = (k * U64(FLT_SLOTS)) >> U64(32)
    k2 = (k * U64(0x297A2D39)) & U64(M)
    k2 ^= k2 >> U64(15)
    s2 = (((k2 * U64(0x85EBCA6B)) & U64(M)) * U64(FLT_SLOTS)) >> U64(32)
    return s1.astype(np.int64), s2.astype(np.int64)


def sketch_rule(anchors, max_gap, min_cnt, flt_round2=0, rounds=None):
    """bool per anchor: what the device's filter keeps.  Per family (A, B) two count-min tables of FLT_SLOTS counters that saturate at
    3; a hit passes if both counters of its A bin or both of its B bin have reached T.  A read with at least flt_round2 hits
    (flt_round2 > 0) is counted a second time over the survivors alone.  Counting commutes, so the result is a function of the
    read's set of hits.  rounds: a list that receives the number of hits each round walked."""
    hi, ba, bb, T = _groups(anchors, max_gap, min_cnt)
    n = len(hi)
    keep = np.ones(n, dtype=bool)
    if n == 0:
        return keep
    a1, a2 = _slots(hi, ba)
    b1, b2 = _slots(hi ^ U64(0x5bd1e995), bb)
    for rnd in range(2 if flt_round2 > 0 and n >= flt_round2 else 1):
        live = np.flatnonzero(keep)
        if rounds is not None:
            rounds.append(len(live))
        c = [np.minimum(np.bincount(s[live], minlength=FLT_SLOTS), 3) for s in (a1, a2, b1, b2)]
        ok = ((c[0][a1[live]] >= T) & (c[1][a2[live]] >= T)) | ((c[2][b1[live]] >= T) & (c[3][b2[live]] >= T))
        keep[:] = False
        keep[live[ok]] = True
    return keep


# ---- the sort's work lists: which buckets of the kept anchors the partition sends to which list (the partition's bin restated:
# strand, then (target, position) squeezed to 13 bits; csrc/map_kernels.h anchor_bin and the host's BinParams) -----------------------
def sort_bins(anchors, lens):
    x = np.asarray(anchors, dtype=U64).reshape(-1, 2)[:, 0]
    rid_bits, pos_bits = 0, 1
    while (1 << rid_bits) < len(lens):
        rid_bits += 1
    while (1 << pos_bits) < max(1, int(np.max(lens))):
        pos_bits += 1
    shift = max(0, rid_bits + pos_bits - 13)
    comp = ((x >> U64(32) & U64(0x7fffffff)) << U64(pos_bits)) | (x & U64(0xffffffff))
    return ((x >> U64(63)) << U64(13) | comp >> U64(shift)).astype(np.int64), shift


def bucket_sizes(anchors, lens):
    """sizes of the per-read buckets (runs of equal bin in the sorted anchors), in order"""
    b, _ = sort_bins(anchors, lens)
    if len(b) == 0:
        return np.zeros(0, dtype=np.int64)
    cut = np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1], [True]]))
    return np.diff(cut)


def list_counts(sizes):
    s = np.asarray(sizes)
    return (int(((s > 16) & (s <= 1024)).sum()), int(((s > 1024) & (s <= 4096)).sum()), int((s > 4096).sum()))
