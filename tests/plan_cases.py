"""Hand-built anchors for the tests of the extension planning stage (test_plan_ref.py on the CPU, test_ext_plan_gpu.py on the
GPU).  No genome and no mapper run: a read is its squeezed anchor list, (x, y) words as the hit stage leaves them (x = strand << 63
| rid << 32 | last target base of the k-mer, y = flags | span << 32 | last read base on the hit's strand), and the hits to plan,
(as, cnt, mlen, split_inv) in the order they are handed over.

families() -> {name: [Batch]}; a batch is one call of the stage: k, target lengths, options, reads."""
import numpy as np

from plan_ref import SEED_IGNORE, SEED_LONG_JOIN, SEED_TANDEM, plan_ref

K = 15
TLEN = 400000      # every target of the default set (longer than any read here)


def word(rid, rev, t, q, span=K, flags=0):
    assert t >= 0 and q >= 0 and 1 <= span <= 255
    return (rev << 63 | rid << 32 | t, flags | span << 32 | q)


def walk(n, t0, q0, d=20, gaps=None, rid=0, rev=0, span=K, spans=None, flags=None):
    """n anchors from (t0, q0), d bases apart on both sequences; gaps {i: g}: the step into anchor i is g bases longer on the
    read (g > 0) or -g bases longer on the target (g < 0); spans / flags {i: value} for single anchors"""
    gaps, spans, flags = gaps or {}, spans or {}, flags or {}
    out, t, q = [], t0, q0
    for i in range(n):
        if i:
            g = gaps.get(i, 0)
            t += d + max(0, -g)
            q += d + max(0, g)
        out.append(word(rid, rev, t, q, spans.get(i, span), flags.get(i, 0)))
    return out


def fuzzy_mlen(a):
    """the match length the hit stage hands over (mm_cal_fuzzy_len's mlen)"""
    m = a[0][1] >> 32 & 0xff
    for p, c in zip(a, a[1:]):
        tl, ql = (c[0] & 0xffffffff) - (p[0] & 0xffffffff), (c[1] & 0xffffffff) - (p[1] & 0xffffffff)
        m += min(min(tl, ql), c[1] >> 32 & 0xff)
    return m


class Read:
    def __init__(self, name, parts, qlen=None, order=None):
        """parts: anchor lists in list order; a part given as (anchors, dict) is a hit (dict: mlen, split_inv), a bare list is not.
        order: the order the hits are handed over in (indices into the hits by position; default: by position)"""
        self.name, self.anchors, hits = name, [], []
        for p in parts:
            a, kw = p if isinstance(p, tuple) else (p, None)
            if kw is not None:
                hits.append((len(self.anchors), len(a), kw.get('mlen', fuzzy_mlen(a)), kw.get('split_inv', 0)))
            self.anchors.extend(a)
        self.hits = hits if order is None else [hits[i] for i in order]
        self.qlen = max(y & 0xffffffff for _, y in self.anchors) + 301 if qlen is None else qlen


class Batch:
    def __init__(self, name, reads, k=K, tlens=(TLEN, TLEN, TLEN), **opt):
        self.name, self.reads, self.k, self.tlens, self.opt = name, reads, k, list(tlens), opt

    def ref(self):
        """plan_ref of every read: [(hits, anchors, evs)]"""
        return [plan_ref(self.k, self.tlens, r.qlen, r.anchors, r.hits, **self.opt) for r in self.reads]

    def arrays(self):
        """the batch as mapper.ext_plan_batch takes it"""
        a_off = np.cumsum([0] + [len(r.anchors) for r in self.reads]).astype(np.int64)
        h_off = np.cumsum([0] + [len(r.hits) for r in self.reads]).astype(np.int64)
        hits = np.array([h for r in self.reads for h in r.hits], dtype=np.int32).reshape(-1, 4)
        return dict(tlens=np.array(self.tlens, dtype=np.int32), q_len=np.array([r.qlen for r in self.reads], dtype=np.int32), anchor_off=a_off,
                    anchors=np.array([p for r in self.reads for p in r.anchors], dtype=np.uint64).reshape(-1, 2), hit_off=h_off,
                    h_as=hits[:, 0].copy(), h_cnt=hits[:, 1].copy(), h_mlen=hits[:, 2].copy(), h_split_inv=hits[:, 3].copy())


def hit(a, **kw):
    return (a, kw)


# ---- ends: tiny hits, missing left windows, the clamp of rs0, both strands, rid > 0, odd and even k -------------------------------
def ends_family():
    batches = []
    for k in (15, 20):
        kh = k >> 1
        reads = []
        for rid, rev in ((0, 0), (2, 1), (1, 0), (1, 1)):
            sfx = '-t%d%s' % (rid, '-' if rev else '+')
            for cnt in (1, 2, 3, 4):
                reads.append(Read('cnt%d%s' % (cnt, sfx), [hit(walk(cnt, 3000, 900, rid=rid, rev=rev, span=k))]))
            # no left window: the first k-mer's centre sits on (or before) the first base of the read / of the target
            reads.append(Read('qs0' + sfx, [hit(walk(5, 3000, kh, rid=rid, rev=rev, span=kh + 1))]))
            reads.append(Read('rs0' + sfx, [hit(walk(5, kh, 900, rid=rid, rev=rev, span=kh + 1))]))
            reads.append(Read('qs0-rs0' + sfx, [hit(walk(5, kh, kh, rid=rid, rev=rev, span=kh + 1))]))
            reads.append(Read('qs1-rs1' + sfx, [hit(walk(5, kh + 1, kh + 1, rid=rid, rev=rev, span=kh + 2))]))
            # a first k-mer that hangs over the target's start: rs0 is clamped at 0 and the left window starts there
            reads.append(Read('rs0-clamp' + sfx, [hit(walk(5, kh + 3, 900, rid=rid, rev=rev, span=k))]))
            # the last anchor on the last base of the read and of the target: the shortest right window there is
            a = walk(5, 3000, 900, rid=rid, rev=rev, span=k)
            reads.append(Read('last-base' + sfx, [hit(a)], qlen=(a[-1][1] & 0xffffffff) + 1))
        batches.append(Batch('ends-k%d' % k, reads, k=k))
        # ... of the target too (targets of different lengths: the length is looked up by rid)
        a = walk(5, 3000, 900, rid=1, span=k)
        tl = [TLEN, (a[-1][0] & 0xffffffff) + 1, 5000]
        batches.append(Batch('ends-tlen-k%d' % k, [Read('t-last-base', [hit(a)]), Read('t2', [hit(walk(6, 3000, 900, rid=2, rev=1, span=k))]),
                                                    Read('both-last', [hit(a)], qlen=(a[-1][1] & 0xffffffff) + 1)], k=k, tlens=tl))
    return batches


# ---- fix_bad_ends ----------------------------------------------------------------------------------------------------------------
def fix_family():
    reads = []
    # trimming at the front, at the back, at both; a gap pair further in gives the filter a range behind the trimmed front
    reads.append(Read('front', [hit(walk(40, 3000, 900, gaps={1: 30}))]))
    reads.append(Read('front-2', [hit(walk(40, 3000, 900, gaps={1: 30, 2: -30}))]))
    reads.append(Read('back', [hit(walk(40, 3000, 900, gaps={39: -30}))]))
    reads.append(Read('back-2', [hit(walk(40, 3000, 900, gaps={38: 25, 37: 20}))]))
    reads.append(Read('both', [hit(walk(40, 3000, 900, gaps={1: 30, 38: -30}))]))
    reads.append(Read('both-filter', [hit(walk(60, 3000, 900, gaps={2: 30, 20: 30, 24: -30, 57: -30}))]))
    # the shortest hit a trim can leave (both scans keep two anchors): the filter then looks at two anchors of a longer mask
    reads.append(Read('cnt3-front', [hit(walk(3, 3000, 900, gaps={1: 30, 2: 30}))]))
    reads.append(Read('to-two-front', [hit(walk(8, 3000, 900, gaps={i: 30 * (-1) ** i for i in range(1, 7)}), mlen=100000)]))
    reads.append(Read('to-two-both', [hit(walk(8, 3000, 900, d=16, gaps={1: 30, 2: -30, 3: 30, 5: 30, 6: -20, 7: 20}), mlen=100000)]))
    reads.append(Read('to-three', [hit(walk(9, 3000, 900, d=16, gaps={1: 30, 2: -30, 3: 30, 6: 30, 7: -20, 8: 20}), mlen=100000)]))
    # each stop condition first: the chain length l (long steps), the match count m (short steps, a large mlen), mlen / 2 (the usual).
    # A bad step into the last anchor a scan looks at trims the hit (-in), one anchor further it is never seen (-out)
    for name, n, d, g, mlen, front_in, back_in in (('l', 12, 300, 600, 100000, 4, 8), ('m', 90, 15, 300, 100000, 33, 57), ('mlen', 30, 20, 100, 150, 4, 26)):
        reads.append(Read('stop-%s-in' % name, [hit(walk(n, 3000, 900, d=d, gaps={front_in: g}), mlen=mlen)]))
        reads.append(Read('stop-%s-out' % name, [hit(walk(n, 3000, 900, d=d, gaps={front_in + 1: -g}), mlen=mlen)]))
        reads.append(Read('stop-%s-back-in' % name, [hit(walk(n, 3000, 900, d=d, gaps={back_in: -g}), mlen=mlen)]))
        reads.append(Read('stop-%s-back-out' % name, [hit(walk(n, 3000, 900, d=d, gaps={back_in - 1: g}), mlen=mlen)]))
    reads.append(Read('stop-never', [hit(walk(6, 3000, 900, gaps={4: 60}), mlen=100000)]))
    # a joined chain's first anchor stops either scan: the bad step behind it stays inside the hit
    reads.append(Read('lj-front', [hit(walk(30, 3000, 900, gaps={3: 40}, flags={2: SEED_LONG_JOIN}), mlen=100000)]))
    reads.append(Read('lj-front-1', [hit(walk(30, 3000, 900, gaps={1: 40}, flags={1: SEED_LONG_JOIN}), mlen=100000)]))
    reads.append(Read('lj-back', [hit(walk(30, 3000, 900, gaps={26: 40}, flags={27: SEED_LONG_JOIN}), mlen=100000)]))
    reads.append(Read('lj-back-last', [hit(walk(30, 3000, 900, gaps={29: 40}, flags={29: SEED_LONG_JOIN}), mlen=100000)]))
    reads.append(Read('lj-none', [hit(walk(30, 3000, 900, gaps={3: 40, 26: 40}), mlen=100000)]))
    return [Batch('fix', reads), Batch('fix-bw100', reads, bw=100, min_chain_score=20)]


# ---- filter_bad_seeds ------------------------------------------------------------------------------------------------------------
def alternating(first, n, every, g=30):
    return {first + j * every: g * (-1) ** j for j in range(n)}


def filter_family():
    reads = []
    reads.append(Read('k0', [hit(walk(60, 3000, 900, gaps={30: 10, 35: -10}))]))           # |gap| = min_gap: no entry
    reads.append(Read('k1', [hit(walk(60, 3000, 900, gaps={30: 30, 35: -10}))]))
    reads.append(Read('k2', [hit(walk(60, 3000, 900, gaps={30: 30, 35: -30}))]))
    reads.append(Read('k2-same-sign', [hit(walk(60, 3000, 900, gaps={30: 30, 35: 30}))]))
    reads.append(Read('k2-11', [hit(walk(60, 3000, 900, gaps={30: 11, 35: -11}))]))
    # the threshold: diff = 2 * min(n_ins, n_del) is even, so 40 (kept) and 42 (marked) are its two sides
    reads.append(Read('diff40', [hit(walk(60, 3000, 900, gaps={30: 20, 35: -25}))]))
    reads.append(Read('diff42', [hit(walk(60, 3000, 900, gaps={30: 21, 35: -25}))]))
    reads.append(Read('diff40-3', [hit(walk(60, 3000, 900, gaps={30: 11, 33: -20, 36: 11}))]))
    reads.append(Read('diff42-3', [hit(walk(60, 3000, 900, gaps={30: 11, 33: -21, 36: 11}))]))
    # runs longer than max_ext_cnt
    reads.append(Read('run12', [hit(walk(120, 3000, 900, d=16, gaps=alternating(30, 12, 3)))]))
    reads.append(Read('run25', [hit(walk(200, 3000, 900, d=16, gaps=alternating(40, 25, 4, 21)))]))
    reads.append(Read('run11', [hit(walk(120, 3000, 900, d=16, gaps={30 + 3 * j: (11 + 2 * j) * (-1) ** j for j in range(11)}))]))
    # the max_ext_len break: the partner lies more than max_gap / 2 bases behind the anchor before the entry
    reads.append(Read('far', [hit(walk(200, 3000, 900, gaps={30: 30, 160: -30}))]))
    reads.append(Read('far-edge-in', [hit(walk(200, 3000, 900, d=20, gaps={30: 40, 152: -30}))]))      # 2500 bases: on the limit
    reads.append(Read('far-edge-out', [hit(walk(200, 3000, 900, d=20, gaps={30: 40, 153: -30}))]))
    # a larger maximum found while inside an earlier range (its partner is beyond the first entry's reach): the marking waits
    reads.append(Read('delayed', [hit(walk(260, 3000, 900, gaps={30: 25, 32: -11, 34: -30, 152: 60}))]))
    reads.append(Read('delayed-2', [hit(walk(260, 3000, 900, gaps={30: 25, 32: -11, 34: -30, 152: 60, 154: -90, 200: 30, 204: -30}))]))
    # entries on the word boundaries of a 64-bit mask, and an all-zero word between two entries
    for p in (63, 64, 65, 127, 128):
        reads.append(Read('bit%d' % p, [hit(walk(150, 3000, 900, d=16, gaps={p - 9: 30, p: -30, p + 7: 12}))]))
        reads.append(Read('bit%d-first' % p, [hit(walk(150, 3000, 900, d=16, gaps={p: 30, p + 1: -30}))]))
    reads.append(Read('bits-all', [hit(walk(150, 3000, 900, d=16, gaps={63: 30, 64: -30, 65: 30, 127: -30, 128: 30}))]))
    reads.append(Read('zero-word', [hit(walk(230, 3000, 900, d=16, gaps={60: 30, 200: -30}))]))
    reads.append(Read('zero-words-3', [hit(walk(330, 3000, 900, d=8, gaps={63: 30, 320: -30}, span=8))]))
    reads.append(Read('word-edges', [hit(walk(330, 3000, 900, d=8, gaps={64: 30, 128: -30, 192: 30, 256: -30}, span=8))]))
    # marked or tandem anchors are skipped by the fills, but never the last anchor of the hit
    reads.append(Read('tandem', [hit(walk(60, 3000, 900, flags={10: SEED_TANDEM, 11: SEED_TANDEM, 30: SEED_TANDEM}))]))
    reads.append(Read('tandem-last', [hit(walk(60, 3000, 900, flags={58: SEED_TANDEM, 59: SEED_TANDEM}))]))
    reads.append(Read('marked-last', [hit(walk(60, 3000, 900, flags={57: SEED_IGNORE, 58: SEED_IGNORE, 59: SEED_IGNORE}))]))
    reads.append(Read('marked-last-2', [hit(walk(2, 3000, 900, flags={1: SEED_IGNORE}))]))
    # an entry at the very last anchor (the back scan is stopped by a joined chain / never trims under a long first span)
    reads.append(Read('k-at-last-lj', [hit(walk(60, 3000, 900, gaps={54: 30, 59: -30}, flags={59: SEED_LONG_JOIN}))]))
    reads.append(Read('k-at-last-span', [hit(walk(60, 3000, 900, gaps={54: 30, 59: -30}, spans={59: 255}))]))
    reads.append(Read('k-at-last-130', [hit(walk(130, 3000, 900, d=16, gaps={120: 30, 129: -30}, spans={129: 200}))]))
    return [Batch('filter', reads), Batch('filter-gap2000', reads, max_gap=2000)]


# ---- the LDS edge (1024 anchors) and the mask edge (8192 anchors) -----------------------------------------------------------------
def edge_reads(edge, about, more=True):
    reads = []
    for cnt in (edge - 1, edge, edge + 1, about):
        gaps = {}
        gaps.update({edge - 4: 30, edge + 5: -30} if cnt >= edge + 20 else {cnt - 14: 30, cnt - 8: -30})
        gaps.update({100: 30, 104: -30})
        if cnt >= edge + 60:
            gaps.update({edge + 30: 25, edge + 36: -25, edge + 50: 30})          # a range, and a single entry, entirely beyond the edge
        reads.append(Read('cnt%d' % cnt, [hit(walk(cnt, 3000, 900, d=16, gaps=gaps))]))
    # big gaps on both sides of the edge: one range that ends on it, one that starts on it, entries on the edge itself
    reads.append(Read('ends-on-edge', [hit(walk(about, 3000, 900, d=16, gaps={edge - 6: 30, edge: -30}))]))
    reads.append(Read('starts-on-edge', [hit(walk(about, 3000, 900, d=16, gaps={edge: 30, edge + 6: -30}))]))
    reads.append(Read('around-edge', [hit(walk(about, 3000, 900, d=16, gaps={edge - 1: 30, edge + 1: -30}))]))
    if more:
        reads.append(Read('before-edge', [hit(walk(about, 3000, 900, d=16, gaps={edge - 7: 30, edge - 1: -30}))]))
        reads.append(Read('tandem-edge', [hit(walk(about, 3000, 900, d=16, flags={i: SEED_TANDEM for i in range(edge - 3, edge + 3)}))]))
    # the hit does not start the read's list, and its front is trimmed: in-hit positions and anchor indices differ
    reads.append(Read('offset', [walk(37, 100, 100, rid=1), hit(walk(about, 3000, 900, d=16, gaps={2: 30, edge - 3: 30, edge + 4: -30})),
                                 walk(5, 390000, 300000)]))
    return reads


def lds_family():
    return [Batch('lds-edge', edge_reads(1024, 1100))]


def mask_family():
    return [Batch('mask-edge', edge_reads(8192, 8300, more=False))]


# ---- neighbours: the anchors before and behind the hit in the read's list ----------------------------------------------------------
def neighbours_family():
    reads = []
    H = lambda **kw: hit(walk(12, 50000, 20000, **kw))      # noqa: E731  (the hit: first k-mer starts at 49986 / 19986)
    for side in ('left', 'right'):
        def nb(n, dt=0, dq=0, **kw):
            """n anchors on the hit's far side, 100 bases apart, the nearest 500 bases off (+ dt / dq)"""
            if side == 'left':
                return walk(n, 49500 + dt - 100 * (n - 1), 19500 + dq - 100 * (n - 1), d=100, **kw)
            return walk(n, 50000 + 11 * 20 + 500 + dt, 20000 + 11 * 20 + 500 + dq, d=100, **kw)

        def rd(name, near, far=None, **kw):
            parts = [near, H(**kw)] if side == 'left' else [H(**kw), near]
            if far is not None:
                parts = [far] + parts if side == 'left' else parts + [far]
            reads.append(Read('%s-%s' % (side, name), parts, qlen=40000))

        other = walk(6, 1000, 1000, rid=1)
        for n in (0, 1, 3, 4, 5, 9):        # min_cnt and min_cnt + 1 qualifying anchors, and the walk ending at the list's end
            if n:
                rd('n%d' % n, nb(n))
            else:
                reads.append(Read('%s-n0' % side, [H()], qlen=40000))
            rd('n%d-then-other' % n, nb(n) if n else [], other)
        # anchors that fail one of the two inequalities do not count
        for which, (dt, dq) in (('x', (600, 0)), ('y', (0, 600)), ('xy', (600, 600))):
            if side == 'left':
                mixed = nb(3) + walk(2, 49500 + dt + 50, 19500 + dq + 50, d=10)
            else:
                mixed = walk(2, 50720 - dt - 60, 20720 - dq - 60, d=10) + nb(3)
            rd('fail-%s' % which, mixed)
            rd('fail-%s-then-4th' % which, mixed, nb(1, -3000 if side == 'left' else 3000, -3000 if side == 'left' else 3000))
        # the first / last k-mer edge itself: one base decides
        for d in (-1, 0, 1):
            edge = walk(1, 49986 + K - 1 + d, 19000) if side == 'left' else walk(1, 50220 + d, 21000)
            rd('edge%+d' % d, (nb(3) + edge) if side == 'left' else (edge + nb(3)))
        # another target or the other strand ends the walk before enough anchors were seen
        rd('cut-by-target', nb(2), nb(4, -3000, -3000) + walk(1, 48000, 18000, rid=1) if side == 'left' else
           walk(1, 53000, 23000, rid=1) + nb(4, 3000, 3000))
        rd('cut-by-strand', nb(2), nb(4, -3000, -3000) + walk(1, 48000, 18000, rev=1) if side == 'left' else
           walk(1, 53000, 23000, rev=1) + nb(4, 3000, 3000))
        rd('rev', nb(5, rev=1, rid=2), rev=1, rid=2)
        rd('far-neighbours', nb(5, -7000 if side == 'left' else 7000, -7000 if side == 'left' else 7000))
    # neighbours close to the target's start: rs1 is clamped
    reads.append(Read('left-rs1-clamp', [walk(4, 20, 19000, d=2, span=3), hit(walk(12, 300, 20000))]))
    return [Batch('neighbours', reads), Batch('neighbours-min-cnt1', reads, min_cnt=1), Batch('neighbours-gap300', reads, max_gap=300)]


# ---- limits -----------------------------------------------------------------------------------------------------------------------
def limits_family():
    out = []
    for name, opt in (('default', {}), ('gap300', dict(max_gap=300)), ('a1-q10-e3', dict(a=1, q=10, e=3)), ('ksw0', dict(min_ksw_len=0)),
                      ('ksw-huge', dict(min_ksw_len=1000000)), ('ksw45', dict(min_ksw_len=45))):
        reads = []
        for q0 in (8, 9, 10, 12, 17, 18, 150, 307, 308, 4000, 5006, 5007, 5008, 9000):      # overhangs around l * a = q and around max_gap
            reads.append(Read('lead%d' % q0, [hit(walk(30, 20000, q0, span=8))]))
            reads.append(Read('lead%d-rev' % q0, [hit(walk(30, 20000, q0, rev=1, rid=1, span=8))]))
        for t0 in (8, 9, 10, 12, 150, 400, 4000):                                          # the target's start is closer than the read's
            reads.append(Read('tlead%d' % t0, [hit(walk(30, t0, 3000, span=8))]))
            reads.append(Read('tlead%d-far' % t0, [hit(walk(30, t0, 9000, span=8))]))
        for t0 in (20, 50):
            reads.append(Read('tlead%d-near' % t0, [hit(walk(30, t0, 200, span=8))]))
        for tail in (8, 9, 10, 11, 12, 150, 299, 300, 301, 4999, 5000, 5001, 9000):
            a = walk(30, 20000, 900)
            reads.append(Read('tail%d' % tail, [hit(a)], qlen=(a[-1][1] & 0xffffffff) - 7 + tail))
        reads.append(Read('gaps', [hit(walk(40, 20000, 900, d=23, gaps={9: 250, 20: -180, 30: 90}))]))
        out.append(Batch('limits-' + name, reads, **opt))
        # the target's end is closer than the read's
        for ttail in (8, 10, 150, 1000):
            a = walk(30, 20000, 900)
            tl = (a[-1][0] & 0xffffffff) - 7 + ttail
            out.append(Batch('limits-%s-ttail%d' % (name, ttail), [Read('ttail', [hit(a)], qlen=12000), Read('ttail-short-read', [hit(a)], qlen=(a[-1][1] & 0xffffffff) + 201)],
                             tlens=(tl, TLEN, TLEN), **opt))
    return out


# ---- refused windows ----------------------------------------------------------------------------------------------------------------
def refused_family():
    reads = [Read('plain', [hit(walk(40, 20000, 900))]),
             Read('long-fill', [hit(walk(40, 20000, 900, gaps={20: 700}))]),
             Read('long-fill-t', [hit(walk(40, 20000, 900, gaps={20: -700}))]),
             Read('short-ends', [hit(walk(40, 100, 100))], qlen=100 + 39 * 20 + 90),
             Read('split-inv', [hit(walk(40, 20000, 900), split_inv=1)])]
    return [Batch('refused-%d' % m, reads, max_sw_mat=m) for m in (0, 1, 30000, 35000, 39999, 40000, 100000, 185000, 1000000, 100000000)]


# ---- a joined chain inside a hit ------------------------------------------------------------------------------------------------------
def long_join_family():
    reads = [Read('lj-q', [hit(walk(40, 20000, 900, gaps={20: 900}, flags={20: SEED_LONG_JOIN}))]),
             Read('lj-t', [hit(walk(40, 20000, 900, gaps={20: -900}, flags={20: SEED_LONG_JOIN}))]),
             Read('lj-short', [hit(walk(40, 20000, 900, gaps={17: 5}, flags={17: SEED_LONG_JOIN}))]),       # forced although shorter than min_ksw_len
             Read('lj-two', [hit(walk(60, 20000, 900, gaps={20: 2600, 40: -1200}, flags={20: SEED_LONG_JOIN, 40: SEED_LONG_JOIN}))]),
             Read('lj-marked', [hit(walk(60, 20000, 900, gaps={18: 30, 22: -30}, flags={20: SEED_LONG_JOIN}))]),   # ... but not when marked
             Read('lj-tandem', [hit(walk(60, 20000, 900, flags={20: SEED_LONG_JOIN | SEED_TANDEM}))])]
    return [Batch('long-join', reads), Batch('long-join-refused', reads, max_sw_mat=500000)]


# ---- rounds: the remainder of a hit cut at a z-drop, planned on the anchors as the first pass left them ---------------------------------
def rounds_family():
    first = [Read('r%d' % j, [walk(5, 100, 100, rid=1),
                              hit(walk(120, 20000, 900, d=16, gaps={10: 30, 14: -30, 50: 25, 58: -40, 100: 30, 101: -30})),
                              walk(6, 30000, 9000)]) for j in range(5)]
    b1 = Batch('rounds-first', first)
    second = []
    for (cut, inv), r, (_, left, _) in zip(((12, 0), (12, 1), (54, 1), (59, 0), (101, 1)), first, b1.ref()):
        assert any(y & SEED_IGNORE for _, y in left)
        as_, cnt, mlen, _ = r.hits[0]
        rd = Read('%s-from%d' % (r.name, cut), [left], qlen=r.qlen)
        rd.hits = [(as_ + cut, cnt - cut, fuzzy_mlen(left[as_ + cut:as_ + cnt]), inv)]
        second.append(rd)
    return [b1, Batch('rounds-second', second), Batch('rounds-second-zdrop', second, zdrop=300, zdrop_inv=77)]


# ---- batch: several reads with several hits each, handed over out of order; long hits before short ones on one block ------------------
def batch_family():
    rng = np.random.default_rng(7)
    reads = []
    for j in range(6):
        parts, t = [], 2000
        nh = int(rng.integers(2, 6))
        for h in range(nh):
            n = int(rng.integers(1, 90))
            rid, rev = int(rng.integers(0, 3)), int(rng.integers(0, 2))
            gaps = {int(g): int(rng.choice([-45, -30, -12, 12, 25, 40])) for g in rng.integers(1, max(2, n), size=n // 6)}
            a = walk(n, t, int(rng.integers(20, 4000)), d=int(rng.integers(12, 30)), gaps=gaps, rid=rid, rev=rev)
            parts.append(hit(a, split_inv=int(rng.integers(0, 2))) if h == 0 or rng.random() < 0.8 else a)
            t = (a[-1][0] & 0xffffffff) + int(rng.integers(30, 3000))
        n_hits = sum(1 for p in parts if isinstance(p, tuple))
        reads.append(Read('mix%d' % j, parts, order=[int(v) for v in rng.permutation(n_hits)]))
    # one block takes these in turn: the 3 and 70 anchors must not see what the 8300 before them left in the staging arrays
    big = walk(8300, 3000, 900, d=16, gaps={30: 30, 33: -30, 69: 25, 8185: 30, 8200: -30, 8250: 30, 8260: -30})
    small = walk(3, 200000, 500, rid=1)
    mid = walk(70, 250000, 3000, rid=2, rev=1, gaps={30: 30, 35: -30})
    reads.append(Read('big-small-mid', [hit(big), hit(small), hit(mid)]))
    reads.append(Read('mid-big-small-same-target', [hit(walk(70, 1000, 300, gaps={30: 30, 35: -30})), hit(walk(8200, 3000, 2000, d=16, gaps={64: 30, 8190: -30})),
                                                    hit(walk(3, 300000, 150000))], order=[1, 2, 0]))
    return [Batch('batch', reads)]


FAMILIES = dict(ends=ends_family, fix_bad_ends=fix_family, filter_bad_seeds=filter_family, lds_edge=lds_family, mask_edge=mask_family,
                neighbours=neighbours_family, limits=limits_family, refused=refused_family, long_join=long_join_family, rounds=rounds_family,
                batch=batch_family)


def families():
    return {name: make() for name, make in FAMILIES.items()}


def validate(b):
    """what the stage entry checks before any launch, restated: every test input passes it"""
    for r in b.reads:
        n_a = len(r.anchors)
        assert r.qlen > 0 and n_a > 0, (b.name, r.name)
        for x, y in r.anchors:
            rid = (x << 1 & (1 << 64) - 1) >> 33
            assert rid < len(b.tlens) and 0 <= (x & 0xffffffff) < min(b.tlens[rid], 1 << 31), (b.name, r.name, 'x')
            assert 0 <= (y & 0xffffffff) < r.qlen and 1 <= (y >> 32 & 0xff) and not y >> 43, (b.name, r.name, 'y')
        used = []
        for as_, cnt, mlen, inv in r.hits:
            assert cnt >= 1 and as_ >= 0 and as_ + cnt <= n_a, (b.name, r.name, 'range')
            for p, c in zip(r.anchors[as_:as_ + cnt], r.anchors[as_ + 1:as_ + cnt]):
                assert p[0] >> 32 == c[0] >> 32 and (p[0] & 0xffffffff) < (c[0] & 0xffffffff) and (p[1] & 0xffffffff) < (c[1] & 0xffffffff), (b.name, r.name)
            used.append((as_, as_ + cnt))
        used.sort()
        assert all(e <= s for (_, e), (s, _) in zip(used, used[1:])), (b.name, r.name, 'overlap')
