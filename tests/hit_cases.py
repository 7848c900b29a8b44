"""Seeded chains for the tests of the hit stage (test_hit_ref.py on the CPU, test_hit_select_gpu.py on the GPU): synthetic anchors,
laid out so that hit selection meets its edges.  A read is a list of chains; a chain is a list of (x, y) anchor words as the
chain stage leaves them (x = strand << 63 | rid << 32 | last target base of the k-mer, y = span << 32 | last read base on the
chain's strand) and a score.  mlen / blen of a chain follow from its anchors by the mm_cal_fuzzy_len rule.

families() -> {name: [Batch]}; a batch is one call of the stage: options, reads, and the max_chains values to run it with."""
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np

from hit_ref import fuzzy_len

K = 15
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Chain:
    def __init__(self, anchors, score):
        self.a, self.score = [(int(x), int(y)) for x, y in anchors], int(score)
        self.mlen, self.blen = fuzzy_len(self.a, 0, len(self.a))


class Read:
    def __init__(self, name, qlen, chains, rng, expect=None):
        self.name, self.qlen, self.expect = name, int(qlen), expect
        assert len({c.a[0][0] for c in chains}) == len(chains), name       # the order of the chains follows their first anchors
        self.sorted = sorted(chains, key=lambda c: c.a[0][0])
        pool = list(self.sorted)
        if len(pool) > 1:     # pool order: arbitrary, and never the order of the first anchors
            perm = rng.permutation(len(pool))
            if all(perm[i] == i for i in range(len(pool))):
                perm = np.roll(perm, 1)
            pool = [pool[i] for i in perm]
        self.pool = pool

    def u_a(self, chains=None):
        """(u, anchors) of the chains in the order of their first anchors: what the oracle and hit_ref take"""
        chains = self.sorted if chains is None else chains
        return [c.score << 32 | len(c.a) for c in chains], [p for c in chains for p in c.a]


class Batch:
    def __init__(self, name, reads, max_chains=(0,), k=K, **opt):
        self.name, self.reads, self.max_chains, self.k, self.opt = name, reads, tuple(max_chains), k, opt

    def arrays(self):
        """the batch as mapper.hit_select_batch takes it (chains and anchors in pool order)"""
        chain_off, anchor_off, u, fx, fy, lx, ly, ml, bl, anchors = [0], [0], [], [], [], [], [], [], [], []
        for r in self.reads:
            for c in r.pool:
                u.append(c.score << 32 | len(c.a))
                fx.append(c.a[0][0]); fy.append(c.a[0][1]); lx.append(c.a[-1][0]); ly.append(c.a[-1][1])
                ml.append(c.mlen); bl.append(c.blen)
                anchors.extend(c.a)
            chain_off.append(len(u)); anchor_off.append(len(anchors))
        un = lambda v: np.array(v, dtype=np.uint64)  # noqa: E731
        return dict(q_len=np.array([r.qlen for r in self.reads], dtype=np.int32), names=[r.name for r in self.reads],
                    chain_off=np.array(chain_off, dtype=np.int64), u=un(u), recs=(un(fx), un(fy), un(lx), un(ly), np.array(ml, dtype=np.int32),
                                                                                     np.array(bl, dtype=np.int32)),
                    anchor_off=np.array(anchor_off, dtype=np.int64), anchors=un(anchors).reshape(-1, 2))


def anchor(rid, rev, t, q, span=K):
    assert t >= 0 and q >= 0
    return (rev << 63 | rid << 32 | t, span << 32 | q)


def chain(rid, rev, ts, qs, lq, n, score, lt=None, rng=None):
    """n anchors from the hit that covers [qs, qs + lq) on the chain's strand of the read and [ts, ts + lt) of target rid (ts < 0:
    a first k-mer that hangs over the target's start); the first and last anchor sit on the interval ends, the others in between
    (with rng: at random places, so that mlen and blen differ)"""
    lt = lq if lt is None else lt
    assert n >= 1 and (n == 1 or (lq >= K + n - 1 and lt >= K + n - 1))
    if n == 1:
        assert lq == K and lt == K
        return Chain([anchor(rid, rev, ts + K - 1, qs + K - 1)], score)

    def places(length):
        if rng is None or n == 2:
            return [round(i * (length - K) / (n - 1)) for i in range(n)]
        inner = sorted(int(v) for v in rng.choice(np.arange(1, length - K), size=n - 2, replace=False))
        return [0] + inner + [length - K]
    return Chain([anchor(rid, rev, ts + K - 1 + dt, qs + K - 1 + dq) for dq, dt in zip(places(lq), places(lt))], score)


def on_read(qlen, rev, qs, lq):
    """start, on the chain's strand, of the hit that covers [qs, qs + lq) of the read"""
    return qs if not rev else qlen - (qs + lq)


# ---- counts: the bounds of the instantiations, of the 64-lane rank sorts and of max_chains ---------------------------------------
COUNTS = (0, 1, 2, 47, 48, 49, 63, 64, 65, 127, 128, 129, 383, 384, 385)


def counts_family(seed=101):
    rng = np.random.default_rng(seed)
    reads = []
    for kind in ('disjoint', 'stacked', 'random'):
        for nc in COUNTS:
            qlen = 60 * 400 + 500
            chains = []
            tpos = rng.permutation(4000)[:nc] * 100 + 50            # distinct first anchors
            for c in range(nc):
                n = int(rng.integers(3, 7))
                rev = int(rng.integers(0, 2))
                if kind == 'disjoint':
                    lq, qs = int(rng.integers(30, 56)), 60 * c + 10
                elif kind == 'stacked':
                    lq, qs = int(rng.integers(380, 400)), 1000 + int(rng.integers(0, 10))
                else:
                    lq = int(rng.integers(30, 900))
                    qs = int(rng.integers(0, qlen - lq))
                score = int(rng.integers(40, 400)) if kind != 'stacked' else int(rng.integers(300, 400))
                chains.append(chain(int(rng.integers(0, 9)), rev, int(tpos[c]), on_read(qlen, rev, qs, lq), lq, n, score, rng=rng))
            reads.append(Read('%s-%d' % (kind, nc), qlen, chains, rng))
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    return [Batch('counts', reads, max_chains=(0, 3, 48)), Batch('counts-N50', reads, max_chains=(0,), best_n=50, pri_ratio=0.5)]


# ---- ties: stacks of chains with one score and count, ordered by the (name, qlen, seed) hash ------------------------------------
TIE_NAMES = ('read/1', 'read/2', 'a', 'strain_read_with_a_long_name_0123456789', '')


def tie_chains(rng, m, qlen, n_anchor=4):
    """m chains with one score and count over (nearly) one read interval, on m targets and both strands"""
    out = []
    for c in range(m):
        rev = c & 1
        lq = 700 + (c % 3)           # no two hits with the same coordinates on one target
        out.append(chain(c, rev, 5000 + 37 * c, on_read(qlen, rev, 200, lq), lq, n_anchor, 600, rng=rng))
    return out


def ties_family(seed=202):
    rng = np.random.default_rng(seed)
    stacks = [(m, tie_chains(rng, m, 2000)) for m in (10, 23, 48, 60)]
    batches = []
    for seed_opt, best_n in ((11, 5), (7, 5), (12345, 50), (0, 1)):
        reads = []
        for m, chains in stacks:
            for name in TIE_NAMES:
                reads.append(Read(name, 2000, chains, rng))
            for qlen in (2001, 2500):    # (the same chains on a longer read: the reverse-strand hits move, the hash changes)
                reads.append(Read(TIE_NAMES[0], qlen, chains, rng))
        batches.append(Batch('ties-seed%d-N%d' % (seed_opt, best_n), reads, seed=seed_opt, best_n=best_n))
    return batches


# ---- mask: overlap fractions at mask_level +- one base ---------------------------------------------------------------------------
def mask_family(seed=303):
    rng = np.random.default_rng(seed)
    batches = []
    for mask in (0.5, 0.3):
        reads = []
        m = Fraction(mask).limit_denominator(10)
        for g in range(24):
            qlen = 6000
            n_pri = 1 + g % 3
            rev = g & 1
            # primaries (higher scores) side by side with gaps; the candidate starts inside the first and runs over the others
            if n_pri < 3:
                lens = [int(rng.integers(600, 1200)) for _ in range(n_pri)]
                gaps = [int(rng.integers(20, 200)) for _ in range(n_pri)]
            else:   # a primary inside the candidate masks it unless the gaps between the primaries are about (1 - mask) of its length
                lens = [int(rng.integers(200, 300)) for _ in range(n_pri)]
                gaps = [int(rng.integers(200, 300)) if mask == 0.5 else int(rng.integers(500, 660)) for _ in range(n_pri)]
            pri, x = [], 500
            for ln, gp in zip(lens, gaps):
                pri.append((x, x + ln))
                x += ln + gp
            def masked(s, e):     # per primary, the mask test in exact arithmetic: only to find where the verdict turns
                cov = sorted((max(a, s), min(b, e)) for a, b in pri if b > s and a < e)
                xx, unc = s, 0
                for a, b in cov:
                    unc += max(0, a - xx)
                    xx = max(xx, b)
                unc += max(0, e - xx)
                res = []
                for a, b in pri:
                    if b <= s or a >= e:
                        continue
                    ol = min(b, e) - max(a, s)
                    mn, mx = min(b - a, e - s), max(b - a, e - s)
                    res.append((ol * mx - unc * mn) * m.denominator > m.numerator * mn * mx)
                return any(res)
            # the candidate ends in or behind the last primary; its start moves through the first one, a base at a time
            s0 = None
            for _ in range(40):
                e = int(rng.integers(pri[-1][0] + 20, pri[-1][1] + 150))
                flips = [s for s in range(pri[0][0] + 1, min(pri[0][1] - 20, e - 61)) if masked(s, e) != masked(s + 1, e)]
                if flips:
                    s0 = flips[int(rng.integers(0, len(flips)))]
                    break
            if s0 is None:
                continue
            cnt_p = 6
            for d in (-1, 0, 1, 2):
                for cnt_c in (cnt_p, cnt_p - 1):
                    chains = [chain(j, rev, 3000 * (j + 1), on_read(qlen, rev, a, b - a), b - a, cnt_p, 2000 - 10 * j, rng=rng)
                              for j, (a, b) in enumerate(pri)]
                    s = s0 + d
                    chains.append(chain(7, rev, 40000, on_read(qlen, rev, s, e - s), e - s, cnt_c, 1700, rng=rng))
                    reads.append(Read('mask%g-g%d-d%d-c%d' % (mask, g, d, cnt_c), qlen, chains, rng, expect=('flip', 'mask%g-g%d-c%d' % (mask, g, cnt_c))))
        batches.append(Batch('mask-%g' % mask, reads, mask_level=mask))
    return batches


# ---- select: -p, min_diff, -N, twins, parents that the in-place compaction has overwritten --------------------------------------
def alias_read(rng, name, qlen=8000):
    """A [0, 1000) with a dropped secondary B, primaries C and D further along, and a secondary E of C that mm_select_sub judges
    against what the compaction has moved into C's old place (D)"""
    sa = int(rng.integers(900, 1100))
    sb = int(sa * 0.5)
    sc = int(rng.integers(380, 420))
    sd = int(sc * rng.uniform(0.70, 0.78))
    se = int(sd * 0.8) + int(rng.integers(1, 8))       # >= 0.8 * D, < 0.8 * C, < C - 30
    sh = int(rng.integers(0, 300))
    return Read(name, qlen, [chain(0, 0, 100, sh, 1000, 8, sa, rng=rng), chain(1, 0, 100, sh + 100, 800, 6, sb, rng=rng),
                             chain(0, 0, 5000, sh + 2000, 1000, 7, sc, rng=rng), chain(0, 0, 9000, sh + 4000, 1000, 6, sd, rng=rng),
                             chain(2, 0, 100, sh + 2100, 800, 5, se, rng=rng)], rng)


def secondaries_read(rng, name, s_pri, scores, qlen=4000, twin=False):
    chains = [chain(0, 0, 1000, 500, 2000, 10, s_pri, rng=rng)]
    for j, s in enumerate(scores):
        rev = j & 1
        lq = 1900 - j
        chains.append(chain(1 + j, rev, 1000 + 3 * j, on_read(qlen, rev, 520, lq), lq, 5, max(1, s), rng=rng))
    if twin:   # the same read interval, target and target interval as the primary, on the other strand
        chains.append(Chain([anchor(0, 1, t, q) for t, q in ((1014, qlen - 2500 + 14), (1900, qlen - 1500), (2999, qlen - 501))], s_pri - 1))
    return Read(name, qlen, chains, rng)


def select_family(seed=404):
    rng = np.random.default_rng(seed)
    batches = []
    for pri_ratio in (0.8, 1.0, 0.0):
        for best_n in (1, 5, 50):
            reads = []
            for s_pri in (100, 1000, 1005, 1001, 4999, 12345):
                thr = int(round(s_pri * pri_ratio))
                reads.append(secondaries_read(rng, 'edge-%d' % s_pri, s_pri, [thr - 1, thr, thr + 1, s_pri - 2 * K - 1, s_pri - 2 * K, s_pri - 2 * K + 1]))
            reads.append(secondaries_read(rng, 'many', 900, [899 - j for j in range(60)]))
            reads.append(secondaries_read(rng, 'twin', 900, [880, 870], twin=True))
            reads.extend(alias_read(rng, 'alias-%d' % j) for j in range(6))
            batches.append(Batch('select-p%g-N%d' % (pri_ratio, best_n), reads, pri_ratio=pri_ratio, best_n=best_n))
    return batches


# ---- join: every refusal of mm_join_long just inside and just outside, runs of joins, parents, bystanders -----------------------
JOIN_DEFAULT = dict(max_join_long=20000, max_join_short=2000, min_join_flank_sc=1000, min_join_flank_ratio=0.5)
JOIN_OTHER = dict(max_join_long=5000, max_join_short=500, min_join_flank_sc=300, min_join_flank_ratio=0.25)


def join_pair(rng, name, expect, gq=500, gt=500, la=(1200, 1200), lb=(1200, 1200), sa=3000, sb=2500, rev=0, rid_b=0, rev_b=None, extra=(),
              qlen=70000, ts=20000):
    """two hits of one target one after the other: A covers la = (read, target) bases, B lb, the last anchor of A and the first of
    B are (gq, gt) apart; extra: more chains of the read"""
    rev_b = rev if rev_b is None else rev_b
    qa = 1000
    a = chain(0, rev, ts, qa, la[0], 8, sa, lt=la[1], rng=rng)
    qb, tb = qa + la[0] - 1 + gq - (K - 1), ts + la[1] - 1 + gt - (K - 1)
    b = chain(rid_b, rev_b, tb, qb, lb[0], 7, sb, lt=lb[1], rng=rng)
    return Read(name, qlen, [a, b] + list(extra), rng, expect=expect)


def join_family(seed=505):
    rng = np.random.default_rng(seed)
    batches = []
    for tag, jo in (('default', JOIN_DEFAULT), ('other', JOIN_OTHER)):
        L, S, FS, FR = jo['max_join_long'], jo['max_join_short'], jo['min_join_flank_sc'], jo['min_join_flank_ratio']
        reads = []
        ok, no = ('join', 1), lambda why: ('refused', why)  # noqa: E731
        for rev in (0, 1):
            sfx = '-rev' if rev else ''
            sec = lambda t: chain(0, rev, t, 1100, 900, 5, 2600, rng=rng)  # noqa: E731   a secondary of A that stays
            reads.append(join_pair(rng, 'plain' + sfx, ok, rev=rev))
            # adjacency in the squeezed list: a secondary whose first anchor lies behind those of A and B, or between them
            reads.append(join_pair(rng, 'adjacent-in' + sfx, ok, rev=rev, extra=[sec(50000)]))
            reads.append(join_pair(rng, 'adjacent-out' + sfx, no('adjacency'), rev=rev, extra=[sec(20600)]))
            reads.append(join_pair(rng, 'rid-out' + sfx, no('rid_strand'), rev=rev, rid_b=1))
            reads.append(join_pair(rng, 'strand-out' + sfx, no('rid_strand'), rev=rev, rev_b=1 - rev))
            reads.append(join_pair(rng, 'step-in' + sfx, ok, rev=rev, gq=1, gt=1))
            reads.append(join_pair(rng, 'step-q0-out' + sfx, no('step'), rev=rev, gq=0, gt=5))
            reads.append(join_pair(rng, 'step-qneg-out' + sfx, no('step'), rev=rev, gq=-7, gt=5))
            reads.append(join_pair(rng, 'step-t0-out' + sfx, no('step'), rev=rev, gq=5, gt=0))
            reads.append(join_pair(rng, 'step-tneg-out' + sfx, no('step'), rev=rev, gq=5, gt=-7))
            big = (int(L * FR) + 200, int(L * FR) + 200)
            for gq, gt, exp in ((S, L, ok), (S, L + 1, no('max_join_long')), (L, S, ok), (L + 1, S, no('max_join_long')),
                                (S, S, ok), (S + 1, S + 1, no('max_join_short')), (S + 1, S, ok), (S, S + 1, ok)):
                reads.append(join_pair(rng, 'gap-%d-%d%s' % (gq, gt, sfx), exp, rev=rev, gq=gq, gt=gt, la=big, lb=big, sa=FS + 500, sb=FS + 400))
            # the score threshold (int)((float)FS / L * max_gap + .499), where FS / L * max_gap + .499 comes close to an integer
            for mg in (10, 11, 30, 31, S - 10, S - 9, S + 10, S + 30, L // 2 + 10, L // 2 + 11, L - 10, L - 9):
                t0 = FS * mg // L
                fl = (max(int(mg * FR) + 50, 100),) * 2
                for sc in range(max(0, t0 - 1), t0 + 3):
                    reads.append(join_pair(rng, 'sc-%d-a%d%s' % (mg, sc, sfx), None, rev=rev, gq=min(mg, S), gt=mg, la=fl, lb=fl, sa=sc, sb=max(0, sc - 1)))
                    reads.append(join_pair(rng, 'sc-%d-b%d%s' % (mg, sc, sfx), None, rev=rev, gq=mg, gt=min(mg, S), la=fl, lb=fl, sa=sc + 1, sb=sc))
            # the flank lengths (int)(max_gap * FR), on the read and on the target, on both hits
            for mg in (S // 2 + 1, S // 2, S - 1):
                f = int(mg * FR)
                for which in range(4):
                    for d, exp in ((0, ok), (-1, no('flank0' if which < 2 else 'flank1'))):
                        la, lb = [f + 40, f + 40], [f + 40, f + 40]
                        (la if which < 2 else lb)[which & 1] = f + d
                        reads.append(join_pair(rng, 'flank-%d-%d-%d%s' % (mg, which, d, sfx), exp, rev=rev, gq=mg - 3, gt=mg, la=tuple(la), lb=tuple(lb)))
            # runs of joinable hits, a secondary on the absorbed hit, bystanders below min_cnt
            for run in (3, 4):
                chains, q, t = [], 1000, 30000
                for j in range(run):
                    chains.append(chain(0, rev, t, q, 1200, 6, 3000 - 100 * j, rng=rng))
                    q, t = q + 1200 + 300, t + 1200 + 320
                chains.append(chain(3, rev, 100, 1000 + 1500 + 50, 1100, 5, 2850, rng=rng))      # secondary of the second hit
                chains.append(chain(4, rev, 100, 1000 + 50, 1100, 5, 2840, rng=rng))             # secondary of the first
                chains.append(chain(5, rev, 700, 40000, 20, 2, 500, rng=rng))                    # a primary below min_cnt
                reads.append(Read('run-%d%s' % (run, sfx), qlen=70000, chains=chains, rng=rng, expect=('join', run - 1)))
            small = [chain(5, rev, 700, 40000, 20, 2, 500, rng=rng), chain(6, rev, 900, 45000, K, 1, 400, rng=rng)]
            reads.append(join_pair(rng, 'bystanders-no-join' + sfx, no('rid_strand'), rev=rev, rid_b=1, extra=small))
            reads.append(join_pair(rng, 'bystanders-join' + sfx, ok, rev=rev, extra=small))
            # a first k-mer that hangs over the start of the target: rs is clamped at 0
            reads.append(join_pair(rng, 'rs-clamp' + sfx, ok, rev=rev, ts=-9))
            reads.append(Read('rs-clamp-single' + sfx, 3000, [chain(2, rev, -14, 100, 800, 6, 900, rng=rng)], rng))
        batches.append(Batch('join-' + tag, reads, **{k: v for k, v in jo.items() if JOIN_DEFAULT[k] != v}))
    return batches


# ---- hand-worked cases: (name, options, qlen, hits as (score, qs, qe, rid, rs, re, cnt) on the forward strand, expected) --------
def hand_read(name, qlen, hits, rng):
    return Read(name, qlen, [chain(rid, 0, rs, qs, qe - qs, cnt, score, lt=re - rs) for score, qs, qe, rid, rs, re, cnt in hits], rng)


HAND = (
    # the in-place mm_select_sub: hit 4 is judged against hit 3, which the compaction has moved over its parent 2
    ('aliased-parent', {}, 6000, [(1000, 0, 1000, 0, 0, 1000, 50), (500, 100, 900, 1, 0, 800, 25), (400, 2000, 3000, 0, 5000, 6000, 20),
                                  (300, 4000, 5000, 0, 9000, 10000, 15), (250, 2100, 2900, 2, 0, 800, 12)],
     dict(score=[1000, 400, 300, 250], parent=[0, 1, 2, 1], cnt=[50, 20, 15, 12], subsc=[500, 250, 0, 0], n_sub=[0, 0, 0, 0], sam_pri=[1, 0, 0, 0],
          **{'as': [0, 50, 70, 85]}), dict(aliased_parent=1, drop_ratio=1, kept_2nd=1, resynced=1)),
    # two hits 500 apart on read and target: joined, the anchors of the second marked
    ('join', {}, 9000, [(3000, 1000, 2200, 0, 20000, 21200, 8), (2500, 2685, 3885, 0, 21685, 22885, 7)],
     dict(score=[5500], parent=[0], cnt=[15], mlen=[225], blen=[2885], **{'as': [0]}, sam_pri=[1]),
     dict(joins=1, resynced=1)),
    # three in a row, joined right to left
    ('three-way-join', {}, 9000, [(3000, 1000, 2200, 0, 20000, 21200, 8), (2500, 2500, 3700, 0, 21520, 22720, 7), (2400, 4000, 5200, 0, 23040, 24240, 6)],
     dict(score=[7900], parent=[0], cnt=[21], blen=[4240], **{'as': [0]}, sam_pri=[1]), dict(joins=2, chained_joins=1, resynced=1)),
    # a join, and a primary of two anchors elsewhere that min_cnt = 3 then drops; without the join it would have stayed
    ('join-drops-bystander', {}, 9000, [(3000, 1000, 2200, 0, 20000, 21200, 8), (2500, 2500, 3700, 0, 21520, 22720, 7), (500, 7000, 7020, 1, 100, 120, 2)],
     dict(score=[5500], parent=[0], cnt=[15], **{'as': [0]}), dict(joins=1, dropped_by_min_cnt=1, resynced=1)),
    ('no-join-keeps-bystander', {}, 9000, [(3000, 1000, 2200, 0, 20000, 21200, 8), (2500, 2500, 3700, 1, 21520, 22720, 7), (500, 7000, 7020, 1, 100, 120, 2)],
     dict(score=[3000, 2500, 500], parent=[0, 1, 2], cnt=[8, 7, 2], sam_pri=[0, 0, 0], **{'as': [0, 10, 8]}), dict(joins=0, dropped_by_min_cnt=0, resynced=0)),
    # -N 2: four eligible secondaries, the two best stay
    ('best-n-cut', dict(best_n=2), 4000, [(1000, 500, 2500, 0, 1000, 3000, 10), (990, 520, 2420, 1, 1000, 2900, 5), (980, 521, 2420, 2, 1000, 2899, 5),
                                         (970, 522, 2420, 3, 1000, 2898, 5), (960, 523, 2420, 4, 1000, 2897, 5)],
     dict(score=[1000, 990, 980], parent=[0, 0, 0], subsc=[990, 0, 0], n_sub=[0, 0, 0], sam_pri=[1, 0, 0]), dict(kept_2nd=2, drop_best_n=2, resynced=1)),
)


def hand_family(seed=606):
    rng = np.random.default_rng(seed)
    return [Batch('hand-' + name, [hand_read(name, qlen, hits, rng)], **opt) for name, opt, qlen, hits, _, _ in HAND]


def families():
    return dict(counts=counts_family(), ties=ties_family(), mask=mask_family(), select=select_family(), join=join_family(), hand=hand_family())


# ---- the host check program (scripts/hit_host_check.cpp: csrc/hit_host.cpp + csrc/hits_block.cpp built for the host) ----------------
BLOCK_FIELDS = ('cnt', 'rid', 'score', 'score0', 'qs', 'qe', 'rs', 're', 'mlen', 'blen', 'rev', 'inv', 'split', 'hash', 'has_p', 'dp_score',
                'dp_max', 'n_ambi')


def build_host_check(out_dir):
    exe = os.path.join(str(out_dir), 'hit_host_check')
    csrc = os.path.join(ROOT, 'megapath_nano_amd', 'csrc')
    base = ['g++', '-std=c++17', '-Wall', '-Werror', '-o', exe, os.path.join(ROOT, 'scripts', 'hit_host_check.cpp'),
            os.path.join(csrc, 'hit_host.cpp'), os.path.join(csrc, 'hits_block.cpp')]
    if subprocess.run(base + ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']).returncode != 0:
        subprocess.run(base + ['-O2'], check=True)
    return exe


def host_hits(exe, tmp, runs):
    """runs: [(batch, the bytes of its mpn_map_opt)] -> per run, per read (hits as dicts of hit_ref.KEYS, n_a, segments (src, dst, cnt,
    flag) or None without CIGARs): the host hit path on the chains in pool order"""
    from hit_ref import KEYS
    out = [struct.pack('<I', len(runs))]
    for b, opt in runs:
        out.append(struct.pack('<I', len(opt)) + opt + struct.pack('<iI', b.k, len(b.reads)))
        for r in b.reads:
            name = r.name.encode()
            out.append(struct.pack('<i', len(name)) + name + struct.pack('<iI', r.qlen, len(r.pool)))
            for c in r.pool:
                out.append(struct.pack('<5Q2i', c.score << 32 | len(c.a), c.a[0][0], c.a[0][1], c.a[-1][0], c.a[-1][1], c.mlen, c.blen))
    src, dst = os.path.join(str(tmp), 'hit_cases.bin'), os.path.join(str(tmp), 'hit_results.bin')
    with open(src, 'wb') as f:
        f.write(b''.join(out))
    subprocess.run([exe, 'hits', src, dst], check=True, timeout=600)
    blob, p, res = open(dst, 'rb').read(), 0, []
    unsigned = ('fx', 'fy', 'lx', 'ly', 'hash')
    for b, opt in runs:
        reads = []
        for _ in b.reads:
            n_regs, n_a, n_segs = struct.unpack_from('<3i', blob, p)
            p += 12
            hits = []
            for _ in range(n_regs):
                w = struct.unpack_from('<15q', blob, p)
                p += 120
                hits.append({key: v & (1 << 64) - 1 if key in unsigned else v for key, v in zip(KEYS, w)})
            segs = [struct.unpack_from('<q3i', blob, p + 20 * t) for t in range(n_segs)]
            p += 20 * n_segs
            reads.append((hits, n_a, segs))
        res.append(reads)
    assert p == len(blob)
    return res


def squeezed(read, n_a, segs):
    """the read's squeezed anchor list as anchor_squeeze_kernel writes it from the segments: every place written exactly once"""
    pool = [p for c in read.pool for p in c.a]
    sq = [None] * n_a
    for src, dst, cnt, flag in segs:
        assert cnt >= 1 and 0 <= src and src + cnt <= len(pool) and 0 <= dst and dst + cnt <= n_a and flag in (0, 1), (read.name, src, dst, cnt, flag)
        for j in range(cnt):
            assert sq[dst + j] is None, (read.name, 'place written twice', dst + j)
            x, y = pool[src + j]
            sq[dst + j] = (x, y | 1 << 40) if j == 0 and flag else (x, y)
    assert None not in sq, (read.name, 'place not written')
    return sq


def host_block(exe, tmp, k, want_text, n_parts, lens, reads, lo, hi):
    """reads: [(rep_len, [(the BLOCK_FIELDS values, CIGAR words)])] -> (block bytes, the fresh accumulator after two imports of reads
    [lo, hi) as (k, n_parts, lens, the reads in the same form), the five counts of the refusal loops)"""
    out = [struct.pack('<4i', k, want_text, n_parts, len(lens)) + struct.pack('<%di' % len(lens), *lens) + struct.pack('<i', len(reads))]
    for rep_len, hits in reads:
        out.append(struct.pack('<2i', rep_len, len(hits)))
        for f, cig in hits:
            out.append(struct.pack('<18i', *f) + struct.pack('<i%dI' % len(cig), len(cig), *cig))
    out.append(struct.pack('<2i', lo, hi))
    src, dst = os.path.join(str(tmp), 'block_cases.bin'), os.path.join(str(tmp), 'block_results.bin')
    with open(src, 'wb') as f:
        f.write(b''.join(out))
    subprocess.run([exe, 'block', src, dst], check=True, timeout=600)
    blob = open(dst, 'rb').read()
    size, k2, parts2, n_seq2 = struct.unpack_from('<q3i', blob, 0)
    p = 20
    lens2 = list(struct.unpack_from('<%di' % n_seq2, blob, p))
    p += 4 * n_seq2
    got = []
    for _ in range(hi - lo):
        rep_len, n_hits = struct.unpack_from('<2i', blob, p)
        p += 8
        hits = []
        for _ in range(n_hits):
            f = struct.unpack_from('<18i', blob, p)
            nc, = struct.unpack_from('<i', blob, p + 72)
            hits.append((f, struct.unpack_from('<%dI' % nc, blob, p + 76)))
            p += 76 + 4 * nc
        got.append((rep_len, hits))
    counts = struct.unpack_from('<5q', blob, p)
    assert p + 40 == len(blob)
    return size, (k2, parts2, lens2, got), counts
