"""Hand-built hits, windows and window results for the tests of the stitching stage (test_stitch_ref.py on the CPU,
test_ext_stitch_gpu.py on the GPU).  No genome, no DP: a case is one read's squeezed anchor list with one hit in it; the hit's
windows (where they start, which anchor a fill ends at, the stitching record) are what plan_ref.py plans for those anchors, so
that the oracle, which plans the hit again by itself, reaches the same windows; what the DP left in every window -- scores,
maxima, end flags, z-drops, CIGARs -- is invented.  A small min_ksw_len makes a gap fill of every anchor, a small max_sw_mat
refuses the windows that are made large.

families() -> {name: [Batch]}; a batch is one call of the stage (one min_cnt).  The windows' places in the compact pool and the
hits' places in the window array are shuffled per batch."""
import random

import numpy as np

from plan_cases import K, TLEN, Read, hit, word
from plan_ref import EZ_EXTZ_ONLY, EZ_REFUSED, plan_ref
from stitch_ref import EZ_INV, stitch_hit

KH = K >> 1
M, I, D = 0, 1, 2
NEG = -(1 << 20)          # a score that was never reached (ksw's NEG_INF, within the entry's range)
# what the result record of a placeholder holds: nothing may look at it.  (In range, so that a kernel that did would give wrong
# numbers, not wrong addresses.)
JUNK = dict(max=999, zdropped=0, max_q=55, max_t=66, mqe_t=77, score=888, reach_end=1, ops=[(M, 9), (I, 1)])


def chain(n, t0=3000, q0=900, d=20, steps=None, span=K, spans=None, flags=None, rid=0, rev=0):
    """n anchors from (t0, q0), d bases apart on both sequences; steps {i: (dt, dq)}: the step into anchor i"""
    steps, spans, flags = steps or {}, spans or {}, flags or {}
    out, t, q = [], t0, q0
    for i in range(n):
        if i:
            dt, dq = steps.get(i, (d, d))
            t, q = t + dt, q + dq
        out.append(word(rid, rev, t, q, spans.get(i, span), flags.get(i, 0)))
    return out


def no_left(n, **kw):
    """a hit whose first k-mer's centre is the first base of the read: no left extension; n anchors give n windows"""
    return chain(n, q0=KH, span=KH + 1, **kw)


def with_left(n, **kw):
    """the anchors of a hit of n windows with both extensions, every anchor but the first ending a fill"""
    return chain(n - 1, **kw)


def default_res(k, w):
    """a result no rule treats specially: two ops that merge with nothing (M first, a gap last), score != max, a maximum behind the
    first anchor of the window (the anchor search ends at once where a fill starts at the anchor before its last)"""
    ops = [(M, 5 + k % 7), (I if k % 2 else D, 1 + k % 3)]
    if w['flag'] & EZ_EXTZ_ONLY:
        return dict(max=40 + k % 11, zdropped=0, max_q=12, max_t=14, mqe_t=17, score=NEG, reach_end=0, ops=ops)
    return dict(max=30 + k % 13, zdropped=0, max_q=8, max_t=9, mqe_t=-1, score=20 + k % 5, reach_end=0, ops=ops)


class Case:
    def __init__(self, name, anchors, res=None, ops=None, inv=(), min_cnt=3, lead=0, trail=0, mlen=None, split_inv=0, qlen=None, rid=0,
                 rev=0, drop_right=False, move=None, default=default_res, **opt):
        """anchors: the hit; lead / trail: that many anchors of another target before / behind it in the read's list.
        res {window: dict of result fields to change}, ops {window: [(kind, length)]}, inv: fills the z-drop test marked as inversions.
        Windows are counted from the hit's first (negative: from its last).  opt: planning options (min_ksw_len, max_sw_mat).
        drop_right: the right extension is taken away; move {window: (dq, dt)}: a window starts elsewhere than planned.  Either makes a
        hit the oracle would plan otherwise: it is the restatement's alone."""
        self.name, self.min_cnt, self.k = name, min_cnt, K
        before = chain(lead, t0=100, q0=100, rid=rid + 1, rev=rev)
        behind = chain(trail, t0=100, q0=40000, rid=rid + 1, rev=rev)
        kw = dict(split_inv=split_inv)
        if mlen is not None:
            kw['mlen'] = mlen
        self.read = Read(name, [before, hit(anchors, **kw), behind], qlen=qlen)
        self.opt = dict(min_ksw_len=10, min_cnt=min_cnt)
        self.opt.update(opt)
        self.tlens = [TLEN, TLEN, TLEN]
        self.as_, self.cnt, self.mlen, self.split_inv = self.read.hits[0]
        hits, left, evs = plan_ref(self.k, self.tlens, self.read.qlen, self.read.anchors, self.read.hits, **self.opt)
        self.hit, self.anchors_planned, self.plan_ev = dict(hits[0]), left, evs[0]
        self.hit.update({'as': self.as_, 'cnt': self.cnt})
        wins = [dict(w) for w in self.hit.pop('windows')]
        self.oracle = not drop_right and not move
        if drop_right:
            assert wins[-1]['kind'] == 'right'
            wins.pop()
        for k, (dq, dt) in (move or {}).items():
            wins[k]['qs'] += dq
            wins[k]['ts'] += dt
        n = len(wins)
        assert all(-n <= k < n for k in list(res or {}) + list(inv)), (name, n)
        res = {(k + n) % n: v for k, v in (res or {}).items()}
        ops = {(k + n) % n: v for k, v in (ops or {}).items() if -n <= k < n}      # (a table of ops may be longer than the hit)
        inv = {(k + n) % n for k in inv}
        for k, w in enumerate(wins):
            r = dict(JUNK) if w['flag'] & EZ_REFUSED else default(k, w)
            r.update(res.get(k, {}))
            if k in ops:
                r['ops'] = list(ops[k])
            if k in inv:
                assert w['kind'] == 'fill'
                w['flag'] |= EZ_INV
            w['res'] = r
        self.wins = wins
        self.hit['n_jobs'] = n

    def ref(self, read=0):
        return stitch_hit(self.anchors_planned, self.hit, self.wins, self.min_cnt, read=read)


class Batch:
    def __init__(self, name, cases, seed=1):
        assert len({c.min_cnt for c in cases}) == 1
        self.name, self.cases, self.min_cnt, self.seed = name, cases, cases[0].min_cnt, seed

    def arrays(self):
        """the batch as mapper.stitch_batch takes it: every case a read with one hit"""
        rng = random.Random(self.seed)
        a_off = np.cumsum([0] + [len(c.anchors_planned) for c in self.cases]).astype(np.int64)
        anchors = np.array([p for c in self.cases for p in c.anchors_planned], dtype=np.uint64).reshape(-1, 2)
        order = list(range(len(self.cases)))
        rng.shuffle(order)                       # the hits' window groups, in any order
        first, at = {}, 0
        for ci in order:
            first[ci] = at
            at += len(self.cases[ci].wins)
        n_win = at
        hits = np.zeros((len(self.cases), 15), dtype=np.int32)
        wins = np.zeros((n_win, 13), dtype=np.int32)
        ops_of = [None] * n_win
        for ci, c in enumerate(self.cases):
            h = c.hit
            hits[ci] = [ci, h['rid'], h['rev'], h['as'], h['cnt'], h['as1'], h['cnt1'], h['qs'], h['rs'], h['qe'], h['re'], h['qs0'], h['qe0'],
                        first[ci], len(c.wins)]
            for k, w in enumerate(c.wins):
                r = w['res']
                wins[first[ci] + k] = [w['flag'], w['reversed'], w['qs'], w['ts'], w['anchor'], r['max'], r['zdropped'], r['max_q'], r['max_t'],
                                       r['mqe_t'], r['score'], r['reach_end'], len(r['ops'])]
                ops_of[first[ci] + k] = [length << 4 | kind for kind, length in r['ops']]
        place = list(range(n_win))
        rng.shuffle(place)                       # the windows' ops, anywhere in the pool, with unused words between them
        cig_pos = np.zeros(n_win, dtype=np.int64)
        pool = []
        for wi in place:
            pool.extend([0xfffffff3] * rng.randrange(3))       # (not an operation: never read)
            cig_pos[wi] = len(pool)
            pool.extend(ops_of[wi])
        return dict(anchor_off=a_off, anchors=anchors, hits=hits, wins=wins, cig_pos=cig_pos, compact=np.array(pool, dtype=np.uint32),
                    min_cnt=self.min_cnt)


def fill_at(c_left, i):
    """the window index of fill i (counted from 0) of a hit with / without a left extension"""
    return i + (1 if c_left else 0)


# ---- sizes: 1 .. 200 windows, with and without either extension, no merges ---------------------------------------------------------
def sizes_family():
    cases = []
    for n in (1, 2, 63, 64, 65, 128, 129, 200):
        if n > 1:
            cases.append(Case('n%d-left' % n, chain(n - 1)))
        cases.append(Case('n%d-noleft' % n, no_left(n)))
    for n in (1, 2, 64, 65):     # no right extension: a hit the oracle never plans (every planned hit has one); the restatement's alone
        if n > 1:
            cases.append(Case('n%d-left-noright' % n, chain(n), drop_right=True))
        cases.append(Case('n%d-noleft-noright' % n, no_left(n + 1), drop_right=True))
    cases.append(Case('n5-lead-trail', chain(4), lead=7, trail=3))
    cases.append(Case('n5-rev-rid1', chain(4, rid=1, rev=1), rid=1, rev=1, lead=2))
    return [Batch('sizes', cases)]


# ---- merge: mm_append_cigar's rule as a scan over windows, across passes of 64, several adds on one word ----------------------------
def runs(n, at, r, kind=I):
    """ops of n windows: window `at` ends in `kind`, the r windows behind it are one op of that kind each, the next starts with it"""
    ops = {at: [(M, 5), (kind, 2)], at + r + 1: [(kind, 3), (M, 4), (3 - kind, 1)]}
    for k in range(at + 1, at + r + 1):
        ops[k] = [(kind, 1 + k % 4)]
    return ops


def merge_family():
    cases = []
    n = 131
    cases.append(Case('every-join', with_left(n), ops={k: [(M, 3 + k % 5), (I if k % 3 else D, 1 + k % 2), (M, 2 + k % 7)] for k in range(n)}))
    cases.append(Case('every-join-noleft', no_left(n), ops={k: [(D, 3 + k % 5), (M, 1 + k % 2), (D, 2 + k % 7)] for k in range(n)}))
    # only the joins between two passes merge
    ops = {63: [(M, 4), (D, 2)], 64: [(D, 5), (M, 1), (I, 2)], 127: [(M, 4), (I, 2)], 128: [(I, 5), (M, 1), (D, 2)]}
    cases.append(Case('pass-joins', with_left(n), ops=ops))
    for r, at in ((2, 10), (3, 10), (2, 62), (3, 61), (3, 62), (3, 63), (70, 5), (70, 58), (2, 126)):
        cases.append(Case('run%d-at%d' % (r, at), with_left(n), ops=runs(n, at, r, kind=I if at % 2 else D)))
    # a run of single M windows from the first window of the hit on
    cases.append(Case('run-from-0', chain(20), ops={k: [(M, 1 + k)] for k in range(8)}))
    # equal kinds at the even joins, unequal ones at the odd joins
    ops = {}
    for k in range(n):
        ops[k] = [(M, 2 + k % 3), (D, 1), (I, 1 + k % 5)] if k % 2 == 0 else [(I, 2 + k % 3), (M, 1), (D, 1 + k % 5)]
    cases.append(Case('alternate', with_left(n), ops=ops))
    return [Batch('merge', cases)]


# ---- empty: windows without operations wherever a merge has to look past them ------------------------------------------------------
def empty_family():
    cases = []
    n = 140
    e = []
    # before, between and behind mergeable windows
    ops = {0: e, 1: e, 2: [(M, 5), (I, 1), (M, 2)], 3: e, 4: e, 5: [(M, 3), (D, 2)], 6: e, 7: [(D, 1)], 8: e, 9: [(D, 2), (M, 9)], 10: e}
    cases.append(Case('around', chain(30), ops=ops))
    # lane 0 of the second and third pass empty; the join reaches over it
    ops = {63: [(M, 4), (I, 2)], 64: e, 65: [(I, 5), (M, 1), (D, 1)], 127: [(M, 4), (D, 2)], 128: e, 129: [(D, 5)], 130: [(D, 1), (M, 1), (I, 1)]}
    cases.append(Case('lane0', with_left(n), ops=ops))
    # a whole pass of empty windows between two that merge; the same from lane 63 to lane 0 two passes on; and to the last window
    for a, b in ((60, 131), (63, 128), (0, 139), (10, 75)):
        ops = {k: e for k in range(a + 1, b)}
        ops[a], ops[b] = [(M, 7), (D, 3)], [(D, 2), (M, 6), (I, 1)]
        cases.append(Case('gap-%d-%d' % (a, b), with_left(n), ops=ops))
    # nothing at all: n_ops 0, has_p 0 (the extensions have maxima: not counted)
    for n2 in (1, 2, 65, 130):
        anchors = chain(n2 - 1) if n2 > 1 else no_left(1)
        cases.append(Case('all-empty-%d' % n2, anchors, default=lambda k, w: dict(default_res(k, w), ops=[])))
    # an extension with a maximum but no operations: its score is not counted, its coordinates are
    cases.append(Case('ext-max-no-ops', chain(5), ops={0: e, -1: e}, res={0: dict(max=77), -1: dict(max=88)}))
    cases.append(Case('left-max-no-ops', chain(5), ops={0: e}, res={0: dict(max=77, reach_end=1)}))
    return [Batch('empty', cases)]


# ---- cut: the first z-dropped gap fill ends the hit -------------------------------------------------------------------------------
def dropped(max_=33, max_t=9, max_q=8):
    return dict(zdropped=1, max=max_, score=NEG, max_t=max_t, max_q=max_q)


def cut_family():
    cases = []
    n = 140
    # every window behind the cut would change the numbers if it were counted: all joins merge, the right extension reaches its end
    ops = {k: [(M, 3 + k % 5), (I if k % 3 else D, 1 + k % 2), (M, 2 + k % 7)] for k in range(n)}
    right = {-1: dict(reach_end=1, mqe_t=150, max=500)}
    cases.append(Case('first-fill-noleft', no_left(n), res={**right, 0: dropped()}, ops=ops))
    for at in (1, 2, 62, 63, 64, 65, 127, 128, n - 2):
        cases.append(Case('at-%d' % at, with_left(n), res={**right, at: dropped()}, ops=ops))
        cases.append(Case('at-%d-plain' % at, with_left(n), res={**right, at: dropped()}))
    cases.append(Case('at-63-noleft', no_left(n), res={**right, 63: dropped()}, ops=ops))
    cases.append(Case('at-64-noleft', no_left(n), res={**right, 64: dropped()}, ops=ops))
    for name, a, b in (('one-pass', 10, 20), ('two-passes', 30, 100), ('63-64', 63, 64), ('64-65', 64, 65), ('1-130', 1, 130), ('70-71-third', 70, 71)):
        cases.append(Case('two-' + name, with_left(n), res={**right, a: dropped(33, 9, 8), b: dropped(44, 10, 11)}, ops=ops))
    cases.append(Case('three', with_left(n), res={**right, 66: dropped(), 67: dropped(1, 0, 0), 130: dropped()}, ops=ops))
    # a z-drop flag on an end extension cuts nothing
    cases.append(Case('left-zdropped', with_left(n), res={0: dict(zdropped=1)}, ops=ops))
    cases.append(Case('right-zdropped', with_left(n), res={-1: dict(zdropped=1)}, ops=ops))
    cases.append(Case('both-zdropped-then-fill', with_left(n), res={0: dict(zdropped=1), -1: dict(zdropped=1), 70: dropped()}, ops=ops))
    cases.append(Case('right-zdropped-short', chain(1), res={-1: dict(zdropped=1)}))
    cases.append(Case('right-zdropped-noleft-64', no_left(64), res={-1: dict(zdropped=1)}, ops=ops))
    # the dropped fill counts its maximum (its score was never reached), with and without operations of its own
    cases.append(Case('max-not-score', chain(10), res={4: dropped(max_=57)}))
    cases.append(Case('max-not-score-empty', chain(10), res={4: dropped(max_=57)}, ops={4: []}))
    cases.append(Case('max-0', chain(10), res={4: dropped(max_=0, max_t=-1, max_q=-1)}, ops={4: []}))
    return [Batch('cut', cases)]


# ---- refused: placeholders of windows that got no DP, in each of the three positions ------------------------------------------------
def refused_family():
    cases = []
    big = {4: (400, 400)}            # the fill into anchor 4 is 400 x 400
    # left extension 893 x 1784, right 308 x 614, fills 20 x 20
    cases.append(Case('left', chain(8), max_sw_mat=1000000))
    cases.append(Case('left-merge-over', chain(8), max_sw_mat=1000000, ops={1: [(M, 9), (D, 1)]}))
    # left 50 x 98, right 308 x 614
    cases.append(Case('right', chain(8, q0=57), max_sw_mat=100000))
    cases.append(Case('both', chain(8), max_sw_mat=100000))
    # left 50 x 98, right 57 x 112, one fill 400 x 400
    small = dict(q0=57, steps=big)
    qlen = 57 + 6 * 20 + 400 + 50
    cases.append(Case('fill', chain(8, **small), qlen=qlen, max_sw_mat=100000))
    cases.append(Case('fill-min-cnt-1', chain(8, **small), qlen=qlen, max_sw_mat=100000, min_cnt=1))
    cases.append(Case('fill-noleft', no_left(8, steps=big), qlen=KH + 6 * 20 + 400 + 50, max_sw_mat=100000))
    cases.append(Case('fill-first', chain(8, q0=57, steps={1: (400, 400)}), qlen=qlen, max_sw_mat=100000))
    # a cut before the point the left extension reached: no planned window starts there (a fill starts at an anchor of the hit, the
    # left extension ends at the first); the spans of the finishing job are clamped at 0
    cases.append(Case('fill-first-moved', chain(8, q0=57, steps={1: (400, 400)}), qlen=qlen, max_sw_mat=100000, move={1: (-14, -16)}))
    cases.append(Case('drop-moved', chain(8, q0=57), res={1: dropped(max_t=3, max_q=2)}, move={1: (-30, -30)}))
    cases.append(Case('fill-last', chain(8, q0=57, steps={7: (400, 400)}), qlen=qlen, max_sw_mat=100000))
    # a refused fill behind a dropped one, and before one: the first of the two ends the hit
    cases.append(Case('fill-after-drop', chain(8, **small), qlen=qlen, max_sw_mat=100000, res={2: dropped()}))
    cases.append(Case('fill-before-drop', chain(8, **small), qlen=qlen, max_sw_mat=100000, res={6: dropped()}))
    two = dict(q0=57, steps={4: (400, 400), 6: (400, 400)})
    cases.append(Case('two-fills', chain(8, **two), qlen=qlen + 400, max_sw_mat=100000))
    # everything refused
    cases.append(Case('all', chain(2, steps={1: (400, 400)}), max_sw_mat=1000))
    # a long hit: a refused fill at lane 0 of the second pass, merges up to it
    n = 100
    ops = {k: [(M, 3), (I, 1), (M, 2)] for k in range(n)}
    cases.append(Case('fill-at-64', with_left(n, q0=57, steps={64: (400, 400)}), qlen=57 + 97 * 20 + 400 + 50, max_sw_mat=100000, ops=ops))
    return [Batch('refused', [c for c in cases if c.min_cnt == 3]), Batch('refused-min-cnt-1', [c for c in cases if c.min_cnt == 1])]


# ---- ends: the two coordinate rules of either extension ----------------------------------------------------------------------------
def ends_family():
    cases = []
    for lr in (0, 1):
        for rr in (0, 1):
            res = {0: dict(reach_end=lr, max_t=21, max_q=19, mqe_t=40), -1: dict(reach_end=rr, max_t=23, max_q=18, mqe_t=45)}
            cases.append(Case('reach-%d-%d' % (lr, rr), chain(6), res=res))
            cases.append(Case('reach-%d-%d-rev' % (lr, rr), chain(6, rev=1, rid=2), res=res, rid=2, rev=1))
    cases.append(Case('right-only-reach', no_left(1), res={0: dict(reach_end=1, max_t=3, max_q=2, mqe_t=30)}))
    cases.append(Case('nothing-reached', chain(3), res={0: dict(max_t=-1, max_q=-1, max=0), -1: dict(max_t=-1, max_q=-1, max=0)}, ops={0: [], -1: []}))
    return [Batch('ends', cases)]


# ---- split: the anchor a cut hit is split at, the min_cnt bar, the measures of the two halves ---------------------------------------
def split_family():
    cases = []
    # fills over five anchors each (min_ksw_len 100, anchors 20 apart): fill f is window f + 1, from anchor 5 f to anchor 5 f + 5
    # whose x are ts + 7, 27, 47, 67, 87 (, 107)
    long_ = dict(min_ksw_len=100)
    for name, f, max_t in (('at-once', 3, 95), ('one-step', 3, 70), ('three-steps', 3, 30), ('four-steps', 3, 7), ('before-window', 3, 6),
                           ('before-window-1', 3, -1), ('fall-through', 0, 6), ('fall-through-1', 0, -1), ('first-anchor', 0, 7)):
        cases.append(Case('search-' + name, chain(41), res={f + 1: dropped(max_t=max_t)}, **long_))
        cases.append(Case('search-%s-lead' % name, chain(41), res={f + 1: dropped(max_t=max_t)}, lead=9, trail=4, **long_))
    cases.append(Case('search-fall-through-noleft', no_left(41), res={0: dropped(max_t=2)}, **long_))
    # the bar: every anchor a fill (fill f ends at anchor f + 1 and is window f + 1); the search ends at once: j + 1 = f + 1
    n = 12
    for min_cnt in (3, 1, 0):
        for left in (n - min_cnt, n - min_cnt - 1, n - min_cnt + 1):       # anchors that stay: cnt1 - left = min_cnt, one more, one fewer
            if 1 <= left <= n - 1:
                cases.append(Case('bar-%d-stay-%d' % (min_cnt, left), chain(n), res={left: dropped()}, min_cnt=min_cnt, inv=(left,)))
    # the shortest remainders there are: the last fill (split_n = cnt - 1), the first (split_n = 1)
    for min_cnt in (1, 0):
        cases.append(Case('last-fill-%d' % min_cnt, chain(n), res={n - 1: dropped()}, min_cnt=min_cnt))
        cases.append(Case('first-fill-%d' % min_cnt, chain(n), res={1: dropped()}, min_cnt=min_cnt))
        cases.append(Case('two-anchors-%d' % min_cnt, no_left(2), res={0: dropped()}, min_cnt=min_cnt))
        cases.append(Case('two-anchors-left-%d' % min_cnt, chain(2), res={1: dropped(max_t=0)}, min_cnt=min_cnt))
    cases.append(Case('first-fill-3', chain(n), res={1: dropped()}))
    # a hit trimmed at the front (as1 > as), at the back, at both: the split counts from as, the search from as1
    steps = {1: (20, 50)}
    cases.append(Case('trim-front', chain(40, steps=steps), res={20: dropped()}))
    cases.append(Case('trim-front-lead', chain(40, steps=steps), res={20: dropped(max_t=0)}, lead=5))
    cases.append(Case('trim-front-first', chain(40, steps=steps), res={1: dropped(max_t=0)}))
    cases.append(Case('trim-back', chain(40, steps={39: (50, 20)}), res={36: dropped()}))
    cases.append(Case('trim-back-bar', chain(40, steps={39: (50, 20)}), res={37: dropped()}))
    cases.append(Case('trim-both', chain(40, steps={1: (20, 50), 39: (50, 20)}), res={35: dropped()}, lead=3))
    # the inversion mark: on the dropped fill (with and without a remainder), on a fill that did not drop, on one behind the cut
    cases.append(Case('inv', chain(20), res={8: dropped()}, inv=(8,)))
    cases.append(Case('inv-no-remainder', chain(20), res={18: dropped()}, inv=(18,)))
    cases.append(Case('inv-elsewhere', chain(20), res={8: dropped()}, inv=(3, 12)))
    cases.append(Case('inv-not-dropped', chain(20), inv=(3, 12)))
    # mm_split_reg's sums: every branch of the mlen rule on either side of the cut, over 2, 64, 65 and 200 anchors
    for cnt in (2, 64, 65, 200):
        steps = {}
        for i in range(3, cnt - 3):
            steps[i] = ((20, 20), (10, 12), (12, 10), (20, 23), (23, 20), (15, 15), (16, 16), (14, 30))[i % 8]
        spans = {i: 11 + i % 5 for i in range(cnt)}
        for cut in sorted({1, cnt // 2, cnt - 2, cnt - 1}):
            if 1 <= cut <= cnt - 1:
                cases.append(Case('sums-%d-cut-%d' % (cnt, cut), chain(cnt, steps=steps, spans=spans), res={cut: dropped(max_t=40)}, min_cnt=1,
                                  lead=cnt % 3))
    batches = []
    for min_cnt in (3, 1, 0):
        batches.append(Batch('split-min-cnt-%d' % min_cnt, [c for c in cases if c.min_cnt == min_cnt]))
    return batches


FAMILY_MAKERS = dict(sizes=sizes_family, merge=merge_family, empty=empty_family, cut=cut_family, refused=refused_family, ends=ends_family,
                     split=split_family)
FAMILIES = tuple(sorted(FAMILY_MAKERS)) + ('batch',)
_cache = {}


def families():
    """{family: [Batch]}, built once"""
    if not _cache:
        for name, make in FAMILY_MAKERS.items():
            _cache[name] = make()
        # every hit above in one call per min_cnt
        every = [c for name in sorted(FAMILY_MAKERS) for b in _cache[name] for c in b.cases]
        _cache['batch'] = [Batch('all-min-cnt-%d' % m, [c for c in every if c.min_cnt == m], seed=7 + m) for m in (3, 1, 0)]
    return _cache


def many_hits(n=8300):
    """n hits of two windows each (more than the blocks of the mapper's grid: its stride loop), from a few templates -> (Batch, template
    index per hit, the templates)"""
    t = [Case('two-left', chain(1), min_cnt=1), Case('two-noleft', no_left(2), min_cnt=1),
         Case('two-noleft-cut', no_left(2), res={0: dropped()}, min_cnt=1, ops={0: [(M, 5)], 1: [(M, 3)]}),
         Case('two-merge', chain(1), min_cnt=1, ops={0: [(M, 5), (I, 2)], 1: [(I, 3)]}),
         Case('two-noleft-cut-inv', no_left(2), res={0: dropped(max_t=0)}, min_cnt=1, inv=(0,))]
    idx = [(i * 7 + i // 5) % len(t) for i in range(n)]
    return Batch('many', [t[i] for i in idx], seed=3), idx, t

