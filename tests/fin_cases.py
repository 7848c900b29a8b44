"""Seeded alignments for the tests of the finishing kernel (test_fin_ref.py on the CPU, test_aln_finish_gpu.py on the GPU).

Every alignment is made by construction: a target, a CIGAR, and the read that walking the CIGAR over the target gives (a few
substitutions in match columns; inserted bases mostly continue the local repeat, which is what lets a gap slide).  Nothing here
is aligned by a DP, so the CIGARs are as awkward as wanted: empty ops, adjacent insertion / deletion runs, gaps first or last."""
import numpy as np

from diff_tags_ref import revcomp_codes
from fin_ref import D, I, M, op

PERIODS = (1, 2, 3, 5, 17)
N_OPS = (2, 3, 63, 64, 65, 127, 128, 129, 512, 513)    # where ceil(n / 64) and the 512-op staging loop change
SEEDS = (0, 1, 2)
LDS_CLASSES = (16384, 32768, 65536)


class Aln:
    """One alignment: q (codes, alignment orientation) against t under cigar; placed in a read with flanks (read orientation:
    for rev the reverse complement of q sits between them) and in a target with flanks.  tl / tr may be code arrays."""

    def __init__(self, name, cigar, q, t, rev=0, ql=0, qr=0, tl=0, tr=0, rng=None, period=0):
        rng = rng or np.random.default_rng(len(q) * 7 + len(t))
        self.name, self.cigar, self.rev, self.period = name, [int(c) for c in cigar], rev, period
        self.q, self.t = np.asarray(q, dtype=np.uint8), np.asarray(t, dtype=np.uint8)
        assert sum(c >> 4 for c in self.cigar if c & 15 != D) == len(self.q) and sum(c >> 4 for c in self.cigar if c & 15 != I) == len(self.t), name
        flank = lambda f: rng.integers(0, 4, f) if isinstance(f, (int, np.integer)) else np.asarray(f)  # noqa: E731
        mid = revcomp_codes(self.q) if rev else self.q
        left, right = flank(ql), flank(qr)
        self.read = np.concatenate([left, mid, right]).astype(np.uint8)
        self.qs, self.qe = len(left), len(left) + len(self.q)
        left, right = flank(tl), flank(tr)
        self.target = np.concatenate([left, self.t, right]).astype(np.uint8)
        self.ts = len(left)

    @property
    def need(self):
        """bytes of LDS the launch code asks for: CIGAR + shift table, both code arrays padded to words, 16"""
        return len(self.cigar) * 8 + ((len(self.q) + 3) & ~3) + ((len(self.t) + 3) & ~3) + 16


def spans(cigar):
    return sum(c >> 4 for c in cigar if c & 15 != D), sum(c >> 4 for c in cigar if c & 15 != I)


def repeat_target(rng, period, length, noise=0.05):
    """a tandem repeat of one random unit, `noise` of its bases randomised"""
    unit = rng.integers(0, 4, period)
    while period > 1 and len(set(unit.tolist())) == 1:
        unit = rng.integers(0, 4, period)
    t = np.resize(unit, length).astype(np.uint8)
    hit = rng.random(length) < noise
    t[hit] = rng.integers(0, 4, int(hit.sum()))
    return t


def walk(rng, cigar, t, period=1, sub=0.02, cont=0.85):
    """the read that `cigar` derives from t: match columns copy t but for a share `sub` of substitutions, an inserted base repeats
    the read `period` bases back with probability `cont`"""
    q, ti = [], 0
    for c in cigar:
        ln, o = c >> 4, c & 15
        for _ in range(ln):
            if o == M:
                q.append((int(t[ti]) + 1 + int(rng.integers(0, 3))) % 4 if t[ti] < 4 and rng.random() < sub else int(t[ti]))
                ti += 1
            elif o == I:
                q.append(q[-period] if len(q) >= period and rng.random() < cont else int(rng.integers(0, 4)))
            else:
                ti += 1
    assert ti == len(t)
    return np.array(q, dtype=np.uint8)


def alt_cigar(rng, n_ops, m_max=11, g_max=5, p_pair=0.08, p_zero=0.04):
    """n_ops ops: match runs of 0..m_max (a few empty) alternating with gaps of 1..g_max (a few empty), now and then two or three
    gaps of alternating kind in a row"""
    cig = []
    while len(cig) < n_ops:
        cig.append(op(0 if rng.random() < p_zero else int(rng.integers(1, m_max + 1)), M))
        g = int(rng.integers(1, 3))
        for _ in range(1 + (rng.random() < p_pair) + (rng.random() < p_pair / 2)):
            cig.append(op(0 if rng.random() < p_zero else int(rng.integers(1, g_max + 1)), g))
            g = 3 - g
    return cig[:n_ops]


def on_repeat(rng, name, cigar, period, **kw):
    t = repeat_target(rng, period, spans(cigar)[1])
    return Aln(name, cigar, walk(rng, cigar, t, period), t, rng=rng, period=period, **kw)


def on_random(rng, name, cigar, sub=0.02, **kw):
    t = rng.integers(0, 4, spans(cigar)[1]).astype(np.uint8)
    return Aln(name, cigar, walk(rng, cigar, t, 1, sub, 0.0), t, rng=rng, **kw)


def repeat_family(period):
    out = []
    for n in N_OPS:
        for seed in SEEDS:
            rng = np.random.default_rng([period, n, seed])
            out.append(on_repeat(rng, 'p%d-n%d-s%d' % (period, n, seed), alt_cigar(rng, n), period, rev=(seed + n) & 1,
                                 ql=int(rng.integers(0, 7)), qr=int(rng.integers(0, 7)), tl=int(rng.integers(0, 40)), tr=int(rng.integers(0, 40))))
    return out


def homopolymer(name, cigar, q_mut=(), period=1, **kw):
    """exact repeat of period 1 (AAAA..) or 2 (ACAC..) under cigar; inserted bases continue it; q_mut: (index, code) in the read"""
    qn, tn = spans(cigar)
    t = np.resize(np.arange(period), tn).astype(np.uint8)
    q, ti = [], 0
    for c in cigar:
        ln, o = c >> 4, c & 15
        for _ in range(ln):
            if o != D:
                q.append(ti % period if o == M else (q[-period] if len(q) >= period else len(q) % period))
            ti += o != I
    q = np.array(q, dtype=np.uint8).reshape(-1)
    for i, c in q_mut:
        q[i] = c
    return Aln(name, cigar, q, t, period=period, **kw)


def leading_gap_cases():
    rng = np.random.default_rng(101)
    out = []
    for k in (1, 3):
        for rev in (0, 1):
            out.append(homopolymer('lead-1M%dI' % k, [op(1, M), op(k, I), op(9, M)], rev=rev, ql=3, qr=2, tl=5, tr=1))
            out.append(homopolymer('lead-2M%dD' % k, [op(2, M), op(k, D), op(9, M)], rev=rev, ql=1, qr=4, tl=2, tr=6))
            out.append(homopolymer('lead-2M%dI-p2' % (2 * k), [op(2, M), op(2 * k, I), op(9, M)], period=2, rev=rev, ql=2, tl=3))
            out.append(homopolymer('lead-2M%dD-p2' % (2 * k), [op(2, M), op(2 * k, D), op(9, M)], period=2, rev=rev, qr=2, tr=3))
    for extra in (70, 130):     # the 64-op chunks of the move-down; the tail must not shift, so it lies on random sequence
        for head, g in (([op(1, M), op(2, I)], 'I'), ([op(2, M), op(3, D)], 'D')):
            tail = [op(int(rng.integers(2, 9)), M) if k % 2 == 0 else op(int(rng.integers(1, 4)), 1 + (k >> 1) % 2) for k in range(extra)]
            cigar = head + tail
            qn, tn = spans(cigar)
            hq, ht = spans(head)
            t = np.concatenate([np.zeros(ht + 6, np.uint8), rng.integers(0, 4, tn - ht - 6)]).astype(np.uint8)
            out.append(Aln('lead-%s-%dops' % (g, extra), cigar, walk(rng, cigar, t, 1, 0.0, 1.0), t, rev=extra == 130, ql=2, tl=7, rng=rng))
    out += [
        homopolymer('becomes-single', [op(3, M), op(2, I), op(4, M)], q_mut=[]),                  # the gap moves to the front: one M left
        homopolymer('becomes-empty', [op(0, M), op(0, I), op(0, M)]),
        homopolymer('becomes-single-D', [op(0, M), op(2, D), op(0, M), op(0, I)]),                # only a deletion is left, then removed
        on_random(rng, 'first-op-gap-I', [op(3, I), op(10, M), op(2, D), op(6, M)], ql=1, tl=1),
        on_random(rng, 'first-op-gap-D', [op(4, D), op(10, M), op(1, I), op(6, M)], rev=1, qr=5, tl=17),
        on_random(rng, 'first-two-gaps', [op(2, I), op(3, D), op(8, M)], tl=2),
    ]
    return out


def merge_edge_cases():
    rng = np.random.default_rng(102)
    c = lambda *xs: [op(n, o) for n, o in xs]  # noqa: E731
    out = [
        on_random(rng, '5I6D7I-middle', c((8, M), (5, I), (6, D), (7, I), (9, M))),
        on_random(rng, '5I6D7I-end', c((8, M), (5, I), (6, D), (7, I)), rev=1, ql=3),
        on_random(rng, '6D5I7D-end-after-0M', c((8, M), (6, D), (5, I), (0, M), (7, D))),
        on_random(rng, 'pair-at-end-k=n-2', c((8, M), (2, D), (6, M), (5, I), (6, D))),          # starts at k = n - 2: not looked at
        on_random(rng, '5I6D-alone', c((5, I), (6, D))),
        on_random(rng, '5I6D-between', c((7, M), (5, I), (6, D), (7, M)), rev=1),
        on_random(rng, 'I-0M-D', c((7, M), (3, I), (0, M), (2, D), (7, M))),                     # no two gaps are neighbours: the scan never starts
        on_random(rng, 'I-D-0M-I', c((7, M), (3, I), (2, D), (0, M), (4, I), (7, M))),
        on_random(rng, 'I-0M-I', c((7, M), (3, I), (0, M), (4, I), (7, M))),                     # one kind only: no merge, the shrink joins them
        on_random(rng, 'I-D-0I', c((7, M), (3, I), (2, D), (0, I), (7, M))),
        on_random(rng, '3M4M', c((3, M), (4, M), (2, I), (6, M))),                               # nothing asks for the shrink: they stay apart
        on_random(rng, '3M4M-shrink', c((3, M), (4, M), (2, I), (0, M), (6, M)), rev=1),
        on_random(rng, '2I3I', c((5, M), (2, I), (3, I), (6, M))),
        on_random(rng, '2I3I-shrink', c((5, M), (2, I), (3, I), (6, M), (0, D), (2, M))),
    ]
    # a third gap that joins an adjacent pair only when its saturated shift has emptied the match run between them
    for rev in (0, 1):
        out.append(homopolymer('adjacent-after-shift', c((4, M), (2, I), (1, D), (2, M), (3, I), (5, M)), rev=rev, ql=rev, tl=3))
        out.append(homopolymer('adjacent-after-shift-p2', c((4, M), (2, D), (2, I), (2, M), (4, D), (6, M)), period=2, rev=rev, tl=9))
    # the same gaps without the pair: 2I 0M 1D 0M 3I after the shifts, and no two gaps are neighbours for the scan to start at
    out.append(homopolymer('emptied-runs-no-pair', c((4, M), (2, I), (2, M), (1, D), (2, M), (3, I), (5, M)), tl=1))
    return out


def ambiguous_cases():
    rng = np.random.default_rng(103)
    out = []
    cigar = [op(20, M), op(3, I), op(15, M), op(4, D), op(30, M)]
    _, tn = spans(cigar)
    N = 4
    for where, (a, b, fl, fr) in dict(before=(0, 0, 6, 0), across_start=(0, 5, 6, 0), inside=(25, 45, 0, 0), across_end=(tn - 5, tn, 0, 6),
                                      after=(0, 0, 0, 6), all=(0, tn, 3, 3)).items():
        for rev in (0, 1):
            t = rng.integers(0, 4, tn).astype(np.uint8)
            t[a:b] = N
            q = walk(rng, cigar, t, 1, 0.05, 0.0)
            tl = np.concatenate([rng.integers(0, 4, 9), np.full(fl, N)])
            tr = np.concatenate([np.full(fr, N), rng.integers(0, 4, 11)])
            out.append(Aln('N-target-' + where, cigar, q, t, rev=rev, ql=2, qr=3, tl=tl, tr=tr, rng=rng))
    for rev in (0, 1):      # N in the read in M and I columns, N in D columns
        t = rng.integers(0, 4, tn).astype(np.uint8)
        t[36:39] = N                    # inside the deletion (target 35..39)
        q = walk(rng, cigar, t, 1, 0.05, 0.0)
        q[[3, 4, 21, 22, 50]] = N       # match columns and the insertion (read 20..23)
        out.append(Aln('N-read-M-I-target-D', cigar, q, t, rev=rev, ql=5, tl=3, rng=rng))
    # N inside a homopolymer next to a gap: N equals N in the shift comparison and nothing else
    for g in (I, D):
        for at in (3, 4, 5):
            cigar2 = [op(6, M), op(1, g), op(6, M)]
            a = homopolymer('N-next-to-gap', cigar2, rev=at & 1, ql=1, tl=2)
            q, t = a.q.copy(), a.t.copy()
            (q if g == I else t)[at] = N
            if at == 5:
                (q if g == I else t)[6] = N
            out.append(Aln('N-next-to-gap-%s-%d' % ('ID'[g - 1], at), cigar2, q, t, rev=at & 1, ql=1, tl=2, rng=rng))
    return out


def dpmax_cases():
    """running scores that clip to 0 inside a lane's range of ops, exactly at a range boundary and across several whole ranges; the
    peak before or after the clip; few ops (most ranges empty); all mismatches"""
    rng = np.random.default_rng(104)
    out = []

    def build(name, n_ops, bad_from, bad_to, long_gap_at=None, head_m=6, tail_m=6, rev=0):
        cigar = []
        for k in range(n_ops):
            if k % 2 == 0:
                cigar.append(op(head_m if k < bad_from else tail_m, M))
            else:
                cigar.append(op(40 if k == long_gap_at else 1, 1 + (k >> 1) % 2))
        _, tn = spans(cigar)
        t = rng.integers(0, 4, tn).astype(np.uint8)
        q, ti = [], 0
        for k, c in enumerate(cigar):
            ln, o = c >> 4, c & 15
            for _ in range(ln):
                if o == M:
                    q.append((int(t[ti]) + 1) % 4 if bad_from <= k < bad_to else int(t[ti]))
                    ti += 1
                elif o == I:
                    q.append(int(rng.integers(0, 4)))
                else:
                    ti += 1
        out.append(Aln(name, cigar, q, t, rev=rev, ql=1, qr=2, tl=3, tr=4, rng=rng))

    per = 4     # 256 ops: four per lane
    build('clip-inside-range', 256, 4 * per + 1, 4 * per + 3)
    build('clip-at-boundary', 256, 8 * per, 9 * per, rev=1)
    build('clip-several-ranges', 256, 10 * per, 17 * per)
    build('clip-long-gap-inside', 256, 300, 300, long_gap_at=20 * per + 1, rev=1)
    build('clip-long-gap-boundary', 256, 300, 300, long_gap_at=20 * per - 1)
    build('peak-before-clip', 256, 40 * per, 50 * per, head_m=9, tail_m=2)
    build('peak-after-clip', 256, 5 * per, 9 * per, head_m=2, tail_m=9, rev=1)
    build('clip-per2', 128, 30, 75)
    build('clip-per3-odd', 129, 29, 76, rev=1)
    build('few-ops', 9, 3, 5)
    build('few-ops-63', 63, 20, 41, rev=1)
    build('all-mismatch', 33, 0, 33)
    build('all-mismatch-1op', 1, 0, 1, rev=1)
    return out


def sized(rng, name, need, n_ops, period=0, **kw):
    """an alignment whose LDS need is exactly `need` bytes with n_ops ops: the last match run is stretched, and one insertion by
    up to 3 bases where both spans would cross a word together"""
    base = alt_cigar(rng, n_ops, m_max=3 if n_ops > 1000 else 11, g_max=2 if n_ops > 1000 else 5)
    last_m = max(k for k, c in enumerate(base) if c & 15 == M)
    an_i = max(k for k, c in enumerate(base) if c & 15 == I)
    qn, tn = spans(base)
    want = need - 16 - 8 * n_ops
    for di in range(4):
        x = max(0, (want - qn - tn - di) // 2 - 8)
        while ((qn + di + x + 3) & ~3) + ((tn + x + 3) & ~3) < want:
            x += 1
        if ((qn + di + x + 3) & ~3) + ((tn + x + 3) & ~3) == want:
            base[last_m] += x << 4
            base[an_i] += di << 4
            a = on_repeat(rng, name, base, period, **kw) if period else on_random(rng, name, base, **kw)
            assert a.need == need, (name, a.need, need)
            return a
    raise AssertionError(name)


def size_class_cases():
    """needs of exactly kLds and kLds + 4 for each LDS class, once mostly through ops and once mostly through span, interleaved with
    small alignments (so that job ids differ from list positions), and three more alignments of different sizes beyond every class,
    one of them a period-2 repeat"""
    rng = np.random.default_rng(105)
    out = []
    small = lambda i: on_repeat(rng, 'small-%d' % i, alt_cigar(rng, 5 + 9 * i), 1 + i % 3, rev=i & 1, ql=i % 4, tl=i % 17)  # noqa: E731
    i = 0
    for lds in LDS_CLASSES:
        for need in (lds, lds + 4):
            out.append(sized(rng, 'ops-%d' % need, need, lds // 8 * 3 // 4, rev=i & 1, ql=i % 3, tl=i % 13))
            out.append(small(i))
            out.append(sized(rng, 'span-%d' % need, need, 180 + i, rev=~i & 1, qr=i % 5, tl=(5 * i) % 16))
            i += 1
            if i % 2:
                out.append(small(i + 10))
    out.insert(1, on_repeat(rng, 'global-repeat-p2', alt_cigar(rng, 9001), 2, rev=1, ql=2, tl=5))
    out.insert(9, on_repeat(rng, 'global-repeat-p1', alt_cigar(rng, 8300, m_max=14), 1, tl=11))
    out.append(on_random(rng, 'global-span', alt_cigar(rng, 301, m_max=500), ql=1, tl=3))
    return out


def offset_cases():
    """every qs mod 4 and (read_len - qe) mod 4 on both strands, every (t_off + ts) mod 16, in the order of the call (what precedes
    a pair moves its words).  The first pair is a reverse-strand alignment at the very start of the first read: the 4-byte load
    of its last group reaches below the buffer.  The last target interval ends in the last word of the packed array."""
    rng = np.random.default_rng(106)
    out, cum_q, cum_t = [], 0, 0
    for rev in (1, 0):
        for a in range(16):
            cigar = alt_cigar(rng, 9 + a % 3)
            qn = spans(cigar)[0]
            ql = 0 if (rev and a == 0) else (a % 4 - cum_q) % 4
            qr = (a // 4 - (cum_q + ql + qn)) % 4      # the read's length as a whole mod 4: where the reverse strand starts reading
            tl = (a - cum_t) % 16
            p = on_repeat(rng, 'off-%d-%d' % (rev, a), cigar, 1 + a % 2, rev=rev, ql=ql, qr=qr, tl=tl, tr=0 if a == 15 else a % 3)
            p.off_qs, p.off_qe, p.off_t = (cum_q + p.qs) % 4, (len(p.read) - p.qe) % 4, (cum_t + p.ts) % 16
            cum_q += len(p.read)
            cum_t += len(p.target)
            out.append(p)
    return out


def zero_span_cases():
    rng = np.random.default_rng(107)
    return [
        on_random(rng, 'qspan-0', [op(7, D)], ql=3, qr=2, tl=4, tr=1),
        on_random(rng, 'qspan-0-ops', [op(0, M), op(7, D), op(0, M)], rev=1, ql=3, tl=4),
        on_random(rng, 'tspan-0', [op(6, I)], ql=1, tl=9),
        on_random(rng, 'tspan-0-ops', [op(0, M), op(6, I), op(0, M)], rev=1, qr=1, tl=0, tr=0),
        on_random(rng, 'both-0', [op(0, M)], ql=2, tl=2),
    ]


# hand-worked cases: (name, cigar, q, t, expected) with q / t as strings over ACGTN, expected under the default scoring
# (a 2, b 4, ambiguous 1, gap 4 + 2 per base); found regressions are added here by name
HAND = [
    # AAAAAA against AAAAA, the inserted A after three: it slides to the front and becomes a leading gap of the read
    ('homopolymer-gap-to-front', [op(3, M), op(1, I), op(2, M)], 'AAAAAA', 'AAAAA',
     dict(n_cigar=1, qshift=1, tshift=0, blen=5, mlen=5, n_ambi=0, dp_max=10, cigar=[op(5, M)])),
    # 3M 2I 0M 4D 1I 5M: 2I lies between two match runs (the second one empty) but G != T, so it stays; 4D and 1I have a gap for a
    # neighbour.  The merge scan looks at 2I + 0M (no pair), skips the empty run, and finds 4D 1I: both kinds but only two ops,
    # which stay as they are.  The empty op is dropped: 3M 2I 4D 1I 5M.  Score: 6, then every gap clips it to 0, then 10.
    ('3M2I0M4D1I5M', [op(3, M), op(2, I), op(0, M), op(4, D), op(1, I), op(5, M)], 'ACGTTACGTAC', 'ACGGGGGCGTAC',
     dict(n_cigar=5, qshift=0, tshift=0, blen=15, mlen=8, n_ambi=0, dp_max=10, cigar=[op(3, M), op(2, I), op(4, D), op(1, I), op(5, M)])),
    # an empty insertion between two match runs: every base before it "equals" the gap's last base (the same base: len 0), so
    # the whole left run moves right, the shrink drops both empty ops
    ('0I-moves-left-run', [op(4, M), op(0, I), op(3, M)], 'ACGTACG', 'ACGTACG',
     dict(n_cigar=1, qshift=0, tshift=0, blen=7, mlen=7, n_ambi=0, dp_max=14, cigar=[op(7, M)])),
    # two ops: no gap has two neighbours, nothing to do; 4M = 8, then 2D costs 8
    ('two-ops', [op(4, M), op(2, D)], 'ACGT', 'ACGTAA',
     dict(n_cigar=2, qshift=0, tshift=0, blen=6, mlen=4, n_ambi=0, dp_max=8, cigar=[op(4, M), op(2, D)])),
    # one op is returned untouched even when it is a gap (and counts its N as ambiguous)
    ('one-op-gap', [op(3, I)], 'ANG', '',
     dict(n_cigar=1, qshift=0, tshift=0, blen=2, mlen=0, n_ambi=1, dp_max=0, cigar=[op(3, I)])),
    ('one-op-match', [op(3, M)], 'ACG', 'ATG',
     dict(n_cigar=1, qshift=0, tshift=0, blen=3, mlen=2, n_ambi=0, dp_max=2, cigar=[op(3, M)])),
]


def hand_alns():
    code = {c: i for i, c in enumerate('ACGTN')}
    return [Aln(name, cigar, [code[c] for c in q], [code[c] for c in t], rev=k & 1, ql=k % 3, tl=k % 5) for k, (name, cigar, q, t, _) in enumerate(HAND)]


def families():
    """name -> list of Aln; every family of both test files"""
    f = {'period-%d' % p: repeat_family(p) for p in PERIODS}
    f.update(leading=leading_gap_cases(), merge=merge_edge_cases(), ambiguous=ambiguous_cases(), dpmax=dpmax_cases(),
             sizes=size_class_cases(), offsets=offset_cases(), zero_span=zero_span_cases(), hand=hand_alns())
    return f
