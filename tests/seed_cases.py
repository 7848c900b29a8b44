"""Constructed inputs for the seed half of the mapper (tests/test_seed_ref.py, tests/test_seed_stage_gpu.py): made indexes and made
minimizers, seeded and small, one family per group of kernels.  Data only, apart from each case's `reach`: a function of the
restatement's results (seed_ref.py) that asserts the case still reaches what it is named for.

A case: name, index (seed_ref.MadeIndex), reads [(minimizers (n, 2) uint64, seq_len)], opt (mid_occ, min_cnt, max_gap), knobs: knob
sets the case runs with beside the standard ones, reach(case, refs) with refs = reference(case, knobs)."""
from collections import namedtuple

import numpy as np

from seed_ref import MadeIndex, U64, bucket_sizes, collect_np, filter_bins, list_counts, needed, sketch_rule, word

Case = namedtuple('Case', 'name index reads opt knobs reach')
FAMILIES = ('lookup', 'occ', 'walk', 'rounds', 'emit', 'sort')
BIG = [1 << 27] * 5000        # a large shift of the sort's bins: a whole target (and strand) is one bin
STD_KNOBS = ({}, dict(grid_cap=1), dict(grid_cap=3), dict(flt_wgs=1), dict(flt_round2=1))


def options(mid_occ=200, min_cnt=1, max_gap=5000):
    return dict(mid_occ=mid_occ, min_cnt=min_cnt, max_gap=max_gap)


class World:
    def __init__(self, seed, lens=BIG, k=15):
        self.rng = np.random.default_rng(seed)
        self.k, self.lens, self.table = k, lens, {}

    def fresh(self):
        while True:
            h = int(self.rng.integers(1, (1 << 2 * self.k) - 1))
            if h not in self.table:
                return h

    def key(self, words, h=None):
        h = self.fresh() if h is None else h
        assert h not in self.table
        self.table[h] = sorted(int(w) for w in words)
        return h

    def keys_of(self, words, per=100):
        """the words dealt at random to keys of at most `per` positions: the keys' position lists interleave"""
        words = [int(w) for w in words]
        order = self.rng.permutation(len(words))
        n_k = max(1, -(-len(words) // per))
        return [self.key([words[j] for j in order[i::n_k]]) for i in range(n_k)] if words else []

    def index(self):
        return MadeIndex(self.k, self.lens, self.table)


def make_read(items, first=300, step=7, tail=40):
    """items: (hash, span, strand[, last_pos]); without a last_pos the minimizers stand `step` bases apart"""
    mz, last = [], first - step
    for it in items:
        last = it[3] if len(it) > 3 else last + step
        mz.append((it[0] << 8 | it[1], last << 1 | it[2]))
    return np.array(mz, dtype=U64).reshape(-1, 2), (last + tail if items else 50)


def shuffled(rng, items):
    return [items[j] for j in rng.permutation(len(items))]


def reference(case, knobs=None):
    """per read dict(a, n_anchor, rep_len, span_sum, keep, sizes, rounds): collect, what the device's filter keeps of it, the sizes
    of the sort's buckets over the kept anchors, the hits each of the filter's rounds walks"""
    r2 = (knobs or {}).get('flt_round2', 0)
    out = []
    for mz, qlen in case.reads:
        a, n_a, rep, ss = collect_np(case.index, mz, qlen, case.opt['mid_occ'])
        rounds = []
        keep = sketch_rule(a, case.opt['max_gap'], case.opt['min_cnt'], r2, rounds)
        out.append(dict(a=a, n_anchor=n_a, rep_len=rep, span_sum=ss, keep=keep, sizes=bucket_sizes(a[keep], case.index.lens), rounds=rounds))
    return out


def emission_differs(case, refs):
    """the order the hits are emitted in (minimizer after minimizer, a key's positions in the index's order) is not the sorted one"""
    for (mz, qlen), r in zip(case.reads, refs):
        x = [int(w) for m in mz for w in case.index.get(int(m[0]) >> 8)]
        if len(x) == r['n_anchor'] and len(x) > 1 and x != sorted(x):
            return True
    return False


def all_sizes(refs):
    return sorted(int(s) for r in refs for s in r['sizes'])


# ---- lookup ----------------------------------------------------------------------------------------------------------------------
def lookup_cases():
    out = []
    for n_keys, bbits in ((40, 8), (5000, 11)):
        w = World(100 + n_keys, lens=[20000] * 3)
        s = 2 * w.k - bbits
        nb = 1 << bbits
        place = lambda: word(int(w.rng.integers(0, 3)), int(w.rng.integers(0, 20000)), int(w.rng.integers(0, 2)))   # noqa: E731
        named = dict(first=1 << s | 9, b_first=3 << s, b_mid1=3 << s | 100, b_mid2=3 << s | 200, b_last=3 << s | ((1 << s) - 1), alone=7 << s | 77,
                     last=(nb - 1) << s | 3)
        for h in named.values():
            w.key([place() for _ in range(int(w.rng.integers(1, 4)))], h)
        while len(w.table) < n_keys:                      # the rest: buckets 10 .. nb - 2, so that bucket 5 stays empty and 7 holds one key
            h = int(w.rng.integers(10, nb - 1)) << s | int(w.rng.integers(0, 1 << s))
            if h not in w.table:
                w.key([place() for _ in range(int(w.rng.integers(1, 4)))], h)
        miss = dict(below=1 << s | 8, zero=0, above=(nb - 1) << s | 4, top=(1 << 2 * w.k) - 1, empty_bucket=5 << s | 9, between=3 << s | 150,
                    before_alone=7 << s | 76, after_alone=7 << s | 78)
        assert not set(miss.values()) & set(w.table)
        items = shuffled(w.rng, [(h, 15, i & 1) for i, h in enumerate(list(named.values()) + list(miss.values()))])
        others = shuffled(w.rng, [(h, 15, 0) for h in list(w.table)[:200]])
        idx = w.index()
        assert 2 * w.k - min(max(8, bbits), 2 * w.k) == s

        def reach(case, refs, named=named, n_named=len(named), n_miss=len(miss)):
            hit = sum(len(case.index.get(h)) for h in named.values())
            assert refs[0]['n_anchor'] == hit and len(case.reads[0][0]) == n_named + n_miss and emission_differs(case, refs)
        out.append(Case('keys%d' % n_keys, idx, [make_read(items), make_read(others), make_read([])], options(mid_occ=10), (), reach))
    w = World(102, lens=[1000])
    out.append(Case('empty-index', w.index(), [make_read([(5, 15, 0), ((1 << 30) - 1, 15, 1), (0, 15, 0)]), make_read([])], options(), (),
                    lambda case, refs: None if len(case.index.keys) == 0 and all(r['n_anchor'] == 0 for r in refs) else 1 / 0))
    return out


# ---- occurrence cut-off, rep_len, span_sum -----------------------------------------------------------------------------------------
def occ_cases():
    w = World(110, lens=[50000] * 4)
    place = lambda: word(int(w.rng.integers(0, 4)), int(w.rng.integers(0, 50000)), int(w.rng.integers(0, 2)))   # noqa: E731
    mid = 5
    under, at, over = (w.key([place() for _ in range(c)]) for c in (mid - 1, mid, mid + 1))
    rare = [w.key([place() for _ in range(int(w.rng.integers(1, 4)))]) for _ in range(40)]
    reps = [at, over] + [w.key([place() for _ in range(int(w.rng.integers(mid, 12)))]) for _ in range(6)]
    gone = [w.fresh() for _ in range(8)]
    reads = []
    # intervals [last + 1 - span, last + 1) of the repetitive minimizers: overlapping, touching, disjoint, nested (same end), and a
    # rare minimizer between two of them
    reads.append(make_read([(at, 20, 0, 100), (over, 20, 1, 110), (rare[0], 15, 0, 120), (reps[2], 20, 0, 130), (under, 15, 0, 150), (reps[3], 15, 1, 200),
                            (reps[4], 5, 0, 200), (reps[5], 2, 0, 201), (reps[6], 255, 0, 600), (reps[7], 1, 1, 600)]))
    rep_at = {0, 1, 5, 30, 61, 62, 63, 64, 65, 66, 100, 126, 127, 128}
    for n in (0, 1, 63, 64, 65, 128, 129):          # spans of 15 every 5 bases: neighbours overlap, also across the tiles of 64
        reads.append(make_read([(reps[i % len(reps)] if i in rep_at else rare[i % len(rare)], 15, i & 1) for i in range(n)], first=30, step=5))
    reads.append(make_read([(reps[i % len(reps)], 15, 0) for i in range(70)], first=30, step=20))      # all repetitive, disjoint intervals
    reads.append(make_read([(gone[i % len(gone)], 15, 0) for i in range(70)]))                          # no key found
    reads.append(make_read([(rare[1], 1, 0, 0), (rare[2], 255, 1, 254), (rare[3], 255, 0, 254), (rare[4], 1, 1, 900), (under, 255, 0, 1000)]))

    def reach(case, refs):
        assert [len(case.index.get(h)) for h in (under, at, over)] == [mid - 1, mid, mid + 1]
        assert refs[0]['rep_len'] == (131 - 81) + (202 - 186) + (601 - 346) and refs[0]['n_anchor'] == len(case.index.get(rare[0])) + mid - 1
        assert refs[8]['n_anchor'] == 0 and refs[8]['rep_len'] == 70 * 15 and refs[9]['n_anchor'] == 0 and refs[9]['rep_len'] == 0
        assert [len(r[0]) for r in case.reads[1:8]] == [0, 1, 63, 64, 65, 128, 129] and refs[7]['rep_len'] > 0
        assert refs[10]['span_sum'] == sum(len(case.index.get(h)) * s for h, s in ((rare[1], 1), (rare[2], 255), (rare[3], 255), (rare[4], 1), (under, 255)))
    return [Case('cut-off', w.index(), reads, options(mid_occ=mid), (), reach)]


# ---- the filter's walk over the hits ------------------------------------------------------------------------------------------------
def distinct(words, n):
    """the first n distinct ones (a word twice in one key would be one anchor twice: nothing orders the two)"""
    out = list(dict.fromkeys(int(v) for v in words))[:n]
    assert len(out) == n
    return out


def stepped(rng, n, start, gap, limit):
    """n ascending positions from steps of {0 (a duplicate), 1, gap / 2 + 1, gap, gap + 1, 2 gap, 10 gap}"""
    steps = [0, 1, gap // 2 + 1, gap, gap + 1, 2 * gap, 10 * gap]
    p, out = start, []
    for _ in range(n):
        out.append(p % limit)
        p += steps[int(rng.integers(0, len(steps)))]
    return out


def walk_cases():
    out = []
    far = (1 << 30) + (1 << 25)
    for min_cnt, max_gap in ((2, 300), (3, 5000), (5, 300), (2, 1), (3, 40000)):
        w = World(120 + min_cnt * 7 + max_gap % 11, lens=[far, 1 << 22, 1 << 22])
        _, sh = filter_bins(max_gap, min_cnt)
        W = 1 << sh
        words = lambda n, rid: distinct([word(rid, p, int(w.rng.integers(0, 2))) for p in stepped(w.rng, 2 * n + 8, int(w.rng.integers(0, 1 << 20)), max_gap, 1 << 22)], n)   # noqa: E731
        # one block of minimizers: owners of 50, 46 and 4000 hits before the chunk of 4096 slots ends, one of 30 that starts exactly on
        # slot 4096, one of 5000 that crosses the windows of 64, the steps of 256 and slot 8192
        k50, k46, k4000, k30, k5000 = (w.key(words(c, 1 + (c & 1))) for c in (50, 46, 4000, 30, 5000))
        small = [w.key(words(int(w.rng.integers(1, 9)), 2)) for _ in range(40)]
        gone = [w.fresh() for _ in range(64)]
        # bin edges: k W - 1 and k W, W / 2 apart, max_gap and max_gap + 1 apart; above 2^30; one place on two targets and both strands
        edge = [3 * W - 1, 3 * W, 3 * W + W // 2, 9 * W - 1, 20 * W, 20 * W + max_gap, 40 * W, 40 * W + max_gap + 1, 60 * W + W // 2 - 1, 60 * W + W // 2]
        k_edge = [w.key([word(0, p, 0)]) for p in edge] + [w.key([word(0, (1 << 30) + p, 1) for p in edge])]
        same = [w.key([word(r, 7 * W, s)]) for r in (1, 2) for s in (0, 1)]
        reads = [make_read([(h, 15, i & 1) for i, h in enumerate([k50, k46, k4000, k30, k5000] + small[:8])]),
                 make_read([(h, 15, 0) for h in small[:32] + small[:32] + gone + small[32:] + k_edge]),           # a block without any hit between two with hits
                 make_read([(h, 15, 1) for h in shuffled(w.rng, k_edge + same + small + small[:9])] + [(small[5], 15, 0)]),   # 65: the last block holds one
                 make_read([(h, 15, 0) for h in same])]
        # two true loci among strays, 60 minimizers 7 bases apart each: one on the read's strand, one on the other (target positions falling)
        line = [w.key([word(1, 2000000 + 7 * i + int(w.rng.integers(0, 2)), 0)] + words(3, 2)) for i in range(60)]
        line += [w.key([word(2, 3000000 - 7 * i, 1)] + words(2, 1)) for i in range(60)]
        reads.append(make_read([(h, 15, 0) for h in line]))

        def reach(case, refs, hits=(50, 46, 4000, 30, 5000)):
            mz = case.reads[0][0]
            t = [len(case.index.get(int(m[0]) >> 8)) for m in mz]
            assert tuple(t[:5]) == hits and sum(t[:3]) == 4096 and sum(t[:4]) < 8192 < sum(t[:5]) and len(mz) <= 64
            t1 = [len(case.index.get(int(m[0]) >> 8)) for m in case.reads[1][0]]
            assert sum(t1[:64]) > 0 and sum(t1[64:128]) == 0 and sum(t1[128:]) > 0
            assert len(case.reads[2][0]) == 65 and refs[3]['n_anchor'] == 4 and needed(refs[4]['a'], 5000, 3).sum() >= 120
            assert not refs[3]['keep'].any() or case.opt['min_cnt'] < 2          # two targets x two strands: never counted together
            assert any(int(a[0]) & 0xffffffff > 1 << 30 for r in refs for a in r['a'][r['keep']][:50]) or case.opt['min_cnt'] > 2
            some = sum(int(r['keep'].sum()) for r in refs)
            assert 0 < some < sum(r['n_anchor'] for r in refs)                   # the filter drops some hits and keeps some
        out.append(Case('cnt%d-gap%d' % (min_cnt, max_gap), w.index(), reads, options(mid_occ=6000, min_cnt=min_cnt, max_gap=max_gap), (), reach))
    return out


# ---- the second counting round, the persistent workgroups ---------------------------------------------------------------------------
def rounds_cases():
    out = []
    w = World(130, lens=[1 << 22] * 8)
    words = lambda n: distinct([word(int(w.rng.integers(0, 8)), p, int(w.rng.integers(0, 2))) for p in stepped(w.rng, 2 * n + 8, int(w.rng.integers(0, 1 << 20)), 300, 1 << 22)], n)   # noqa: E731
    keys = [w.key(words(int(w.rng.integers(1, 11)))) for _ in range(200)]
    pick = lambda hits: [(keys[int(j)], 15, int(j) & 1) for j in w.rng.integers(0, len(keys), hits // 5)]   # noqa: E731
    five = [make_read(pick(h)) for h in (100, 200, 0, 400, 50)]

    def reach_five(case, refs):
        n = [r['n_anchor'] for r in refs]
        assert min(n[0], n[1]) < 150 <= max(n[0], n[1]) and len(refs) == 5
        two = reference(case, dict(flt_round2=150))
        assert [len(r['rounds']) for r in two] == [2 if r['n_anchor'] >= 150 else min(r['n_anchor'], 1) for r in two] and {1, 2} <= {len(r['rounds']) for r in two}
    out.append(Case('five-reads', w.index(), five, options(min_cnt=3, max_gap=300), (dict(flt_round2=150), dict(flt_round2=150, flt_wgs=1)), reach_five))

    many = [make_read(pick(int(h) * 5)) for h in w.rng.integers(0, 9, 300)]

    def reach_many(case, refs):
        classes = {(r['n_anchor'] + 1).bit_length() for r in refs}
        assert len(refs) == 300 and 0 in [r['n_anchor'] for r in refs] and len(classes) >= 5 and max(r['n_anchor'] for r in refs) <= 80
    out.append(Case('300-reads', w.index(), many, options(min_cnt=2, max_gap=300), (dict(flt_wgs=3), dict(flt_wgs=3, flt_round2=20)), reach_many))

    # one read of ~200 000 hits: 150 loci of 70 colinear hits among strays spread over 64 targets, more than the tables hold
    w = World(131, lens=[1 << 27] * 64)
    stray = [word(int(r), int(p), int(s)) for r, p, s in zip(w.rng.integers(0, 64, 190000), w.rng.integers(0, 1 << 27, 190000), w.rng.integers(0, 2, 190000))]
    loci = [word(int(rid), int(p0) + 37 * j, 0) for rid, p0 in zip(w.rng.integers(0, 64, 150), w.rng.integers(0, (1 << 27) - 4000, 150)) for j in range(70)]
    big = [make_read([(h, 15, 0) for h in w.keys_of(list(dict.fromkeys(stray + loci)), per=100)], step=5)]

    def reach_big(case, refs):
        r = refs[0]
        assert 195000 <= r['n_anchor'] <= 205000 and len(np.unique(r['a'], axis=0)) == r['n_anchor']
        nd = needed(r['a'], 5000, 3)
        assert nd.sum() >= 150 * 70 and r['keep'].sum() > 2 * nd.sum()          # overfilled: many strays pass the first round
        two = reference(case, dict(flt_round2=20000))[0]
        assert len(two['rounds']) == 2 and two['keep'].sum() < r['keep'].sum() and (two['keep'] >= nd).all()
    out.append(Case('saturated', w.index(), big, options(min_cnt=3, max_gap=5000), (dict(flt_round2=20000),), reach_big))
    return out


# ---- emission -------------------------------------------------------------------------------------------------------------------------
def emit_cases():
    w = World(140, lens=[30000] * 6)
    place = lambda: word(int(w.rng.integers(0, 6)), int(w.rng.integers(0, 30000)), int(w.rng.integers(0, 2)))   # noqa: E731
    keys = [w.key([place() for _ in range(int(w.rng.integers(1, 6)))]) for _ in range(80)]
    both = w.key([word(2, 500, 0), word(2, 900, 1), word(4, 100, 0), word(4, 101, 1)])
    gone = w.fresh()
    reads = []
    # reverse hits whose read position comes from last_pos = span - 1 (the read's first k-mer) and last_pos = seq_len - 1 (its last)
    mz = np.array([(both << 8 | 15, 14 << 1 | 0), (both << 8 | 15, 14 << 1 | 1), (keys[0] << 8 | 21, 20 << 1 | 1), (both << 8 | 15, 999 << 1 | 0),
                   (both << 8 | 15, 999 << 1 | 1)], dtype=U64)
    reads.append((mz, 1000))
    # tandem neighbours (equal hashes side by side) at the read's first and last minimizers and across the blocks of 64
    seq = [keys[i % 80] for i in range(130)]
    seq[1] = seq[0]
    seq[64] = seq[63]
    seq[129] = seq[128]
    seq[20] = seq[22] = keys[7]          # equal hashes that are no neighbours: no flag
    seq[21] = gone
    reads.append(make_read([(h, 15, i % 3 == 0) for i, h in enumerate(seq)]))
    # a minimizer without hits between two with hits: it shares its start slot with its successor
    reads.append(make_read([(keys[3], 15, 0), (gone, 15, 0), (keys[4], 15, 1), (gone, 15, 1), (gone, 15, 0), (keys[5], 17, 0)]))

    def reach(case, refs):
        a = refs[0]['a']
        rev = a[a[:, 0] >> U64(63) == 1]
        assert len(rev) and {14, 999} <= {int(y) & 0xffffffff for y in rev[:, 1]} and {14, 999} <= {int(y) & 0xffffffff for y in a[a[:, 0] >> U64(63) == 0][:, 1]}
        t = refs[1]['a'][:, 1] >> U64(42) & U64(1)
        assert 0 < t.sum() < len(t) and emission_differs(case, refs)
    return [Case('strands-tandem', w.index(), reads, options(mid_occ=10), (), reach)]


# ---- the anchor sort ------------------------------------------------------------------------------------------------------------------
def bucket(w, rid, n, strand=0, per=100):
    """keys whose n distinct positions all lie on one strand of target rid: one bucket of the sort under the large shift"""
    p = w.rng.choice(1 << 20, n, replace=False)
    return w.keys_of([word(rid, int(v), strand) for v in p], per=per)


def sort_cases():
    out = []

    def sized(name, seed, sizes_per_read):
        w = World(seed)
        reads = []
        for sizes in sizes_per_read:
            items = [(h, 15, 0) for j, n in enumerate(sizes) for h in bucket(w, 10 + 7 * j, n, strand=j & 1)]
            reads.append(make_read(shuffled(w.rng, items), step=3))
        want = sorted(n for sizes in sizes_per_read for n in sizes)

        def reach(case, refs, want=want):
            assert all_sizes(refs) == want and emission_differs(case, refs)
            assert list_counts(all_sizes(refs)) == list_counts(want)
        out.append(Case(name, w.index(), reads, options(), (), reach))
    sized('sizes-small', 150, [[1, 2, 15, 16, 17, 18], [], [18, 17, 16, 15, 2, 1]])
    sized('sizes-1024', 151, [[1023, 1024, 1025]])
    sized('sizes-4096', 152, [[4095, 4096, 4097]])
    sized('sizes-9000', 153, [[9000, 3]])
    # buckets of 16 and 17 that start at positions 1008, 1023 and 1024 of the first window of 1024 anchors: single anchors on targets
    # of their own before them, a few behind
    for size in (16, 17):
        for at in (1008, 1023, 1024):
            w = World(160 + size + at)
            single = [w.key([word(r, int(w.rng.integers(0, 1 << 20)), 0)]) for r in w.rng.permutation(at)]
            after = [w.key([word(3000 + r, int(w.rng.integers(0, 1 << 20)), 0)]) for r in range(5)]
            items = [(h, 15, 0) for h in single + bucket(w, 2000, size, per=6) + after]

            def reach(case, refs, size=size, at=at):
                s = [int(v) for v in refs[0]['sizes']]
                assert s[:at] == [1] * at and s[at] == size and len(s) == at + 6 and emission_differs(case, refs)
            out.append(Case('straddle-%d-at-%d' % (size, at), w.index(), [make_read(shuffled(w.rng, items), step=3)], options(), (), reach))
    # read boundaries inside a window: 300 reads of two or three anchors in ONE bin (the bin at the end of a read is the bin at the start of
    # the next), empty reads between them
    w = World(170)
    gone = w.fresh()
    reads = []
    for i in range(300):
        p = sorted(int(v) for v in w.rng.choice(1 << 20, 3, replace=False))
        reads.append(make_read([(w.key([word(77, p[0], 0), word(77, p[2], 0)]), 15, 0), (w.key([word(77, p[1], 0)]), 15, 0)]))
        if i % 50 == 7:
            reads += [make_read([]), make_read([(gone, 15, 0)])]

    def reach_b(case, refs):
        n = [r['n_anchor'] for r in refs]
        assert sum(n) > 600 and sum(1 for v in n[:280] if v) > 256 and sum(n[:280]) < 1024 and 0 in n and emission_differs(case, refs)
    out.append(Case('boundaries', w.index(), reads, options(), (), reach_b))
    # batch totals around the window of 1024 and its 16 extra records
    for total in (1, 1023, 1024, 1025, 1040, 1041, 2048):
        w = World(180 + total)
        sizes, left = [], total
        while left:
            sizes.append(min(left, int(w.rng.integers(1, 17))))
            left -= sizes[-1]
        cut = sorted(int(v) for v in w.rng.integers(0, len(sizes) + 1, 2))
        reads = []
        for part in (sizes[:cut[0]], sizes[cut[0]:cut[1]], sizes[cut[1]:]):
            items = [(h, 15, 0) for j, n in enumerate(part) for h in bucket(w, 5 + j, n, per=4)]
            reads.append(make_read(shuffled(w.rng, items), step=3))
        out.append(Case('total-%d' % total, w.index(), reads, options(), (),
                        lambda case, refs, total=total: None if sum(r['n_anchor'] for r in refs) == total and max(all_sizes(refs)) <= 16 and
                        (total == 1 or emission_differs(case, refs)) else 1 / 0))
    # shift 0: one target of 8192 bases, every position a bin of its own; anchors with equal x that only the read position orders, with
    # differing spans and tandem flags: 1, 2, 16, 17, 18 and 40 minimizers on one key each
    w = World(190, lens=[8192])
    items = []
    for j, reps in enumerate((1, 2, 16, 17, 18, 40)):
        h = w.key([word(0, 100 + 50 * j, 0)])
        items += [(h, 11 + (i % 5), 0) for i in range(reps)]
    extra = [w.key([word(0, int(p), int(w.rng.integers(0, 2))) for p in 1000 + w.rng.choice(7000, 3, replace=False)]) for _ in range(200)]
    items = shuffled(w.rng, items + [(h, 15, 1) for h in extra])

    def reach_0(case, refs):
        from seed_ref import sort_bins
        assert sort_bins(refs[0]['a'], case.index.lens)[1] == 0 and {16, 17, 18, 40} <= set(all_sizes(refs))
        a = refs[0]['a']
        eq = a[1:, 0] == a[:-1, 0]
        assert eq.sum() > 80 and ((a[1:, 1] >> U64(32))[eq] != (a[:-1, 1] >> U64(32))[eq]).any() and emission_differs(case, refs)
    out.append(Case('shift0', w.index(), [make_read(items, step=3)], options(), (), reach_0))
    return out


_MAKERS = dict(lookup=lookup_cases, occ=occ_cases, walk=walk_cases, rounds=rounds_cases, emit=emit_cases, sort=sort_cases)


def families():
    return {name: _MAKERS[name]() for name in FAMILIES}


def merged(cases, seed=5):
    """the reads of several cases with one option set as ONE case over one index: every case's targets behind those of the cases before
    it, its hashes (found or not) mapped one to one to hashes no other case uses"""
    rng = np.random.default_rng(seed)
    k = cases[0].index.k
    lens, table, reads, used = [], {}, [], set()
    for c in cases:
        assert c.index.k == k and c.opt == cases[0].opt
        hs = sorted({int(h) for h in c.index.keys} | {int(x) >> 8 for mz, _ in c.reads for x in mz[:, 0]})
        to = {}
        for h in hs:
            while True:
                v = int(rng.integers(0, 1 << 2 * k))
                if v not in used:
                    break
            used.add(v)
            to[h] = v
        shift = len(lens) << 32
        for h in (int(v) for v in c.index.keys):
            table[to[h]] = [int(v) + shift for v in c.index.get(h)]
        lens += [int(v) for v in c.index.lens]
        for mz, qlen in c.reads:
            m2 = mz.copy()
            if len(m2):
                m2[:, 0] = [to[int(x) >> 8] << 8 | int(x) & 0xff for x in mz[:, 0]]
            reads.append((m2, qlen))
    return Case('+'.join(c.name for c in cases), MadeIndex(k, lens, table), reads, dict(cases[0].opt), (), None)
