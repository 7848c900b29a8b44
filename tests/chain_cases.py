"""Constructed anchors for the chaining stage: families of reads, each with an option set, built to reach one mechanism of the
chaining kernels (csrc/map_kernels.h: compaction, segment cutting, chain DP, chain ends, their sort, both backtracks) on purpose and
at the smallest size that still reaches it.  test_chain_ref.py pins the restatement (chain_ref.py) to the oracle on every family and
asserts from the restatement's record that each family reaches what it is here for; test_chain_stage_gpu.py runs the kernels on them."""
import numpy as np

from chain_ref import options

MAX_GAP = 5000          # the default -g


def anc(rev, rid, pos, qpos, span=15, flags=0):
    """one anchor: x = strand << 63 | target << 32 | target position, y = flags << 40 | seed length << 32 | read position"""
    assert 0 <= pos < 1 << 31 and 0 <= qpos < 1 << 31 and 0 < span < 256 and 0 <= rid < 1 << 31
    return (rev << 63 | rid << 32 | pos, flags << 40 | span << 32 | qpos)


def read(anchors):
    """anchors as the anchor sort leaves them: ascending x, then y"""
    return np.array(sorted(anchors), dtype=np.uint64).reshape(-1, 2)


def run(pos, q, n, step=20, span=15, rev=0, rid=0):
    return [anc(rev, rid, pos + step * k, q + step * k, span) for k in range(n)]


class Case:
    """a batch: reads (uint64 [n, 2] each) chained with one option set"""

    def __init__(self, name, reads, **opt):
        self.name, self.reads, self.opt = name, reads, options(**opt)

    def arrays(self):
        off = np.zeros(len(self.reads) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(r) for r in self.reads])
        return off, (np.concatenate(self.reads) if self.reads else np.zeros((0, 2), dtype=np.uint64)).reshape(-1, 2)


def diag():
    return [Case('diag', [read(run(1000, 100, 300))])]


def grid():
    """a tandem repeat: every read position of the repeat hits every copy.  On the exact lattice the diagonals win whatever the
    options are: every variant returns the default's 75 chains, so these cases walk the paths (walks broken by the skip counter,
    tiles beyond the ring, the iteration cut on each side of the tile and ring edges) without telling a wrong cut from a right one.
    The chains of the jittered lattice (jittered_grid) and of iter_edge do depend on the options."""
    r = read([anc(0, 0, 5000 + 37 * a + 3, 100 + 37 * b + 3) for a in range(40) for b in range(40)])
    out = [Case('grid', [r])]
    out += [Case('grid skip %d' % v, [r], max_chain_skip=v) for v in (0, 3)]
    out += [Case('grid iter %d' % v, [r], max_chain_iter=v) for v in (50, 63, 64, 65, 127, 128, 129)]
    return out + [Case('grid bw 40', [r], bw=40), Case('grid gap 100', [r], max_gap=100)]


def jittered_grid():
    """the lattice with the copies a few bases off their places: forks, ends that stop at taken anchors, and chains that change with
    max_chain_skip and max_chain_iter"""
    r = read([anc(0, 0, 5000 + 37 * a + 3 + (a * 7 + b * 3) % 11, 100 + 37 * b + 3 + (a * 5 + b) % 3) for a in range(40) for b in range(40)])
    return [Case('jittered', [r]), Case('jittered skip 0', [r], max_chain_skip=0), Case('jittered skip 3', [r], max_chain_skip=3),
            Case('jittered iter 50', [r], max_chain_iter=50)]


ITER_EDGES = (63, 64, 65, 127, 128, 129)


def iter_edge():
    """a run of ten, then N - 1 anchors that nothing can chain with (read positions below the run's, falling: dq <= 0, never scored,
    never a skip), then one anchor that continues the run: its only admissible predecessor is exactly N anchors back, at the edge of
    a tile of 64 or of the ring of 128.  With max_chain_iter N - 1 the run stays at ten anchors, with N and N + 1 it has eleven."""
    out = []
    for n in ITER_EDGES:
        a = run(1000, 2000, 10) + [anc(0, 0, 1000 + 20 * 9 + 1 + 10 * k, 1500 - 10 * k) for k in range(n - 1)]
        a.append(anc(0, 0, 1000 + 20 * 9 + 1500, 2000 + 20 * 9 + 1500))
        out += [Case('iter edge %d at %d' % (n, m), [read(a)], max_chain_iter=m) for m in (n - 1, n, n + 1)]
    return out


WIDEST_GAP = 66076418   # the largest max_gap the chain DP's 32-bit running coordinate holds


def widest_gap():
    """the largest max_gap: 70 lone anchors on 70 targets take the running coordinate past 2^32 (each step counts max_gap + 1), then
    60 anchors 30 000 000 apart on target and read chain, two steps within max_gap, three beyond it; then steps of exactly max_gap"""
    a = [anc(0, k, 1000, 100) for k in range(70)]
    a += run(1000, 100, 60, step=30000000, rid=100)
    a += run(1000, 100, 30, step=WIDEST_GAP, rid=101) + run(1000, 100, 20, step=20, rid=102)
    return [Case('widest gap', [read(a)], max_gap=WIDEST_GAP, bw=WIDEST_GAP)]


def peak():
    """30 colinear anchors, then three that each shift the diagonal by the whole band width: the tail's score falls below the peak"""
    a = run(1000, 100, 30)
    pos, q = a[-1][0], 100 + 20 * 29
    for _ in range(3):
        pos, q = pos + 20 + 500, q + 20
        a.append(anc(0, 0, pos, q))
    return [Case('peak', [read(a)])]


def trunk(n_b=0, with_c=False):
    """a colinear trunk of 40 + 10 anchors (steps of 100); branch B leaves anchor 20 on a diagonal 185 off with read positions below
    those of trunk anchor 21, so that nothing but anchor 20 can precede it; C: two anchors with seeds of 200 at another locus, D a
    branch off C's first anchor"""
    a = run(10000, 1000, 50, step=100)
    a += [anc(0, 0, 10000 + 2000 + 185 + 14 * k, 1000 + 2000 + 14 * k) for k in range(1, n_b + 1)]
    if with_c:
        a += [anc(0, 0, 50000, 5000, 200), anc(0, 0, 50300, 5300, 200)]
        a += [anc(0, 0, 50000 + 185 + 14 * k, 5000 + 14 * k) for k in range(1, 7)]
    return read(a)


def trunk_and_branches():
    return [Case('trunk', [trunk(4), trunk(6), trunk(0, True), trunk(4, True)])]


RANDOM_SETS = 12


def random_small():
    """jittered diagonals that cross, fork and overlap; one option set per batch of 200 reads"""
    out = []
    for s in range(RANDOM_SETS):
        rng = np.random.default_rng(1000 + s)
        opt = dict(min_cnt=int(rng.integers(1, 6)), min_chain_score=int(rng.choice([10, 25, 40, 80])), max_chain_skip=int(rng.choice([0, 1, 3, 25])),
                   bw=int(rng.choice([20, 100, 500])), max_chain_iter=int(rng.choice([5, 20, 5000])), max_gap=int(rng.choice([60, 300, 5000])))
        reads = []
        for _ in range(200):
            rev, rid, a = int(rng.integers(0, 2)), int(rng.integers(0, 3)), []
            for _ in range(int(rng.integers(2, 6))):
                n, step, off, start = int(rng.integers(3, 41)), int(rng.integers(8, 41)), int(rng.integers(-300, 301)), int(rng.integers(0, 600))
                for k in range(n):
                    q = 500 + start + k * step + int(rng.integers(-2, 3))
                    a.append(anc(rev, rid, 10000 + start + k * step + off + int(rng.integers(-3, 4)), q, int(rng.choice([11, 15, 19]))))
            reads.append(read(a))
        out.append(Case('random %d' % s, reads, **opt))
    return out


def many_ends():
    """600 loci of three anchors (every fourth of four), all of one shape: equal scores, so the order of the ends falls to the index"""
    a = []
    for s in range(600):
        a += run(20000 * s + 1000, 100, 4 if s % 4 == 3 else 3)
    r = read(a)
    return [Case('many ends', [r]), Case('many ends 46', [r], min_chain_score=46)]


def big_segment():
    """one segment above CHAIN_BIG whose 700 chain ends all but one stop at a taken anchor; and the same on two diagonals"""
    one = read([anc(0, 0, 1000 + 7 * i + i % 3, 100 + 7 * i + i % 2) for i in range(4200)])
    two = read([anc(0, 0, 1000 + 7 * i + 300 * (i % 2), 100 + 7 * i) for i in range(4200)])
    return [Case('big segment', [one, two])]


def compaction_read(phase, n_seg=1500, sizes=(2, 3, 4), gap=MAX_GAP):
    a, pos = [], 1000
    for s in range(n_seg):
        size = sizes[(s + phase) % len(sizes)]
        for k in range(size):
            a.append(anc(0, 0, pos, 100 + 20 * k))
            # one step inside a segment is exactly max_gap; the segments are max_gap + 1 and max_gap + 2 apart in turn
            pos += (gap if s == 7 and k == 0 else 20) if k < size - 1 else gap + 1 + s % 2
    return read(a)


def compaction():
    reads = [compaction_read(p) for p in range(3)]
    out = [Case('compaction min_cnt %d' % m, reads, min_cnt=m) for m in (1, 2, 3, 4, 5)]
    # (with the default min_chain_score a chain of two anchors never survives: the segments min_cnt 1 and 2 keep show at 10)
    out += [Case('compaction min_cnt %d score 10' % m, reads, min_cnt=m, min_chain_score=10) for m in (1, 2)]
    small = [compaction_read(p, 8, (63, 64, 65, 100)) for p in range(4)]
    return out + [Case('compaction saturated %d' % m, small, min_cnt=m) for m in (64, 65, 100)]


def picture(rev, rid, pos, flag_seed):
    """a run with a fork, placed anywhere; bits 40 and up of y carry arbitrary flags"""
    rng = np.random.default_rng(flag_seed)
    a = run(pos, 200, 12, rev=rev, rid=rid) + run(pos + 120 + 60, 200 + 120, 8, rev=rev, rid=rid, span=19)
    return [(x, y | int(rng.integers(1, 1 << 24)) << 40) for x, y in a]


def targets_and_strands():
    top = (1 << 31) - 1
    a = []
    for s, (rev, rid, pos) in enumerate(((0, 0, 1000), (1, 0, 1000), (0, 5, 700), (1, 5, 90000), (0, 70000, top - 700), (1, (1 << 31) - 1, top - 700),
                                         (0, 3, top - 12 * 20 - 400))):
        a += picture(rev, rid, pos, 50 + s)
    return [Case('targets and strands', [read(a), read(picture(1, 9, top - 700, 7))])]


def gap_read(spans, seg_len=2):
    """501 isolated segments: a colinear run, then one anchor 0..500 off its diagonal, to either side in turn, and (for runs longer
    than one anchor) as long a run on the new diagonal, so that the chain goes on whatever the step cost"""
    a, k = [], 0
    for d in range(501):
        pos, q = 1000 + 6000 * d, 1000
        for _ in range(seg_len - 1):
            a.append(anc(0, 0, pos, q, spans[k % len(spans)]))
            pos, q, k = pos + 40, q + 40, k + 1
        pos, q = pos + (d if d % 2 else 0), q + (0 if d % 2 else d)
        for _ in range(max(1, seg_len - 1)):
            a.append(anc(0, 0, pos, q, spans[k % len(spans)]))
            pos, q, k = pos + 40, q + 40, k + 1
    return read(a)


def gap_cost():
    reads = [gap_read((15, 19)), gap_read((15, 15, 19)), gap_read((15, 19, 19, 19)), gap_read((15, 15, 19), seg_len=8)]
    return [Case('gap cost', reads, min_cnt=1, min_chain_score=1)]


def edges():
    reads = [read(run(1000, 100, n)) for n in (0, 1, 2, 63, 64, 65, 127, 128, 129)]
    reads.append(read(run(1000, 100, 10) + [anc(0, 0, 1000 + 20 * k, 130 + 20 * k) for k in range(10)]))      # equal x, other y
    reads.append(read(run(1000, 100, 10) + [anc(0, 0, 1030 + 20 * k, 100 + 20 * k) for k in range(10)]))      # equal read positions
    reads.append(read([anc(k % 2, k, 1000 + 9000 * k, 100 + 50 * k) for k in range(70)]))                     # strays only
    return [Case('edges', reads), Case('edges min_cnt 1', reads, min_cnt=1, min_chain_score=10)]


def far_peak():
    """a run of 30, then 140 anchors that neither chain with it nor with each other (read positions beyond max_gap, falling), then one
    anchor that chains to the run's last, 141 anchors back, at a step that costs more than it gains: its peak score is that of an
    anchor which has left the 128-anchor ring; and the same with a step that pays and a run behind it"""
    a = run(1000, 100, 30)
    a += [anc(0, 0, 1000 + 20 * 29 + 1 + 10 * k, 100 + 20 * 29 + 8000 - 10 * k) for k in range(140)]
    costly = a + [anc(0, 0, 1000 + 20 * 29 + 1500, 100 + 20 * 29 + 1100)]
    # the same with a step that pays: the chain goes on through a predecessor that is read from global memory, not from the ring
    cheap = a + [anc(0, 0, 1000 + 20 * 29 + 1500, 100 + 20 * 29 + 1450)] + run(1000 + 20 * 29 + 1520, 100 + 20 * 29 + 1470, 5)
    return [Case('far peak', [read(costly), read(cheap)])]


def strays():
    """a run whose diagonal shifts by 300 half way, among 20 lone anchors with seeds of 255 that the compaction drops: the average seed
    length is taken over all 40 anchors (135), and at that the shift costs too much to chain across"""
    shifted = run(1000, 100, 10) + run(1000 + 200 + 300, 100 + 200, 10)
    lone = [anc(0, 1, 1000 + 9000 * k, 100, 255) for k in range(20)]
    return [Case('strays', [read(shifted + lone), read(shifted)])]


def exact_gap():
    """steps of exactly max_gap on target and read: the anchors to either side are in one segment and chain (the next larger step
    starts a segment): two pairs that only together make min_cnt, and 260 + 10 anchors, more than a work item before the step"""
    pairs = run(1000, 100, 2) + run(1020 + MAX_GAP, 120 + MAX_GAP, 2) + run(40000, 100, 2) + run(40020 + MAX_GAP + 1, 120 + MAX_GAP, 2)
    long_ = run(1000, 100, 260, step=10) + run(1000 + 2590 + MAX_GAP, 100 + 2590 + MAX_GAP, 10, step=10)
    return [Case('exact gap', [read(pairs), read(long_)])]


BUILDERS = {'diag': diag, 'grid': grid, 'jittered-grid': jittered_grid, 'iter-edge': iter_edge, 'widest-gap': widest_gap, 'peak': peak, 'trunk-and-branches': trunk_and_branches, 'random-small': random_small,
            'many-ends': many_ends, 'big-segment': big_segment, 'compaction': compaction, 'targets-and-strands': targets_and_strands,
            'gap-cost': gap_cost, 'edges': edges, 'far-peak': far_peak, 'strays': strays, 'exact-gap': exact_gap}
FAMILIES = tuple(BUILDERS)


def families():
    return {name: build() for name, build in BUILDERS.items()}
