"""Cases for the read split (include/mpn_reads.h): the smallest shapes at which the plan or the gather can still go wrong.
A case: dict(name, buf, qbuf or None, off, lens, mem_read, mem_group, n_groups); the source buffer is packed like pack_seqs packs
it, except where a case says otherwise.  restate() is the plain loop over dicts the numpy statement is checked against;
expected() is the numpy statement, computed once per case and shared (treat it as read-only)."""
import functools

import numpy as np

# around every power of two the gather cares about: its 16-byte slots, its 1 KiB wave chunks, and a few pages
LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]
LONG = [70000, 300000]      # reads that span many wave chunks (and, the second, more chunks than one block's waves take in one round)


def _pack(rng, lens, quals, pad=16):
    lens = np.asarray(lens, dtype=np.int32)
    off = np.zeros(len(lens), dtype=np.int64)
    if len(lens) > 1:
        off[1:] = np.cumsum(lens[:-1].astype(np.int64))
    total = int(lens.astype(np.int64).sum())
    buf = np.zeros(total + pad, dtype=np.uint8)
    buf[:total] = rng.choice(np.frombuffer(b'ACGTN', dtype=np.uint8), size=total, p=[.24, .24, .24, .24, .04])
    qbuf = None
    if quals:
        qbuf = np.zeros(total + pad, dtype=np.uint8)
        qbuf[:total] = rng.integers(33, 91, size=total, dtype=np.uint8)
    return buf, qbuf, off, lens


def _case(name, rng, lens, pairs, n_groups, quals, pad=16):
    buf, qbuf, off, lens = _pack(rng, lens, quals, pad)
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    return dict(name=name, buf=buf, qbuf=qbuf, off=off, lens=lens, mem_read=np.ascontiguousarray(pairs[:, 0]),
                mem_group=np.ascontiguousarray(pairs[:, 1]), n_groups=n_groups)


@functools.lru_cache(maxsize=None)
def make_cases():
    rng = np.random.default_rng(20241018)
    cases = []
    every = LENGTHS + LONG
    n = len(every)
    # all reads in one group, in reverse pair order, with qualities
    cases.append(_case('one_group_all_lengths_q', rng, every, [(r, 0) for r in reversed(range(n))], 1, True))
    # two groups that overlap, pairs shuffled, every pair of group 1 given twice; the order of the lengths is shuffled too so that
    # the boundaries fall elsewhere than in the case above
    order = rng.permutation(n)
    pairs = [(r, 0) for r in range(n) if r % 3 != 1] + [(r, 1) for r in range(n) if r % 2] * 2
    cases.append(_case('two_groups_shuffled_dups', rng, [every[i] for i in order], [pairs[i] for i in rng.permutation(len(pairs))], 2, False))
    # 1000 groups, most of them empty: the first, the last and a few in between
    where = [0, 7, 8, 500, 999]
    cases.append(_case('thousand_groups_sparse_q', rng, every, [(r, where[r % len(where)]) for r in range(n)] + [(n - 1, 0), (0, 999)], 1000, True))
    # every read in every group, 8 x 8, reads of 32..88 bytes (each holds a whole 16-byte slot), read-major pairs (the wrong order)
    cases.append(_case('all_in_all_8x8', rng, [32 + 8 * r for r in range(8)], [(r, g) for r in range(8) for g in range(8)], 8, True))
    # no read in any group; no pairs at all; no reads at all
    cases.append(_case('no_pairs', rng, LENGTHS, [], 3, True))
    cases.append(_case('no_reads', rng, [], [], 3, False))
    cases.append(_case('no_reads_no_groups', rng, [], [], 0, False))
    # the last read ends exactly at the end of the source buffer (no padding behind it) and is copied from an odd offset
    cases.append(_case('source_ends_with_last_read', rng, [5, 77, 1025, 4097], [(3, 0), (1, 1), (3, 1), (0, 1)], 2, True, pad=0))
    # many short reads of 17..80 bytes over 5 groups: every residue mod 16 on either side, every relative shift
    lens = rng.integers(17, 81, size=400)
    cases.append(_case('residues', rng, lens, [(r, int(g)) for r, g in zip(range(400), rng.integers(0, 5, size=400))] +
                       [(r, 4) for r in range(0, 400, 7)], 5, False))
    # group sizes that are multiples of 16 (no padding needed at the boundary) next to ones that are not; runs of empty reads at a
    # boundary and inside a slot
    cases.append(_case('boundaries', rng, [16, 48, 0, 0, 0, 15, 0, 1, 64, 0], [(0, 0), (1, 0), (2, 0), (3, 1), (4, 1), (5, 1), (6, 1), (7, 1), (8, 2), (9, 3),
                                                                                    (2, 3), (5, 4), (8, 4)], 6, True))
    # more output than one round of the gather's grid takes (2048 blocks x 4 waves x 1 KiB = 8 MiB): the grid-stride step
    cases.append(_case('second_grid_round', rng, [262144 + 37 * r for r in range(40)], [(r, r % 2) for r in range(40)], 2, False))
    return tuple(cases)


def restate(case):
    """nanosplit's semantics as a loop over dicts -> the arrays host_split_reads returns"""
    lens, off = case['lens'], case['off']
    members = {g: set() for g in range(case['n_groups'])}
    for r, g in zip(case['mem_read'].tolist(), case['mem_group'].tolist()):
        members[g].add(r)                                           # a set: a pair given twice counts once
    out_read, out_off, group_first, group_byte, placed = [], [], [], [], []
    pos = 0
    for g in range(case['n_groups']):
        pos = -(-pos // 16) * 16                                    # every group's block starts at a multiple of 16
        group_first.append(len(out_read))
        group_byte.append(pos)
        for r in sorted(members[g]):                                # input order inside a group
            out_read.append(r)
            out_off.append(pos)
            placed.append((pos, int(off[r]), int(lens[r])))
            pos += int(lens[r])
    pos = -(-pos // 16) * 16
    group_first.append(len(out_read))
    group_byte.append(pos)
    out_bytes = pos + 16                                            # 4 readable bytes behind the last base, a multiple of 16
    outs = []
    for src in (case['buf'], case['qbuf']):
        if src is None:
            outs.append(None)
            continue
        o = np.zeros(out_bytes, dtype=np.uint8)
        for d, s, l in placed:
            o[d:d + l] = src[s:s + l]
        outs.append(o)
    return dict(n_out=len(out_read), out_read=np.array(out_read, dtype=np.int32), group_first=np.array(group_first, dtype=np.int64),
                out_off=np.array(out_off, dtype=np.int64), group_byte=np.array(group_byte, dtype=np.int64), out_bytes=out_bytes,
                seqs=outs[0], quals=outs[1])


@functools.lru_cache(maxsize=None)
def expected(i):
    """host_split_reads of case i"""
    from megapath_nano_amd import mapper
    c = make_cases()[i]
    return mapper.host_split_reads(c['buf'], c['off'], c['lens'], c['mem_read'], c['mem_group'], c['n_groups'], c['qbuf'])


def assert_same(got, want, what):
    for k in ('n_out', 'out_bytes'):
        assert int(got[k]) == int(want[k]), (what, k, got[k], want[k])
    for k in ('out_read', 'group_first', 'out_off', 'group_byte', 'seqs', 'quals'):
        if want[k] is None:
            assert got[k] is None, (what, k)
            continue
        assert got[k] is not None and got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape if got[k] is not None else None, want[k].shape)
        bad = np.flatnonzero(np.asarray(got[k]) != np.asarray(want[k]))
        assert len(bad) == 0, (what, k, 'first difference at', int(bad[0]), int(got[k][bad[0]]), int(want[k][bad[0]]), len(bad), 'differ')
