"""Cases and brute-force statements shared by tests/test_bed_select.py (CPU) and tests/test_bed_select_gpu.py."""
import numpy as np


def random_small_case(rng):
    """1-4 keys in 1-3 groups, 0-25 BED intervals and 0-12 queries with coordinates <= 60: touching, nested, duplicate and empty
    or reversed BED intervals are common, and so are queries that are empty, end on an interval's edge or lie in a gap."""
    n_keys = int(rng.integers(1, 5))
    n_groups = int(rng.integers(1, 4))
    key_group = rng.integers(0, n_groups, size=n_keys).astype(np.int32)
    n = int(rng.integers(0, 26))
    key = rng.integers(0, n_keys, size=n).astype(np.int32)
    start = rng.integers(0, 56, size=n).astype(np.int64)
    end = np.clip(start + rng.integers(-2, 12, size=n), 0, 60)
    if n > 2 and rng.random() < 0.5:                                # a duplicate and a book-end of an earlier interval
        key[-1], start[-1], end[-1] = key[0], start[0], end[0]
        key[-2], start[-2], end[-2] = key[1], end[1], min(int(end[1]) + 5, 60)
    n_q = int(rng.integers(0, 13))
    q_key = rng.integers(0, n_keys, size=n_q).astype(np.int32)
    q_start = rng.integers(0, 58, size=n_q).astype(np.int64)
    q_end = np.minimum(q_start + rng.integers(0, 30, size=n_q), 60)
    return dict(bed=dict(key=key, start=start, end=end, n_keys=n_keys, key_group=key_group, n_groups=n_groups),
                query=dict(q_key=q_key, q_start=q_start, q_end=q_end))


def brute_force(bed, query, top=64):
    """A flag per position and key; merged intervals, span per group and covered positions per query read off it with loops."""
    mark = np.zeros((bed['n_keys'], top + 1), dtype=bool)          # mark[:, top] stays False and closes the last run
    for k, s, e in zip(bed['key'], bed['start'], bed['end']):
        mark[int(k), int(s):max(int(e), int(s))] = True
    merged, span = [], [0] * bed['n_groups']
    for k in range(bed['n_keys']):
        run_from = None
        for p in range(top + 1):
            if mark[k, p] and run_from is None:
                run_from = p
            if not mark[k, p] and run_from is not None:
                merged.append((k, run_from, p))
                span[int(bed['key_group'][k])] += p - run_from
                run_from = None
    covered = [int(mark[int(k), int(s):int(e)].sum()) for k, s, e in zip(query['q_key'], query['q_start'], query['q_end'])]
    return merged, span, covered


def union_as_lists(result):
    (ok, os_, oe), span = result
    return [tuple(int(v) for v in t) for t in zip(ok, os_, oe)], [int(v) for v in span]


def same_union(a, b):
    """two ((key, start, end), span) results equal as arrays: values, lengths, order and integer widths"""
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(list(a[0]) + [a[1]], list(b[0]) + [b[1]]))


def fraction_text(c, length):
    """what `bedtools annotate` prints for c covered of `length` positions: the float32 quotient with six decimals"""
    if length == 0:
        return 'nan'
    return '%f' % float(np.float32(c) / np.float32(length))


def passes(c, length, max_overlap=100, can_equal_to_max=True, min_overlap=0, can_equal_to_min=True):
    """select_alignment_by_bed's decision for one row (megapath_nano.py:708-711), through the text as pandas reads it back"""
    x = float(fraction_text(c, length))
    hi, lo = max_overlap / 100, min_overlap / 100
    return (x <= hi if can_equal_to_max else x < hi) and (x >= lo if can_equal_to_min else x > lo)
