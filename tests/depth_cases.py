"""Cases and brute-force statements shared by tests/test_depth_bed.py (CPU) and tests/test_depth_bed_gpu.py."""
import numpy as np
import pandas as pd


def random_small_case(rng):
    """1-4 keys of length 1-80 in 1-3 groups, 0-30 intervals: empty and reversed ones, ones that start at or beyond the length,
    ones that cross it; a depth range per group (sometimes empty, sometimes none at all)."""
    n_keys = int(rng.integers(1, 5))
    n_groups = int(rng.integers(1, 4))
    key_len = rng.integers(1, 81, size=n_keys).astype(np.int64)
    key_group = rng.integers(0, n_groups, size=n_keys).astype(np.int32)
    n = int(rng.integers(0, 31))
    key = rng.integers(0, n_keys, size=n).astype(np.int32)
    start = rng.integers(0, 100, size=n).astype(np.int64)
    end = start + rng.integers(-3, 40, size=n)
    end = np.maximum(end, 0)
    at_len = rng.random(n) < 0.15                                  # starts exactly at the length, ends exactly at the length
    start = np.where(at_len & (rng.random(n) < 0.5), key_len[key], start)
    end = np.where(at_len, key_len[key] + rng.integers(0, 2, size=n) * 7, end)
    if rng.random() < 0.25:
        lo = hi = None
    else:
        lo = rng.integers(0, 4, size=n_groups).astype(np.int32)
        hi = (lo + rng.integers(-1, 4, size=n_groups)).astype(np.int32)
    return dict(key=key, start=start, end=end, key_len=key_len, key_group=key_group, n_groups=n_groups, depth_lo=lo, depth_hi=hi)


def brute_force(key, start, end, key_len, key_group, n_groups, depth_lo=None, depth_hi=None):
    """A counter per position; rows, BED and span read off it with plain loops."""
    rows, bed, span = [], [], np.zeros(n_groups, dtype=np.int64)
    for k in range(len(key_len)):
        L = int(key_len[k])
        count = [0] * (L + 1)                                      # count[L] = 0 closes the last run
        for i in np.flatnonzero(np.asarray(key) == k):
            for p in range(int(start[i]), min(int(end[i]), L)):
                count[p] += 1
        g = int(key_group[k])
        run_from = 0
        for p in range(1, L + 1):
            if count[p] != count[p - 1]:
                if count[p - 1] > 0:
                    rows.append((k, run_from, p, count[p - 1]))
                run_from = p
        ok = [c > 0 and (depth_lo is None or depth_lo[g] <= c <= depth_hi[g]) for c in count]
        bed_from = None
        for p in range(L + 1):
            if ok[p] and bed_from is None:
                bed_from = p
            if not ok[p] and bed_from is not None:
                bed.append((k, bed_from, p))
                span[g] += p - bed_from
                bed_from = None
    return rows, bed, span


def as_lists(result):
    (rk, rs, re, rd), (bk, bs, be), span = result
    return ([tuple(int(v) for v in t) for t in zip(rk, rs, re, rd)], [tuple(int(v) for v in t) for t in zip(bk, bs, be)],
            [int(v) for v in span])


def same_result(a, b):
    """two (profile, bed, span) results equal as arrays: values, lengths, order and integer widths"""
    flat_a, flat_b = list(a[0]) + list(a[1]) + [a[2]], list(b[0]) + list(b[1]) + [b[2]]
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(flat_a, flat_b))


def read_table(seed=9, n_reads=400):
    """An alignment table of about n_reads reads over 3 assemblies x 2 sequences with a pile-up on A1_c1, and the assembly
    lengths: what the spike tests run on."""
    rng = np.random.default_rng(seed)
    seq_len = {'A1_c1': 9000, 'A1_c2': 7000, 'A2_c1': 9000, 'A2_c2': 8000, 'A3_c1': 9500, 'A3_c2': 6000}
    rows = []
    for r in range(n_reads):
        for _ in range(int(rng.integers(1, 4))):
            a = str(rng.choice(['A1', 'A2', 'A3']))
            s = a + str(rng.choice(['_c1', '_c2']))
            s0 = int(rng.integers(0, seq_len[s] - 200))
            if s == 'A1_c1' and rng.random() < 0.6:
                s0 = int(rng.integers(3000, 3300))                 # the spike
            e0 = min(s0 + int(rng.integers(1, 3000)), seq_len[s])
            rows.append((f'r{r}', 5000, a, s, seq_len[s], s0, e0, max(1, (e0 - s0) // 2), 5, int(rng.integers(100, 900)), float(rng.random())))
    al = pd.DataFrame(rows, columns=['read_id', 'read_length', 'assembly_id', 'sequence_id', 'sequence_length', 'sequence_from', 'sequence_to',
                                     'match', 'edit_dist', 'alignment_score', 'alignment_score_tiebreaker'])
    lens = pd.DataFrame({'assembly_id': ['A1', 'A2', 'A3'], 'assembly_length': [16000, 17000, 15500]})
    return al, lens
