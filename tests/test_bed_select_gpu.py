"""GPU tests (-m gpu) of mpn_bed_union and mpn_cover_by_bed (include/mpn_abundance.h; csrc/interval_kernels.hip): the merged
intervals, the span per group and the covered positions per query must equal the numpy statements as arrays, order included, and
a flag per position -- on random small cases, on tiny inputs in every relation of one interval to one query, at interval counts
around the multiples of the sweep's tile, with one key through hundreds of tiles beside many small ones, at the top of the
coordinate domain -- and the mirrors of the reference's select_alignment_by_bed, merge_bed_with_assembly_id, step_noise_removal
and step_closing_spike_filter must equal their host forms."""
import ctypes as ct

import numpy as np
import pandas as pd
import pytest

from bed_cases import brute_force, random_small_case, same_union, union_as_lists
from depth_cases import read_table

pytestmark = pytest.mark.gpu


def _brief(arg):
    return {k: (v if np.ndim(v) == 0 or len(v) < 40 else f'[{len(v)}]') for k, v in arg.items()}


def _both(**arg):
    from megapath_nano_amd.abundance import device_bed_union, host_bed_union
    dev, host = device_bed_union(**arg), host_bed_union(**arg)
    assert same_union(dev, host), _brief(arg)
    return dev


def _both_cover(**arg):
    from megapath_nano_amd.abundance import device_cover_by_bed, host_cover_by_bed
    dev, host = device_cover_by_bed(**arg), host_cover_by_bed(**arg)
    assert dev.dtype == host.dtype and np.array_equal(dev, host), _brief(arg)
    return dev


def _cover_arg(bed, query):
    return dict(bed_key=bed['key'], bed_start=bed['start'], bed_end=bed['end'], n_keys=bed['n_keys'], **query)


def test_device_equals_host_equals_brute_force_on_small_cases(libmpn):
    rng = np.random.default_rng(41)
    for trial in range(150):
        c = random_small_case(rng)
        want_merged, want_span, want_covered = brute_force(c['bed'], c['query'])
        merged, span = union_as_lists(_both(**c['bed']))
        assert merged == want_merged and span == want_span, trial
        assert _both_cover(**_cover_arg(c['bed'], c['query'])).tolist() == want_covered, trial


def test_tiny_inputs_and_every_relation_of_one_interval_to_one_query(libmpn):
    q3 = dict(q_key=[0, 0, 1], q_start=[0, 5, 0], q_end=[10, 5, 7])
    assert _both_cover(bed_key=[], bed_start=[], bed_end=[], n_keys=2, **q3).tolist() == [0, 0, 0]          # n_bed = 0
    assert _both_cover(bed_key=[0], bed_start=[4], bed_end=[4], n_keys=2, **q3).tolist() == [0, 0, 0]       # only an empty interval
    assert len(_both_cover(bed_key=[0], bed_start=[4], bed_end=[9], n_keys=2, q_key=[], q_start=[], q_end=[])) == 0      # n_q = 0
    assert union_as_lists(_both(key=[], start=[], end=[], n_keys=1)) == ([], [0])
    assert union_as_lists(_both(key=[0], start=[9], end=[2], n_keys=1)) == ([], [0])
    assert union_as_lists(_both(key=[0], start=[3], end=[8], n_keys=1)) == ([(0, 3, 8)], [5])
    # the BED interval [20, 30) and one query
    relations = {'disjoint left': (5, 15, 0), 'disjoint right': (35, 40, 0), 'touching left': (10, 20, 0), 'touching right': (30, 40, 0),
                 'query inside': (22, 27, 5), 'interval inside': (10, 40, 10), 'identical': (20, 30, 10), 'over the left edge': (15, 21, 1),
                 'over the right edge': (29, 33, 1), 'empty query inside': (25, 25, 0)}
    for name, (s, e, want) in relations.items():
        assert _both_cover(bed_key=[0], bed_start=[20], bed_end=[30], n_keys=1, q_key=[0], q_start=[s], q_end=[e]).tolist() == [want], name
    together = list(relations.values())
    got = _both_cover(bed_key=[1], bed_start=[20], bed_end=[30], n_keys=3, q_key=[1] * len(together), q_start=[t[0] for t in together], q_end=[t[1] for t in together])
    assert got.tolist() == [t[2] for t in together]


def _sizes():
    from megapath_nano_amd.abundance import BED_TILE
    return sorted({t * BED_TILE + d for t in (1, 2, 3, 5) for d in (-1, 0, 1)})


def test_interval_counts_around_the_tile_boundaries(libmpn):
    rng = np.random.default_rng(42)
    for n in _sizes():
        key = np.zeros(n, dtype=np.int32)
        one = dict(n_keys=1)
        # (a) random intervals on one key: about half of them merge with a neighbour
        start = rng.integers(0, 60 * n, size=n)
        end = start + rng.integers(0, 60, size=n)
        (mk, ms, me), span = _both(key=key, start=start, end=end, **one)
        assert n // 4 < len(mk) < n and span[0] == (me - ms).sum()
        qs = rng.integers(0, 60 * n, size=500)
        qe = qs + rng.integers(0, 3000, size=500)
        _both_cover(bed_key=key, bed_start=start, bed_end=end, n_keys=1, q_key=np.zeros(500, np.int32), q_start=qs, q_end=qe)
        # (b) a chain of book-ended intervals, in random order: exactly one merged row
        chain = 10 * rng.permutation(n)
        assert union_as_lists(_both(key=key, start=chain, end=chain + 10, **one)) == ([(0, 0, 10 * n)], [10 * n])
        got = _both_cover(bed_key=key, bed_start=chain, bed_end=chain + 10, n_keys=1, q_key=[0, 0, 0], q_start=[0, 5, 10 * n], q_end=[10 * n, 10 * n + 50, 10 * n + 9])
        assert got.tolist() == [10 * n, 10 * n - 5, 0]
        # (c) disjoint intervals with gaps of one position: nothing merges
        s = 10 * np.arange(n)
        (mk, ms, me), span = _both(key=key, start=s, end=s + 9, **one)
        assert len(mk) == n and np.array_equal(ms, s) and np.array_equal(me, s + 9) and span.tolist() == [9 * n]
        # queries that end exactly on merged starts and ends, and queries wholly in a gap
        j = rng.integers(0, n - 1, size=400)
        q_start = np.concatenate([s[j] + 9, s[j], s[j] + 9, s[j] + 4, [0]])
        q_end = np.concatenate([s[j] + 10, s[j + 1], s[j + 1] + 9, s[j + 1] + 4, [10 * n]])
        got = _both_cover(bed_key=key, bed_start=s, bed_end=s + 9, n_keys=1, q_key=np.zeros(len(q_start), np.int32), q_start=q_start, q_end=q_end)
        assert got.tolist() == [0] * 400 + [9] * 400 + [9] * 400 + [9] * 400 + [9 * n]
        # (d) one interval over everything and n - 1 nested in it, the wide one last in the input
        s = rng.integers(1, 10 * n, size=n)
        e = s + rng.integers(0, 50, size=n)
        s[-1], e[-1] = 0, 10 * n + 60
        assert union_as_lists(_both(key=key, start=s, end=e, **one)) == ([(0, 0, 10 * n + 60)], [10 * n + 60])
        # ... and the same with every interval on its own key, where nothing may be carried from key to key
        (mk, ms, me), span = _both(key=np.arange(n, dtype=np.int32)[::-1], start=s, end=e, n_keys=n, key_group=np.arange(n) % 3, n_groups=3)
        assert len(mk) == int((s < e).sum()) and np.array_equal(mk, np.sort(mk)) and span.sum() == (e - s).sum()


def test_many_small_keys_beside_one_that_holds_half_of_the_intervals(libmpn):
    """600 000 BED intervals, 300 000 keys, 2000 groups, 600 000 queries: every tile holds hundreds of key changes, and one key
    runs through hundreds of tiles"""
    rng = np.random.default_rng(43)
    n, n_groups, small, n_q = 600000, 2000, 300000, 600000
    n_keys = small + 1
    # BED rows only on the big key and on keys up to 200 000; queries only on the big key and on keys from 100 000 up
    key = np.where(rng.random(n) < 0.5, 0, rng.integers(1, 200001, size=n)).astype(np.int32)
    key_group = np.concatenate([[0], rng.integers(1, n_groups, size=small)]).astype(np.int32)
    reach = np.where(key == 0, 50_000_000, 20000)
    start = (rng.random(n) * reach).astype(np.int64)
    end = start + rng.integers(-5, 400, size=n)
    (mk, ms, me), span = _both(key=key, start=start, end=end, n_keys=n_keys, key_group=key_group, n_groups=n_groups)
    assert n // 2 < len(mk) < n and (span > 0).all() and np.array_equal(span, np.bincount(key_group[mk], weights=(me - ms), minlength=n_groups).astype(np.int64))
    q_key = np.where(rng.random(n_q) < 0.5, 0, rng.integers(100000, n_keys, size=n_q)).astype(np.int32)
    q_reach = np.where(q_key == 0, 50_000_000, 20000)
    q_start = (rng.random(n_q) * q_reach).astype(np.int64)
    q_end = q_start + rng.integers(0, 3000, size=n_q)
    has_bed, has_query = np.zeros(n_keys, dtype=bool), np.zeros(n_keys, dtype=bool)
    has_bed[mk], has_query[q_key] = True, True
    assert (has_bed & ~has_query).sum() > 1000 and (has_query & ~has_bed).sum() > 1000 and (has_bed & has_query).sum() > 1000
    covered = _both_cover(bed_key=key, bed_start=start, bed_end=end, n_keys=n_keys, q_key=q_key, q_start=q_start, q_end=q_end)
    assert (covered[~has_bed[q_key]] == 0).all() and (covered <= q_end - q_start).all()
    assert (covered > 0).sum() > n_q // 4 and (covered == q_end - q_start).sum() > 100 and (covered[q_key == 0] > 0).sum() > 1000


def test_coordinates_at_the_top_of_the_domain(libmpn):
    top = 2 ** 32 - 1
    key, start, end = [0, 0, 0, 1, 1], [top - 10, top - 5, 0, top - 1, 0], [top, top, 7, top, top]
    merged, span = union_as_lists(_both(key=key, start=start, end=end, n_keys=2, key_group=[0, 1], n_groups=2))
    assert merged == [(0, 0, 7), (0, top - 10, top), (1, 0, top)] and span == [17, top]
    got = _both_cover(bed_key=key, bed_start=start, bed_end=end, n_keys=2, q_key=[0, 1, 0, 1, 0], q_start=[0, 0, top - 3, top, top - 10], q_end=[top, top, top, top, top - 9])
    assert got.tolist() == [17, top, 3, 0, 1]
    # the summed length before an interval passes 2^32 without harm
    n = 5000
    s = np.arange(n, dtype=np.int64) * 800000
    (mk, ms, me), span = _both(key=np.zeros(n, np.int32), start=s, end=s + 799999, n_keys=1)
    assert span.tolist() == [799999 * n]
    got = _both_cover(bed_key=np.zeros(n, np.int32), bed_start=s, bed_end=s + 799999, n_keys=1, q_key=[0, 0], q_start=[0, s[-2] + 5], q_end=[top, top])
    assert got.tolist() == [799999 * n, 2 * 799999 - 5]


def test_bad_arguments_return_minus_two_and_leave_the_outputs_untouched(libmpn):
    from megapath_nano_amd import _ffi, abundance
    lib = abundance._lib()
    key, start, end = np.array([0, 1, 0], np.int32), np.array([0, 5, 10], np.int64), np.array([10, 9, 30], np.int64)
    key_group = np.array([0, 1], np.int32)

    def union(key=key, start=start, cap=3, key_group=key_group):
        out_key, out64 = np.full(5, -7, np.int32), [np.full(5, -7, np.int64) for _ in range(3)]
        n_out = ct.c_int64(-7)
        rc = lib.mpn_bed_union(3, key.ctypes.data, start.ctypes.data, end.ctypes.data, 2, key_group.ctypes.data, 2, cap, out_key.ctypes.data,
                               out64[0].ctypes.data, out64[1].ctypes.data, ct.byref(n_out), out64[2].ctypes.data)
        untouched = (out_key == -7).all() and all((a == -7).all() for a in out64) and n_out.value == -7
        return rc, untouched, n_out.value, out64[2][:2].tolist()

    assert union() == (0, False, 2, [30, 4])                       # [0,10) and [10,30) on key 0 are book-ended: one row
    rc, untouched = union(cap=2)[:2]
    assert rc == -2 and untouched and 'cap' in _ffi.last_error()
    rc, untouched = union(key=np.array([0, 2, 0], np.int32))[:2]
    assert rc == -2 and untouched and 'record 1' in _ffi.last_error()
    rc, untouched = union(key=np.array([0, 1, -1], np.int32))[:2]
    assert rc == -2 and untouched and 'record 2' in _ffi.last_error()
    rc, untouched = union(start=np.array([0, 1 << 32, 0], np.int64))[:2]
    assert rc == -2 and untouched and 'record 1' in _ffi.last_error()
    rc, untouched = union(key_group=np.array([0, 2], np.int32))[:2]
    assert rc == -2 and untouched and 'key 1' in _ffi.last_error()

    q_key, q_start, q_end = np.array([1, 0], np.int32), np.array([0, 12], np.int64), np.array([7, 40], np.int64)

    def cover(key=key, start=start, q_key=q_key, q_start=q_start):
        covered = np.full(4, -7, np.int64)
        rc = lib.mpn_cover_by_bed(3, key.ctypes.data, start.ctypes.data, end.ctypes.data, 2, q_key.ctypes.data, q_start.ctypes.data, q_end.ctypes.data, 2,
                                  covered.ctypes.data)
        return rc, bool((covered == -7).all()), covered[:2].tolist()

    assert cover() == (0, False, [2, 18])
    rc, untouched = cover(key=np.array([0, 1, 2], np.int32))[:2]
    assert rc == -2 and untouched and 'record 2' in _ffi.last_error()
    rc, untouched = cover(start=np.array([1 << 32, 5, 10], np.int64))[:2]
    assert rc == -2 and untouched and 'record 0' in _ffi.last_error()
    rc, untouched = cover(q_key=np.array([1, 2], np.int32))[:2]
    assert rc == -2 and untouched and 'query 1' in _ffi.last_error()
    rc, untouched = cover(q_start=np.array([8, 12], np.int64))[:2]                  # start > end
    assert rc == -2 and untouched and 'query 0' in _ffi.last_error()
    rc, untouched = cover(q_start=np.array([0, 1 << 32], np.int64))[:2]
    assert rc == -2 and untouched and 'query 1' in _ffi.last_error()
    with pytest.raises(_ffi.MpnError):
        abundance.device_cover_by_bed([0], [0], [5], [0], [7], [3], 1)
    with pytest.raises(_ffi.MpnError):
        abundance.device_bed_union([0, 5], [0, 0], [1, 1], 1)


def test_mirrors_on_the_device_equal_their_host_forms(libmpn):
    from megapath_nano_amd.abundance import (align_list_to_depth_bed, closing_spike_filter, merge_bed_with_assembly_id, noise_removal,
                                             select_alignment_by_bed, spike_noise)
    al, lens = read_table()
    mn = pd.DataFrame({'assembly_id': ['A1', 'A2', 'A3'], 'min_depth': [40.0, 18.0, 18.0]})
    bed = align_list_to_depth_bed(align_list=al, min_depth=mn, device=False)[0]
    for kw in (dict(max_overlap=50), dict(max_overlap=50, can_equal_to_max=False), dict(min_overlap=50, can_equal_to_min=False), dict(min_overlap=30, max_overlap=60),
               dict(max_overlap=0), dict(min_overlap=100)):
        dev, host = select_alignment_by_bed(align_list=al, bed=bed, device=True, **kw), select_alignment_by_bed(align_list=al, bed=bed, device=False, **kw)
        pd.testing.assert_frame_equal(dev, host)
        assert 0 < len(dev) < len(al), kw
    pd.testing.assert_frame_equal(select_alignment_by_bed(align_list=al, bed=bed, max_overlap=50), select_alignment_by_bed(align_list=al, bed=bed, max_overlap=50, device=False))
    spike = spike_noise(al, lens, expected_max_depth_stdev=1, device=False)[0]
    bare = pd.DataFrame({'sequence_id': ['A1_c1', 'A1_c1'], 'start': [5, 9], 'end': [9, 30]})
    beds = [bed, spike, bare]
    dev, host = merge_bed_with_assembly_id(beds, device=True), merge_bed_with_assembly_id(beds, device=False)
    pd.testing.assert_frame_equal(dev, host)
    pd.testing.assert_frame_equal(merge_bed_with_assembly_id(beds), host)                       # None is the device
    assert 0 < len(dev) < len(bed) + len(spike) + len(bare)
    dev = noise_removal(align_list=al, noise_bed=bed, non_zero_assembly_ids=['A1', 'A3'], max_align_noise_overlap=20, device=True)
    host = noise_removal(align_list=al, noise_bed=bed, non_zero_assembly_ids=['A1', 'A3'], max_align_noise_overlap=20, device=False)
    pd.testing.assert_frame_equal(dev[0], host[0])
    assert dev[1:] == host[1:] and 0 < dev[2] < dev[1]
    with_short = al.sort_values(['read_id', 'alignment_score', 'alignment_score_tiebreaker']).drop_duplicates(subset=['read_id'], keep='last')
    best = with_short[(with_short['sequence_to'] - with_short['sequence_from']) >= 300]
    arg = dict(align_list=al[al['read_id'].isin(best['read_id'])], best_align_list=best, best_align_list_with_short_alignment=with_short, noise_bed=bed,
               assembly_length=lens, max_align_noise_overlap=30, expected_max_depth_stdev=1)
    dev, host = closing_spike_filter(device=True, **arg), closing_spike_filter(device=False, **arg)
    for d, h in zip(dev[:4], host[:4]):
        pd.testing.assert_frame_equal(d, h)
        assert len(d) > 0
    assert dev[4:] == host[4:] and 0 < len(dev[0]) < len(arg['align_list']) and 0 < dev[5] < dev[4]
