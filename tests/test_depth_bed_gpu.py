"""GPU tests (-m gpu) of mpn_depth_by_key (include/mpn_abundance.h; csrc/interval_kernels.hip): depth profile, depth BED and depth
span must equal the numpy statement and a counter per position as arrays, order included -- on random small cases, at the sizes
where a tiled scan goes wrong (the event count 2n around the multiples of the tile), and through the mirrors of the reference's
align_list_to_depth_bed and step_spike_filter."""
import ctypes as ct

import numpy as np
import pandas as pd
import pytest

from depth_cases import as_lists, brute_force, random_small_case, read_table, same_result

pytestmark = pytest.mark.gpu


def _both(**arg):
    from megapath_nano_amd.abundance import device_depth_by_key, host_depth_by_key
    dev, host = device_depth_by_key(**arg), host_depth_by_key(**arg)
    assert same_result(dev, host), {k: (v if np.ndim(v) == 0 or len(v) < 40 else f'[{len(v)}]') for k, v in arg.items()}
    return dev


def test_device_equals_host_equals_brute_force_on_small_cases(libmpn):
    rng = np.random.default_rng(22)
    for trial in range(150):
        c = random_small_case(rng)
        rows, bed, span = as_lists(_both(**c))
        want_rows, want_bed, want_span = brute_force(**c)
        assert rows == want_rows and bed == want_bed and span == list(want_span), trial


def test_worked_example_and_tiny_inputs(libmpn):
    one = dict(key_len=[100], key_group=[0], n_groups=1)
    arg = dict(key=[0] * 7, start=[0, 5, 10, 40, 50, 95, 70], end=[10, 20, 30, 50, 60, 120, 70], **one)
    rows, bed, span = as_lists(_both(**arg))
    assert rows == [(0, 0, 5, 1), (0, 5, 20, 2), (0, 20, 30, 1), (0, 40, 60, 1), (0, 95, 100, 1)]
    assert bed == [(0, 0, 30), (0, 40, 60), (0, 95, 100)] and span == [55]
    rows, bed, span = as_lists(_both(**arg, depth_lo=[2], depth_hi=[2 ** 31 - 1]))
    assert bed == [(0, 5, 20)] and span == [15]
    assert as_lists(_both(key=[], start=[], end=[], **one)) == ([], [], [0])                 # n = 0
    assert as_lists(_both(key=[0], start=[3], end=[8], **one)) == ([(0, 3, 8, 1)], [(0, 3, 8)], [5])   # n = 1
    assert as_lists(_both(key=[0], start=[7], end=[7], **one)) == ([], [], [0])               # one empty interval only
    assert as_lists(_both(key=[0], start=[9], end=[2], **one)) == ([], [], [0])               # start > end


def test_clip_and_ignore_rules_at_the_key_length(libmpn):
    two = dict(key_len=[100, 50], key_group=[0, 1], n_groups=2)
    rows, bed, span = as_lists(_both(key=[0, 0, 0, 0, 1, 1, 1], start=[100, 99, 150, 90, 50, 49, 0], end=[120, 100, 160, 400, 60, 51, 50], **two))
    # start == length and start > length: ignored; an end beyond the length: clipped; end == length: kept whole
    assert rows == [(0, 90, 99, 1), (0, 99, 100, 2), (1, 0, 49, 1), (1, 49, 50, 2)]
    assert bed == [(0, 90, 100), (1, 0, 50)] and span == [10, 50]


def _sizes():
    """n with the event count 2n just below, at and just above a multiple of the tile (2n is even, so that is -2, 0, +2; the
    cases below move the content by one event where the parity matters)"""
    from megapath_nano_amd.abundance import DEPTH_TILE
    return sorted({t * DEPTH_TILE // 2 + d for t in (1, 2, 3, 5) for d in (-1, 0, 1)})


def test_event_counts_around_the_tile_boundaries(libmpn):
    from megapath_nano_amd.abundance import DEPTH_TILE
    one = dict(key_len=[10 ** 7], key_group=[0], n_groups=1)
    rng = np.random.default_rng(23)
    for n in _sizes():
        key = np.zeros(n, dtype=np.int32)
        # one key spanning all tiles, random intervals
        start = rng.integers(0, 40 * n, size=n)
        _both(key=key, start=start, end=start + rng.integers(1, 200, size=n), **one)
        # all intervals with the same start: one position carries the net change n, the depth reaches n
        rows, bed, span = _both(key=key, start=np.full(n, 1000), end=1001 + np.arange(n), **one)
        assert rows[3][0] == n and len(rows[0]) == n and bed[1].tolist() == [1000] and bed[2].tolist() == [1000 + n] and span.tolist() == [n]
        # ... and the same end: one row of depth n
        rows, bed, span = as_lists(_both(key=key, start=np.full(n, 1000), end=np.full(n, 2000), **one))
        assert rows == [(0, 1000, 2000, n)] and bed == [(0, 1000, 2000)] and span == [1000]
        # a chain of book-ended intervals: exactly one row
        chain = 10 * np.arange(n)
        rows, bed, span = as_lists(_both(key=key, start=chain, end=chain + 10, **one))
        assert rows == [(0, 0, 10 * n, 1)] and bed == [(0, 0, 10 * n)] and span == [10 * n]
        # the chain with every second link overlapped by one extra interval: the depth alternates link by link.  wide: one
        # interval over the whole chain in place of the last extra, which moves every row boundary by one event
        links = (2 * n + 2) // 3
        c = 10 * np.arange(links)
        for wide in (False, True):
            s = np.concatenate([c, c[::2][:n - links]])
            e = s + 10
            if wide:
                s[-1], e[-1] = 0, 10 * links + 5
            assert len(s) == n
            rows, bed, span = _both(key=key, start=s, end=e, **one)
            assert len(rows[0]) >= n - links and len(bed[0]) == 1 and span.tolist() == [10 * links + 5 * wide]
            rows, bed, span = _both(key=key, start=s, end=e, **one, depth_lo=[2], depth_hi=[2])
            assert len(bed[0]) >= (n - links) // 2
    # row boundaries exactly at the tile edges: a pattern of 4 events per period, so every tile starts where a period starts; the
    # position between two periods carries an end and a start (net change 0) and must not split the row of depth 1
    links = DEPTH_TILE * 3 // 4
    c = 20 * np.arange(links)
    s, e = np.concatenate([c, c + 10]), np.concatenate([c + 15, c + 20])            # [0,15) [10,20) | [20,35) [30,40) ...
    assert 2 * len(s) == 3 * DEPTH_TILE
    rows, bed, span = _both(key=np.zeros(len(s), dtype=np.int32), start=s, end=e, **one)
    assert rows[3].tolist() == [1, 2] * links + [1] and rows[2][:3].tolist() == [10, 15, 30] and len(bed[0]) == 1 and span.tolist() == [20 * links]


def test_many_small_keys_beside_one_that_holds_half_of_the_intervals(libmpn):
    """the shape of the cover test: 600 000 intervals, 2000 groups; every tile holds hundreds of key changes, and one key runs
    through hundreds of tiles"""
    rng = np.random.default_rng(24)
    n, n_groups, small = 600000, 2000, 300000
    key = np.where(rng.random(n) < 0.5, 0, rng.integers(1, small + 1, size=n)).astype(np.int32)
    key_len = np.concatenate([[50_000_000], rng.integers(1000, 30000, size=small)]).astype(np.int64)
    key_group = np.concatenate([[0], rng.integers(1, n_groups, size=small)]).astype(np.int32)
    start = (rng.random(n) * key_len[key] * 1.02).astype(np.int64)
    end = start + rng.integers(0, 20000, size=n)
    dev = _both(key=key, start=start, end=end, key_len=key_len, key_group=key_group, n_groups=n_groups)
    assert len(dev[0][0]) > n // 2 and dev[0][3].max() > 50
    lo = rng.integers(1, 3, size=n_groups).astype(np.int32)
    lo[0], hi = 40, lo + rng.integers(-1, 3, size=n_groups).astype(np.int32)
    hi[0] = 2 ** 31 - 1
    dev = _both(key=key, start=start, end=end, key_len=key_len, key_group=key_group, n_groups=n_groups, depth_lo=lo, depth_hi=hi)
    assert 0 < len(dev[1][0]) < len(dev[0][0]) and dev[2][0] > 0


def test_filter(libmpn):
    # key 0 / group 0: depths 1 2 3 2 1 on [0,10) [10,20) [20,30) [30,40) [40,50); key 1 / group 1 and key 2 / group 2: the same
    s, e = [0, 10, 20], [50, 40, 30]
    arg = dict(key=[0] * 3 + [1] * 3 + [2] * 3, start=s * 3, end=e * 3, key_len=[100] * 3, key_group=[0, 1, 2], n_groups=3)
    # group 0: 2..3 -> touching passing rows of different depth merge; group 1: lo > hi -> nothing; group 2: 1..1 -> the failing
    # rows in the middle keep the two passing rows apart
    rows, bed, span = as_lists(_both(**arg, depth_lo=[2, 3, 1], depth_hi=[3, 2, 1]))
    assert len(rows) == 15 and bed == [(0, 10, 40), (2, 0, 10), (2, 40, 50)] and span == [30, 0, 20]
    # groups on both sides of the bounds: everything below, everything above
    rows, bed, span = as_lists(_both(**arg, depth_lo=[4, 0, -5], depth_hi=[9, 0, 0]))
    assert bed == [] and span == [0, 0, 0]
    rows, bed, span = as_lists(_both(**arg, depth_lo=[-2 ** 31, 1, 3], depth_hi=[2 ** 31 - 1, 3, 3]))
    assert bed == [(0, 0, 50), (1, 0, 50), (2, 20, 30)] and span == [50, 50, 10]
    # two keys of one group add into one span
    two = dict(key=[0, 1, 1], start=[0, 5, 5], end=[10, 9, 9], key_len=[100, 100], key_group=[0, 0], n_groups=1)
    assert as_lists(_both(**two, depth_lo=[1], depth_hi=[2]))[2] == [14]


def test_bad_arguments_return_minus_two_and_leave_the_outputs_untouched(libmpn):
    from megapath_nano_amd import _ffi, abundance
    lib = abundance._lib()
    n, cap = 3, 6
    key, start, end = np.array([0, 1, 0], np.int32), np.array([0, 5, 10], np.int64), np.array([10, 9, 30], np.int64)
    key_len, key_group = np.array([100, 100], np.int64), np.array([0, 1], np.int32)

    def call(key=key, start=start, cap=cap, key_group=key_group):
        out32 = [np.full(cap + 2, -7, np.int32) for _ in range(3)]
        out64 = [np.full(cap + 2, -7, np.int64) for _ in range(5)]
        n_rows, n_bed = ct.c_int64(-7), ct.c_int64(-7)
        rc = lib.mpn_depth_by_key(n, key.ctypes.data, start.ctypes.data, end.ctypes.data, 2, key_len.ctypes.data, key_group.ctypes.data, 2, None, None, cap,
                                  out32[0].ctypes.data, out64[0].ctypes.data, out64[1].ctypes.data, out32[1].ctypes.data, ct.byref(n_rows),
                                  out32[2].ctypes.data, out64[2].ctypes.data, out64[3].ctypes.data, ct.byref(n_bed), out64[4].ctypes.data)
        untouched = all((a == -7).all() for a in out32 + out64) and n_rows.value == -7 and n_bed.value == -7
        return rc, untouched, n_rows.value, n_bed.value, out64[4][:2].tolist()

    assert call() == (0, False, 2, 2, [30, 4])                      # [0,10) and [10,30) on key 0 are book-ended: one row
    rc, untouched = call(cap=5)[:2]
    assert rc == -2 and untouched and 'cap' in _ffi.last_error()
    rc, untouched = call(key=np.array([0, 2, 0], np.int32))[:2]
    assert rc == -2 and untouched and 'record 1' in _ffi.last_error()
    rc, untouched = call(key=np.array([0, 1, -1], np.int32))[:2]
    assert rc == -2 and untouched and 'record 2' in _ffi.last_error()
    rc, untouched = call(start=np.array([0, 1 << 32, 0], np.int64))[:2]
    assert rc == -2 and untouched and 'record 1' in _ffi.last_error()
    rc, untouched = call(key_group=np.array([0, 2], np.int32))[:2]
    assert rc == -2 and untouched and 'key 1' in _ffi.last_error()
    with pytest.raises(_ffi.MpnError):
        abundance.device_depth_by_key([0, 5], [0, 0], [1, 1], [10], [0], 1)


def test_mirrors_on_the_device_equal_their_host_forms(libmpn):
    from megapath_nano_amd.abundance import align_list_to_depth_bed, depth_profile, spike_noise
    al, lens = read_table()
    for stdev in (6, 1):
        dev, host = spike_noise(al, lens, expected_max_depth_stdev=stdev, device=True), spike_noise(al, lens, expected_max_depth_stdev=stdev, device=False)
        pd.testing.assert_frame_equal(dev[0], host[0])
        pd.testing.assert_frame_equal(dev[1], host[1])
        assert len(dev[0]) > 0
    mx = pd.DataFrame({'assembly_id': ['A1', 'A3'], 'max_depth': [30.5, float('nan')]})
    mn = pd.DataFrame({'assembly_id': ['A1', 'A2', 'A3'], 'min_depth': [2, 1, 1.5]})
    for kw in (dict(), dict(max_depth=mx, can_equal_to_max=False), dict(min_depth=mn, max_depth=mx), dict(min_depth=mn, can_equal_to_min=False)):
        dev, host = align_list_to_depth_bed(align_list=al, device=True, **kw), align_list_to_depth_bed(align_list=al, device=False, **kw)
        pd.testing.assert_frame_equal(dev[0], host[0])
        pd.testing.assert_frame_equal(dev[1], host[1])
        assert len(dev[0]) > 0
    pd.testing.assert_frame_equal(depth_profile(al, device=True), depth_profile(al, device=False))
    pd.testing.assert_frame_equal(depth_profile(al), depth_profile(al, device=False))          # None is the device
