"""CPU tests of the depth profile, depth BED and depth span (megapath_nano_amd/abundance.py; no GPU, no library): the numpy
statement host_depth_by_key against a counter per position, the threshold conversions, and the mirrors of the reference's
align_list_to_depth_bed (bin/megapath_nano.py:417-482) and step_spike_filter (:1759-1806) against plain loops."""
import math
import os
import re

import numpy as np
import pandas as pd
import pytest

from depth_cases import as_lists, brute_force, random_small_case, read_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_depth_by_key_against_a_counter_per_position():
    from megapath_nano_amd.abundance import host_depth_by_key
    rng = np.random.default_rng(21)
    seen_rows = seen_bed = 0
    for trial in range(400):
        c = random_small_case(rng)
        rows, bed, span = as_lists(host_depth_by_key(**c))
        want_rows, want_bed, want_span = brute_force(**c)
        assert rows == want_rows and bed == want_bed and span == list(want_span), (trial, c)
        seen_rows += len(rows)
        seen_bed += len(bed)
    assert seen_rows > 2000 and seen_bed > 300                      # the cases are not degenerate


def test_worked_example():
    from megapath_nano_amd.abundance import host_depth_by_key
    start, end = [0, 5, 10, 40, 50, 95, 70], [10, 20, 30, 50, 60, 120, 70]
    arg = dict(key=[0] * 7, start=start, end=end, key_len=[100], key_group=[0], n_groups=1)
    rows, bed, span = as_lists(host_depth_by_key(**arg))
    assert rows == [(0, 0, 5, 1), (0, 5, 20, 2), (0, 20, 30, 1), (0, 40, 60, 1), (0, 95, 100, 1)]
    assert bed == [(0, 0, 30), (0, 40, 60), (0, 95, 100)] and span == [55]
    rows2, bed, span = as_lists(host_depth_by_key(**arg, depth_lo=[2], depth_hi=[2 ** 31 - 1]))    # depth > 1
    assert rows2 == rows and bed == [(0, 5, 20)] and span == [15]


def test_threshold_conversions_equal_the_float_comparisons():
    from megapath_nano_amd.abundance import depth_bound
    for x in (0, 0.5, 1, 1.5, 2.9999, 3):
        for depth in range(0, 7):
            assert (depth <= depth_bound(x, '<')) == (depth < x)
            assert (depth <= depth_bound(x, '<=')) == (depth <= x)
            assert (depth >= depth_bound(x, '>')) == (depth > x)
            assert (depth >= depth_bound(x, '>=')) == (depth >= x)
    assert depth_bound(3, '<') == 2 and depth_bound(3, '<=') == 3 and depth_bound(3, '>') == 4 and depth_bound(3, '>=') == 3
    assert depth_bound(2.9999, '<') == 2 and depth_bound(2.9999, '<=') == 2 and depth_bound(2.9999, '>') == 3 and depth_bound(2.9999, '>=') == 3
    assert depth_bound(math.inf, '<=') == 2 ** 31 - 1 and depth_bound(-math.inf, '>') == -2 ** 31


def test_tile_constant_is_the_header_constant():
    from megapath_nano_amd import abundance
    text = open(os.path.join(ROOT, 'include', 'mpn_abundance.h')).read()
    assert int(re.search(r'#define\s+MPN_DEPTH_TILE\s+(\d+)', text).group(1)) == abundance.DEPTH_TILE


def _table(rows):
    return pd.DataFrame(rows, columns=['assembly_id', 'sequence_id', 'sequence_length', 'sequence_from', 'sequence_to'])


def test_align_list_to_depth_bed_on_a_hand_made_table():
    from megapath_nano_amd.abundance import align_list_to_depth_bed, depth_profile
    # string order of assembly_id + ',' + sequence_id: 'A,,a' < 'A,b' < 'B,s' < 'C,s', while the tuple ('A', 'b') < ('A,', 'a')
    assert sorted(['A,b', 'A,,a']) == ['A,,a', 'A,b'] and sorted([('A,', 'a'), ('A', 'b')]) == [('A', 'b'), ('A,', 'a')]
    al = _table([('A', 'b', 100, 0, 10), ('A', 'b', 100, 5, 20), ('A', 'b', 100, 10, 30), ('A', 'b', 100, 40, 50), ('A', 'b', 100, 50, 60),
                 ('A', 'b', 100, 95, 120), ('A', 'b', 100, 70, 70),
                 ('A,', 'a', 50, 3, 9), ('A,', 'a', 50, 3, 9), ('A,', 'a', 50, 3, 9),
                 ('C', 's', 30, 0, 30), ('C', 's', 30, 10, 20),
                 ('B', 's', 30, 1, 4)])
    prof = depth_profile(al, device=False)
    assert list(prof.columns) == ['assembly_id', 'sequence_id', 'start', 'end', 'depth']
    assert [tuple(r) for r in prof.itertuples(index=False)] == [
        ('A,', 'a', 3, 9, 3), ('A', 'b', 0, 5, 1), ('A', 'b', 5, 20, 2), ('A', 'b', 20, 30, 1), ('A', 'b', 40, 60, 1), ('A', 'b', 95, 100, 1),
        ('B', 's', 1, 4, 1), ('C', 's', 0, 10, 1), ('C', 's', 10, 20, 2), ('C', 's', 20, 30, 1)]
    # no threshold: everything, merged
    bed, span = align_list_to_depth_bed(align_list=al, temp_dir_name='/nonexistent', device=False)
    assert list(bed.columns) == ['sequence_id', 'start', 'end', 'assembly_id'] and list(span.columns) == ['assembly_id', 'span_bp']
    assert [tuple(r) for r in bed.itertuples(index=False)] == [('a', 3, 9, 'A,'), ('b', 0, 30, 'A'), ('b', 40, 60, 'A'), ('b', 95, 100, 'A'),
                                                               ('s', 1, 4, 'B'), ('s', 0, 30, 'C')]
    assert dict(zip(span['assembly_id'], span['span_bp'])) == {'A': 55, 'A,': 6, 'B': 3, 'C': 30} and list(span['assembly_id']) == ['A', 'A,', 'B', 'C']
    # depth > 1 for A, NaN (-1) for C, B absent (dropped), 'A,' needs > 3 (nothing): span_bp only for assemblies with rows
    mn = pd.DataFrame({'assembly_id': ['A', 'C', 'A,', 'ZZ'], 'min_depth': [1.0, float('nan'), 3, 0], 'other': [7, 7, 7, 7]})
    bed, span = align_list_to_depth_bed(align_list=al, min_depth=mn, can_equal_to_min=False, device=False)
    assert [tuple(r) for r in bed.itertuples(index=False)] == [('b', 5, 20, 'A'), ('s', 0, 30, 'C')]
    assert [tuple(r) for r in span.itertuples(index=False)] == [('A', 15), ('C', 30)]
    bed, span = align_list_to_depth_bed(align_list=al, min_depth=mn, can_equal_to_min=True, device=False)
    assert [tuple(r) for r in span.itertuples(index=False)] == [('A', 55), ('A,', 6), ('C', 30)]
    # the variable-region form: depth < max; NaN is 99999999
    mx = pd.DataFrame({'assembly_id': ['A', 'C', 'B'], 'max_depth': [2, float('nan'), 0.5]})
    bed, span = align_list_to_depth_bed(align_list=al, max_depth=mx, can_equal_to_max=False, device=False)
    assert [tuple(r) for r in bed.itertuples(index=False)] == [('b', 0, 5, 'A'), ('b', 20, 30, 'A'), ('b', 40, 60, 'A'), ('b', 95, 100, 'A'), ('s', 0, 30, 'C')]
    assert [tuple(r) for r in span.itertuples(index=False)] == [('A', 40), ('C', 30)]
    # both bounds: 2 <= depth <= 2 on A and C; B is in the maximum table only and drops out
    mn2 = pd.DataFrame({'assembly_id': ['A', 'C'], 'min_depth': [1.5, 2]})
    mx2 = pd.DataFrame({'assembly_id': ['A', 'C', 'B'], 'max_depth': [2.5, 2, 9]})
    bed, span = align_list_to_depth_bed(align_list=al, min_depth=mn2, max_depth=mx2, device=False)
    assert [tuple(r) for r in bed.itertuples(index=False)] == [('b', 5, 20, 'A'), ('s', 10, 20, 'C')]
    assert [tuple(r) for r in span.itertuples(index=False)] == [('A', 15), ('C', 10)]
    # the BED goes straight into the statistic's noise branch column-wise
    assert bed['start'].dtype == np.int64 and bed['end'].dtype == np.int64 and span['span_bp'].dtype == np.int64


def test_empty_table_and_inconsistent_lengths():
    from megapath_nano_amd.abundance import align_list_to_depth_bed, depth_profile
    empty = _table([])
    bed, span = align_list_to_depth_bed(align_list=empty, device=False)
    assert list(bed.columns) == ['sequence_id', 'start', 'end', 'assembly_id'] and len(bed) == 0
    assert list(span.columns) == ['assembly_id', 'span_bp'] and len(span) == 0
    prof = depth_profile(empty, device=False)
    assert list(prof.columns) == ['assembly_id', 'sequence_id', 'start', 'end', 'depth'] and len(prof) == 0
    # also with device=True: an empty table needs no GPU
    assert len(align_list_to_depth_bed(align_list=empty, device=True)[0]) == 0
    with pytest.raises(ValueError, match='sequence_length'):
        align_list_to_depth_bed(align_list=_table([('A', 's', 100, 0, 10), ('A', 's', 101, 5, 9)]), device=False)


def _spike_restatement(al, lens, stdev):
    """megapath_nano.py:1768-1798 with plain loops: the statistic's adjusted_average_depth from the best row per (read, assembly),
    expected_max_depth, then a counter per position over ALL rows and the positions above the threshold."""
    best = {}
    for row in al.itertuples(index=False):
        k = (row.read_id, row.assembly_id)
        if k not in best or (row.alignment_score, row.alignment_score_tiebreaker) > (best[k].alignment_score, best[k].alignment_score_tiebreaker):
            best[k] = row
    length = dict(zip(lens['assembly_id'], lens['assembly_length']))
    bed, stat = [], []
    seq_len = {}
    for row in al.itertuples(index=False):
        seq_len[(row.assembly_id, row.sequence_id)] = row.sequence_length
    for a in sorted({k[1] for k in best}):
        mine = [v for k, v in best.items() if k[1] == a]
        covered = set()
        for v in mine:
            covered |= {(v.sequence_id, p) for p in range(v.sequence_from, v.sequence_to)}
        tab = sum(v.sequence_to - v.sequence_from for v in mine)
        aad = (len(covered) / length[a]) * tab / length[a]
        expected = max(1, int(aad + stdev * math.sqrt(aad)))
        span = 0
        for (a2, s) in sorted(seq_len, key=lambda t: t[0] + ',' + t[1]):
            if a2 != a:
                continue
            count = [0] * (seq_len[(a2, s)] + 1)
            for row in al.itertuples(index=False):
                if row.assembly_id == a and row.sequence_id == s:
                    for p in range(row.sequence_from, min(row.sequence_to, seq_len[(a2, s)])):
                        count[p] += 1
            run = None
            for p, c in enumerate(count):
                if c > expected and run is None:
                    run = p
                if c <= expected and run is not None:
                    bed.append((s, run, p, a))
                    span += p - run
                    run = None
        if span:
            stat.append((a, span, span / length[a]))
    return bed, stat


def test_spike_noise_against_a_plain_restatement_and_through_the_statistic():
    from megapath_nano_amd.abundance import align_stat_by_assembly_id, spike_noise
    al, lens = read_table()
    some = False
    for stdev in (6, 1, 9):
        bed, stat = spike_noise(al, lens, expected_max_depth_stdev=stdev, device=False)
        want_bed, want_stat = _spike_restatement(al, lens, stdev)
        assert list(bed.columns) == ['sequence_id', 'start', 'end', 'assembly_id']
        assert list(stat.columns) == ['assembly_id', 'spike_span_bp', 'spike_span_percent']
        assert [tuple(r) for r in bed.itertuples(index=False)] == want_bed
        assert [(r[0], r[1]) for r in stat.itertuples(index=False)] == [(w[0], w[1]) for w in want_stat]
        assert all(abs(r[2] - w[2]) < 1e-15 for r, w in zip(stat.itertuples(index=False), want_stat))
        some |= stdev == 6 and len(want_bed) > 0 and len(want_stat) < 3
        # fed back as the noise BED of the statistic: noise_span_bp is the spike span
        again = align_stat_by_assembly_id(al, lens, noise_bed=bed, device=False).set_index('assembly_id')
        spike = dict(zip(stat['assembly_id'], stat['spike_span_bp']))
        assert {a: int(again.loc[a, 'noise_span_bp']) for a in again.index} == {a: int(spike.get(a, 0)) for a in again.index}
    assert some                                                     # the default threshold finds the pile-up and not every assembly
