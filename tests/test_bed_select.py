"""CPU tests of the BED union and of the selection of alignments by their overlap with a BED (megapath_nano_amd/abundance.py; no
GPU, no library): the numpy statements host_bed_union / host_cover_by_bed against a flag per position, and the mirrors of the
reference's select_alignment_by_bed (bin/megapath_nano.py:666-717), merge_bed_with_assembly_id (:362-382), step_noise_removal
(:2257-2278) and step_closing_spike_filter (:2353-2408) against plain restatements."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from bed_cases import brute_force, fraction_text, passes, random_small_case, union_as_lists
from depth_cases import read_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_union_and_cover_against_a_flag_per_position():
    from megapath_nano_amd.abundance import host_bed_union, host_cover_by_bed
    rng = np.random.default_rng(31)
    seen_merged = seen_dropped = seen_partial = 0
    for trial in range(300):
        c = random_small_case(rng)
        bed, query = c['bed'], c['query']
        want_merged, want_span, want_covered = brute_force(bed, query)
        merged, span = union_as_lists(host_bed_union(**bed))
        assert merged == want_merged and span == want_span, (trial, c)
        covered = host_cover_by_bed(bed['key'], bed['start'], bed['end'], n_keys=bed['n_keys'], **query)
        assert covered.dtype == np.int64 and covered.tolist() == want_covered, (trial, c)
        seen_merged += len(merged)
        seen_dropped += int((bed['start'] >= bed['end']).sum())
        seen_partial += sum(0 < v < e - s for v, s, e in zip(want_covered, query['q_start'], query['q_end']))
    assert seen_merged > 1000 and seen_dropped > 300 and seen_partial > 300            # the cases are not degenerate


def test_worked_example():
    from megapath_nano_amd.abundance import host_bed_union, host_cover_by_bed
    # key 0: [0,10) + [10,20) touch, [15,18) nested, [30,30) empty, [40,35) reversed, [50,60) twice; key 2: [5,6)
    key, start, end = [0, 0, 0, 0, 0, 0, 2, 0], [10, 0, 15, 30, 40, 50, 5, 50], [20, 10, 18, 30, 35, 60, 6, 60]
    merged, span = union_as_lists(host_bed_union(key, start, end, 3, key_group=[1, 0, 0], n_groups=2))
    assert merged == [(0, 0, 20), (0, 50, 60), (2, 5, 6)] and span == [1, 30]
    q = dict(q_key=[0, 0, 0, 0, 0, 1, 2, 0], q_start=[0, 20, 19, 5, 25, 0, 5, 55], q_end=[60, 50, 51, 5, 30, 60, 6, 70])
    # whole; in the gap, touching both neighbours; one position of each; empty query; gap; a key without BED; identical; right clip
    assert host_cover_by_bed(key, start, end, n_keys=3, **q).tolist() == [30, 0, 2, 0, 0, 0, 1, 5]
    with pytest.raises(ValueError):
        host_cover_by_bed(key, start, end, q_key=[0], q_start=[9], q_end=[8], n_keys=3)


def test_tile_constant_is_the_header_constant():
    from megapath_nano_amd import abundance
    text = open(os.path.join(ROOT, 'include', 'mpn_abundance.h')).read()
    assert int(re.search(r'#define\s+MPN_BED_TILE\s+(\d+)', text).group(1)) == abundance.BED_TILE


def _world():
    from megapath_nano_amd.abundance import align_list_to_depth_bed
    al, lens = read_table()
    mn = pd.DataFrame({'assembly_id': ['A1', 'A2', 'A3'], 'min_depth': [40.0, 18.0, 18.0]})
    bed, _ = align_list_to_depth_bed(align_list=al, min_depth=mn, device=False)
    return al, lens, bed


def _covered_by_loops(al, bed):
    """covered bp per alignment with a set of positions per (assembly, sequence)"""
    pos = {}
    asm = bed['assembly_id'] if 'assembly_id' in bed.columns else [''] * len(bed)
    for a, s, b, e in zip(asm, bed['sequence_id'], bed['start'], bed['end']):
        pos.setdefault((a, s), set()).update(range(int(b), int(e)))
    return [len(pos.get((r.assembly_id, r.sequence_id), set()) & set(range(r.sequence_from, r.sequence_to))) for r in al.itertuples(index=False)]


def test_select_against_the_text_restatement():
    from megapath_nano_amd.abundance import select_alignment_by_bed
    al, _, bed = _world()
    al = al.set_axis(np.arange(len(al))[::-1] * 3 + 7, axis=0)      # an index that is neither a range nor sorted
    covered = _covered_by_loops(al, bed)
    length = (al['sequence_to'] - al['sequence_from']).tolist()
    assert sum(c == 0 for c in covered) > 50 and sum(c == n for c, n in zip(covered, length)) > 50 and sum(0 < c < n for c, n in zip(covered, length)) > 50
    sizes = set()
    for lo, hi in ((0, 100), (0, 50), (50, 100), (0, 0), (100, 100), (50, 50), (30, 60)):
        for eq_max in (True, False):
            for eq_min in (True, False):
                kw = dict(max_overlap=hi, can_equal_to_max=eq_max, min_overlap=lo, can_equal_to_min=eq_min)
                got = select_alignment_by_bed(align_list=al, bed=bed, temp_dir_name='/nonexistent', device=False, **kw)
                want = al[[passes(c, n, **kw) for c, n in zip(covered, length)]]
                pd.testing.assert_frame_equal(got, want)
                sizes.add(len(got))
    assert len(sizes) > 6 and 0 in sizes and len(al) in sizes
    # strand is no part of the match, and no `index` column appears
    got = select_alignment_by_bed(align_list=al.assign(strand='-'), bed=bed, max_overlap=50, device=False)
    assert list(got.columns) == list(al.columns) + ['strand'] and list(got.index) == list(select_alignment_by_bed(align_list=al, bed=bed, max_overlap=50, device=False).index)


def test_empty_bed_truth_table():
    from megapath_nano_amd.abundance import select_alignment_by_bed
    al, _, bed = _world()
    for empty in (None, bed.iloc[0:0]):
        for hi in (0, 50, 100):
            for lo in (0, 50):
                for eq_max in (True, False):
                    for eq_min in (True, False):
                        got = select_alignment_by_bed(align_list=al, bed=empty, max_overlap=hi, can_equal_to_max=eq_max, min_overlap=lo,
                                                      can_equal_to_min=eq_min, device=False)
                        whole = lo == 0 and eq_min and (hi != 0 or eq_max)       # megapath_nano.py:676
                        pd.testing.assert_frame_equal(got, al if whole else al.iloc[0:0])
                        assert list(got.dtypes) == list(al.dtypes)
                        # with a BED that covers nothing of any alignment the covered fraction is 0.0 everywhere: the same answer
                        away = pd.DataFrame({'sequence_id': ['A1_c1'], 'start': [10 ** 8], 'end': [10 ** 8 + 5], 'assembly_id': ['A1']})
                        pd.testing.assert_frame_equal(select_alignment_by_bed(align_list=al, bed=away, max_overlap=hi, can_equal_to_max=eq_max, min_overlap=lo,
                                                                              can_equal_to_min=eq_min, device=False), got)


def _rows(rows):
    return pd.DataFrame(rows, columns=['read_id', 'assembly_id', 'sequence_id', 'sequence_from', 'sequence_to'])


def test_zero_and_negative_lengths_and_the_assembly_in_the_match():
    from megapath_nano_amd.abundance import select_alignment_by_bed
    bed = pd.DataFrame({'sequence_id': ['s'], 'start': [0], 'end': [100], 'assembly_id': ['A']})
    al = _rows([('r0', 'A', 's', 10, 10), ('r1', 'A', 's', 10, 20), ('r2', 'B', 's', 10, 20), ('r3', 'A', 't', 10, 20)])
    # L == 0: NaN passes no comparison, whatever the range
    for kw in (dict(), dict(max_overlap=0), dict(min_overlap=100), dict(can_equal_to_max=False, can_equal_to_min=False)):
        assert 'r0' not in list(select_alignment_by_bed(align_list=al, bed=bed, device=False, **kw)['read_id'])
    assert list(select_alignment_by_bed(align_list=al, bed=bed, device=False)['read_id']) == ['r1', 'r2', 'r3']
    # the same sequence_id under another assembly, and the same assembly with another sequence, are not covered
    assert list(select_alignment_by_bed(align_list=al, bed=bed, min_overlap=0, can_equal_to_min=False, device=False)['read_id']) == ['r1']
    other = bed.assign(assembly_id='B2')
    assert len(select_alignment_by_bed(align_list=al, bed=other, min_overlap=0, can_equal_to_min=False, device=False)) == 0
    # a BED without assembly_id is assembly '' and matches alignments of assembly '' only
    bare = bed[['sequence_id', 'start', 'end']]
    assert len(select_alignment_by_bed(align_list=al, bed=bare, min_overlap=0, can_equal_to_min=False, device=False)) == 0
    assert list(select_alignment_by_bed(align_list=al.assign(assembly_id=''), bed=bare, min_overlap=0, can_equal_to_min=False, device=False)['read_id']) == ['r1', 'r2']
    with pytest.raises(ValueError, match='sequence_to'):
        select_alignment_by_bed(align_list=_rows([('r0', 'A', 's', 10, 20), ('r1', 'A', 's', 10, 9)]), bed=bed, device=False)


ROUNDING = [(9999, 19998), (10000, 19999), (500001, 1000000), (1000001, 2000000), (2 ** 24 + 1, 2 ** 25 + 2), (2 ** 32 - 1, 2 ** 32 - 1)]


def test_rounding_cases_follow_the_text_and_not_the_rational():
    from megapath_nano_amd.abundance import overlap_fraction, select_alignment_by_bed
    assert fraction_text(9999, 19998) == '0.500000' and fraction_text(10000, 19999) == '0.500025'
    c, n = np.array([p[0] for p in ROUNDING], dtype=np.int64), np.array([p[1] for p in ROUNDING], dtype=np.int64)
    assert overlap_fraction(c, n).tolist() == [float(fraction_text(a, b)) for a, b in ROUNDING]
    # through the select: alignment i = [0, L_i) on its own sequence, covered by one BED interval [0, c_i)
    al = _rows([(f'r{i}', 'A', f's{i}', 0, b) for i, (a, b) in enumerate(ROUNDING)])
    bed = pd.DataFrame({'sequence_id': [f's{i}' for i in range(len(ROUNDING))], 'start': 0, 'end': [a for a, b in ROUNDING], 'assembly_id': 'A'})
    differs = 0
    for eq_max in (True, False):
        got = list(select_alignment_by_bed(align_list=al, bed=bed, max_overlap=50, can_equal_to_max=eq_max, device=False)['read_id'])
        want = [passes(a, b, max_overlap=50, can_equal_to_max=eq_max) for a, b in ROUNDING]
        assert got == [f'r{i}' for i, w in enumerate(want) if w]
        exact = [(2 * a <= b) if eq_max else (2 * a < b) for a, b in ROUNDING]
        differs += sum(w != e for w, e in zip(want, exact))
    assert differs > 0                                              # e.g. 500001 / 1000000 prints as 0.500001 but 1000001 / 2000000 as 0.500000
    # the two forms of the fraction, row by row, on random pairs and around every printed tie in reach
    rng = np.random.default_rng(32)
    n = rng.integers(1, 2 ** 32, size=3000)
    c = (rng.random(3000) * (n + 1)).astype(np.int64)
    assert overlap_fraction(c, n).tolist() == [float(fraction_text(a, b)) for a, b in zip(c.tolist(), n.tolist())]


def _bed(rows, with_assembly=True):
    cols = ['sequence_id', 'start', 'end', 'assembly_id']
    return pd.DataFrame(rows, columns=cols if with_assembly else cols[:3])


def test_merge_bed_with_assembly_id():
    from megapath_nano_amd.abundance import merge_bed_with_assembly_id
    one = _bed([('b', 10, 20, 'A'), ('s', 0, 5, 'C'), ('a', 3, 9, 'A,'), ('b', 40, 50, 'A'), ('b', 7, 7, 'A')])
    two = _bed([('b', 20, 30, 'A'), ('b', 45, 47, 'A'), ('s', 5, 6, 'B'), ('s', 4, 8, 'C'), ('a', 9, 12, 'A,'), ('b', 0, 9, 'A')])
    got = merge_bed_with_assembly_id([one, None, one.iloc[0:0], two], device=False)
    assert list(got.columns) == ['sequence_id', 'start', 'end', 'assembly_id']
    # 'A,,a' < 'A,b' < 'B,s' < 'C,s'; [10,20) + [20,30) touch across the two BEDs; [0,9) stays apart from [10,30); [7,7) is empty
    assert [tuple(r) for r in got.itertuples(index=False)] == [('a', 3, 12, 'A,'), ('b', 0, 9, 'A'), ('b', 10, 30, 'A'), ('b', 40, 50, 'A'),
                                                               ('s', 5, 6, 'B'), ('s', 0, 8, 'C')]
    assert got['start'].dtype == np.int64 and got['end'].dtype == np.int64
    # a BED without assembly_id is assembly '': ',b' sorts before everything else and does not merge with ('A', 'b')
    bare = _bed([('b', 25, 35), ('b', 35, 36)], with_assembly=False)
    got = merge_bed_with_assembly_id([one, bare], device=False)
    assert [tuple(r) for r in got.itertuples(index=False)][:3] == [('b', 25, 36, ''), ('a', 3, 9, 'A,'), ('b', 10, 20, 'A')]
    # all empty: the four columns with the depth BED's dtypes, and no GPU needed whatever `device` says
    from megapath_nano_amd.abundance import align_list_to_depth_bed
    ref = align_list_to_depth_bed(align_list=pd.DataFrame(columns=['assembly_id', 'sequence_id', 'sequence_length', 'sequence_from', 'sequence_to']), device=False)[0]
    for beds in ([], [None], [one.iloc[0:0], bare.iloc[0:0]]):
        for device in (False, True, None):
            pd.testing.assert_frame_equal(merge_bed_with_assembly_id(beds, device=device), ref)


def test_noise_removal_against_plain_pandas():
    from megapath_nano_amd.abundance import noise_removal
    al, _, bed = _world()
    covered = _covered_by_loops(al, bed)
    keep_ids = pd.DataFrame({'assembly_id': ['A3', 'A1', 'ZZ']})
    for max_overlap in (0, 20, 100):
        got, before, after = noise_removal(align_list=al, noise_bed=bed, non_zero_assembly_ids=keep_ids, max_align_noise_overlap=max_overlap, device=False)
        # megapath_nano.py:2259-2272: the select with max_overlap, then the inner m:1 merge on assembly_id
        sel = al[[passes(c, n, max_overlap=max_overlap) for c, n in zip(covered, al['sequence_to'] - al['sequence_from'])]]
        want = sel.merge(right=keep_ids.set_index('assembly_id'), how='inner', left_on='assembly_id', right_index=True, validate='m:1')
        pd.testing.assert_frame_equal(got, want)
        assert (before, after) == (len(al), len(want)) and 0 < after < before
    by_list = noise_removal(align_list=al, noise_bed=bed, non_zero_assembly_ids=['A3', 'A1'], max_align_noise_overlap=100, device=False)[0]
    pd.testing.assert_frame_equal(by_list, got)                     # plain ids in place of the table
    with pytest.raises(ValueError):
        noise_removal(align_list=al, noise_bed=bed, non_zero_assembly_ids=['A1', 'A3', 'A1'], max_align_noise_overlap=20, device=False)


def test_closing_spike_filter_against_plain_pandas():
    from megapath_nano_amd.abundance import closing_spike_filter, merge_bed_with_assembly_id, spike_noise
    al, lens, bed = _world()
    with_short = al.sort_values(['read_id', 'alignment_score', 'alignment_score_tiebreaker']).drop_duplicates(subset=['read_id'], keep='last')
    best = with_short[(with_short['sequence_to'] - with_short['sequence_from']) >= 300]
    al_in = al[al['read_id'].isin(best['read_id'])]
    for stdev, max_overlap in ((9, 30), (1, 30), (1, 90)):
        out, noise_bed, spike_bed, stat, before, after = closing_spike_filter(
            align_list=al_in, best_align_list=best, best_align_list_with_short_alignment=with_short, noise_bed=bed, assembly_length=lens,
            max_align_noise_overlap=max_overlap, expected_max_depth_stdev=stdev, device=False)
        # megapath_nano.py:2353-2408
        want_spike, want_stat = spike_noise(with_short, lens, stdev, device=False)
        pd.testing.assert_frame_equal(spike_bed, want_spike)
        assert list(stat.columns) == ['assembly_id', 'closing_spike_span_bp', 'closing_spike_span_percent'] and stat.values.tolist() == want_stat.values.tolist()
        want_bed = merge_bed_with_assembly_id([bed, want_spike], device=False)
        pd.testing.assert_frame_equal(noise_bed, want_bed)
        covered = _covered_by_loops(best, want_bed)
        gone = best[[passes(c, n, min_overlap=max_overlap, can_equal_to_min=False) for c, n in zip(covered, best['sequence_to'] - best['sequence_from'])]][['read_id']]
        want = al_in.merge(right=gone.set_index('read_id').assign(read_to_remove=lambda x: 1), how='left', left_on='read_id', right_index=True,
                           validate='m:1').fillna(0).query('read_to_remove == 0').drop(['read_to_remove'], axis=1)
        pd.testing.assert_frame_equal(out, want)
        assert before == len(best) and after == want.sort_values(['read_id']).drop_duplicates(subset=['read_id']).shape[0]
        assert 0 < len(gone) < len(best) and 0 < len(out) < len(al_in) and after == before - len(gone)
    assert len(want_spike) > 0 and len(want_bed) <= len(bed) + len(want_spike)
