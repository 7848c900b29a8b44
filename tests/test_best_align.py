"""CPU tests of the best alignment per read (megapath_nano_amd/abundance.py): the numpy statements of mpn_best_candidates,
mpn_pick_weighted and mpn_second_best_by_read against plain loops, the tie rules on literals, and the mirrors
align_list_to_best_align_list, short_alignment_removal and unique_alignment (device=False) against goldens made by the reference's
own functions (tests/golden/make_best_align_golden.py), against the loops, and in the number and order of their random draws."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from best_cases import (BELOW_ONE, LENGTHS, TINY, best_table, brute_candidates, brute_pick, brute_second, check_against_brute_force, check_against_golden,
                        counter_rng, golden, golden_cases, golden_inputs, noise_bed_for, random_pick_case, random_small_case, read_classes)
from megapath_nano_amd import abundance
from megapath_nano_amd.abundance import (align_list_to_best_align_list, host_best_candidates, host_pick_weighted, host_second_best_by_read)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def as_lists(result):
    return [[float(v) if a.dtype.kind == 'f' else int(v) for v in a] for a in result]


def test_tile_constant_equals_the_header():
    text = open(os.path.join(ROOT, 'include', 'mpn_abundance.h')).read()
    assert int(re.search(r'#define MPN_BEST_TILE (\d+)', text).group(1)) == abundance.BEST_TILE


def test_host_statements_equal_the_loops_on_small_cases():
    rng = np.random.default_rng(51)
    seen_several = 0
    for trial in range(150):
        c = random_small_case(rng)
        got = host_best_candidates(**c)
        assert [a.dtype for a in got] == [np.int64, np.int32, np.int64, np.int64]
        want = brute_candidates(c['read'], c['assembly'], c['score'], c['tiebreak'], c['n_reads'])
        assert as_lists(got) == [list(w) for w in want], trial
        p = random_pick_case(rng, got[1], c['n_reads'])
        new, winner = host_pick_weighted(**p)
        assert new.dtype == np.float64 and winner.dtype == np.int64
        want_new, want_winner = brute_pick(p['read'], p['weight'], p['tiebreak'], p['draw'], p['n_reads'])
        assert [x.hex() for x in new.tolist()] == [x.hex() for x in want_new] and winner.tolist() == want_winner, trial
        seen_several += int((got[2] > 1).sum())
        excluded = rng.integers(-1, c['n_assemblies'], size=c['n_reads']).astype(np.int32)
        second = host_second_best_by_read(c['read'], c['assembly'], c['score'], c['n_reads'], excluded)
        assert second.dtype == np.int64 and second.tolist() == brute_second(c['read'], c['assembly'], c['score'], c['n_reads'], excluded), trial
    assert seen_several > 100


def test_tie_rules_on_literals():
    # read 0: assembly 0 has rows 0, 2, 4 -- 2 and 4 equal in score and tiebreak: the last, 4, is kept; assembly 1 has row 1 with a
    # lower tiebreak but the same score: both are candidates.  read 1: one row.  read 2: none.  read 3: assembly 2 scores higher.
    read, assembly = [0, 0, 0, 1, 0, 3, 3, 3], [0, 1, 0, 5, 0, 1, 2, 2]
    score, tiebreak = [7, 7, 7, -3, 7, 4, 5, 5], [0.1, 0.0, 0.5, 0.9, 0.5, 0.9, 0.2, 0.3]
    row, rd, count, first = host_best_candidates(read, assembly, score, tiebreak, 4, 6)
    assert (row.tolist(), rd.tolist(), count.tolist(), first.tolist()) == ([4, 1, 3, 7], [0, 0, 1, 3], [2, 1, 0, 1], [0, 2, 3, 3])
    # -0.0 and 0.0 are one tiebreaker: the later row wins whichever sign it has
    assert host_best_candidates([0, 0], [0, 0], [1, 1], [0.0, -0.0], 1, 1)[0].tolist() == [1]
    assert host_best_candidates([0, 0], [0, 0], [1, 1], [-0.0, 0.0], 1, 1)[0].tolist() == [1]
    # every row identical: the last input row of every assembly, and in the draw the last assembly among equal products
    row, rd, count, first = host_best_candidates([0] * 6, [2, 1, 2, 1, 0, 0], [9] * 6, [0.5] * 6, 1, 3)
    assert row.tolist() == [5, 3, 2] and count.tolist() == [3]
    new, winner = host_pick_weighted(rd, [0, 0, 0], [0.5] * 3, [0.25, 0.25, 0.25], 1)
    assert new.tolist() == [0.25, 0.25, 0.25] and winner.tolist() == [2]                 # all weights 0: relative = 1
    # one weight 0 among positive ones: its product is 0.0 whatever it drew; a read alone keeps its tiebreak and ignores its draw
    new, winner = host_pick_weighted([0, 0, 0, 2], [3, 0, 1, 0], [0.9, 0.9, 0.9, 0.125], [0.5, BELOW_ONE, 0.5, 0.7], 3)
    assert new.tolist() == [0.5 * (3 / 4), 0.0, 0.5 * (1 / 4), 0.125] and winner.tolist() == [0, -1, 3]
    # sums near 2^52 and denormal draws
    big = 2 ** 52 - 1
    new, winner = host_pick_weighted([0, 0], [big, big], [0.0, 0.0], [TINY, BELOW_ONE], 1)
    assert new.tolist() == [TINY * (big / (2 * big)), BELOW_ONE * 0.5] and winner.tolist() == [1]
    with pytest.raises(ValueError):
        host_pick_weighted([0, 0], [2 ** 52, 2 ** 52], [0.0, 0.0], [0.5, 0.5], 1)
    with pytest.raises(ValueError):
        host_pick_weighted([1, 0], [1, 1], [0.0, 0.0], [0.5, 0.5], 2)
    with pytest.raises(ValueError):
        host_best_candidates([0], [0], [1], [float('nan')], 1, 1)
    with pytest.raises(ValueError):
        host_best_candidates([0], [1], [1], [0.5], 1, 1)
    assert host_second_best_by_read([0, 0, 1, 2], [0, 1, 1, 0], [9, -4, 6, 5], 4, [0, 1, -1, -1]).tolist() == [-4, 0, 5, 0]


def test_the_tables_hold_both_classes_of_reads():
    for case in golden_cases()[:2] + golden_cases()[-1:]:
        table = best_table(**case['table'])
        one, several, without = read_classes(table)
        assert one >= (one + several) / 4 and several >= (one + several) / 4 and 'A6' in without, (case['name'], one, several, without)
    one, several, _ = read_classes(best_table(**golden_cases()[2]['table']))
    assert one == 0 and several == 25                                                   # every row tied: no abundance at all


def test_mirrors_equal_the_goldens():
    cases = golden()
    assert [c['name'] for c in cases] == [c['name'] for c in golden_cases()]
    drawn = 0
    for rec in cases:
        best = check_against_golden(rec, device=False)
        table, _ = golden_inputs(rec)
        drawn += int((best['alignment_score_tiebreaker'].to_numpy() != table.loc[best.index, 'alignment_score_tiebreaker'].to_numpy()).sum())
    assert drawn > 100


def test_mirror_equals_the_loops_and_draws_once_per_candidate_in_order():
    total = 0
    for case in golden_cases():
        table = best_table(**case['table'])
        noise = noise_bed_for(table, case['noise_seed']) if 'noise_seed' in case else None
        total += check_against_brute_force(table, noise, device=False)
    assert total > 500
    # the k-th draw goes to the k-th candidate in (read_id, assembly_id) order: with every weight 0 the tiebreaker IS the draw
    table = best_table(seed=73, n_reads=25, all_tied=True)
    rng = counter_rng()
    best = align_list_to_best_align_list(align_list=table, assembly_length=LENGTHS, rng=rng, device=False)
    pairs = sorted(set(zip(table['read_id'], table['assembly_id'])))
    assert rng.calls == len(pairs)
    last_of_read = {r: k + 1 for k, (r, _) in enumerate(pairs)}                          # the largest draw of a read is its last one
    assert [t * 2 ** 20 for t in best['alignment_score_tiebreaker']] == [last_of_read[r] for r in best['read_id']]
    assert [a for a in best['assembly_id']] == [max(a for r2, a in pairs if r2 == r) for r in best['read_id']]


def test_no_draw_without_a_tie_and_none_for_an_empty_table():
    def never():
        raise AssertionError('drawn')
    table = best_table(seed=3, n_reads=20)
    table = table.sort_values(['read_id', 'alignment_score']).drop_duplicates('read_id', keep='last')      # one row a read
    best = align_list_to_best_align_list(align_list=table, assembly_length=LENGTHS, rng=never, device=False)
    pd.testing.assert_frame_equal(best, table.sort_values('read_id'))
    empty = align_list_to_best_align_list(align_list=table.iloc[0:0], assembly_length=LENGTHS, rng=never, device=False)
    assert empty.shape[0] == 0 and list(empty.columns) == list(table.columns)
    out, before, after = abundance.short_alignment_removal(align_list=table, min_align_length=10 ** 6, assembly_length=LENGTHS, rng=never, device=False)
    assert (out.shape[0], before, after) == (0, 20, 0)


def test_closing_spike_step_draws_for_the_filtered_table_first():
    with_short = best_table(seed=81, n_reads=40)
    table = with_short[(with_short['sequence_to'] - with_short['sequence_from']) >= 400]
    rng = counter_rng()
    got = abundance.closing_spike_step(align_list=table, align_list_with_short_alignment=with_short, noise_bed=None, assembly_length=LENGTHS,
                                       max_align_noise_overlap=30, expected_max_depth_stdev=1, rng=rng, device=False)
    again = counter_rng()
    best = align_list_to_best_align_list(align_list=table, assembly_length=LENGTHS, rng=again, device=False)
    first_calls = again.calls
    best_short = align_list_to_best_align_list(align_list=with_short, assembly_length=LENGTHS, rng=again, device=False)
    assert 0 < first_calls < again.calls == rng.calls
    want = abundance.closing_spike_filter(align_list=table, best_align_list=best, best_align_list_with_short_alignment=best_short, noise_bed=None,
                                          assembly_length=LENGTHS, max_align_noise_overlap=30, expected_max_depth_stdev=1, device=False)
    for g, w in zip(got[:4], want[:4]):
        pd.testing.assert_frame_equal(g, w)
    assert got[4:] == want[4:] and got[4] == best.shape[0]


def test_unique_alignment_and_combine_on_literals():
    al = pd.DataFrame({'read_id': ['a', 'a', 'a', 'b', 'b', 'c'], 'assembly_id': ['X', 'Y', 'X', 'X', 'Y', 'Z'], 'alignment_score': [100, 90, 95, 50, 50, 10]},
                      index=[5, 6, 7, 8, 9, 10])
    best = al.loc[[5, 9, 10]]
    human = pd.DataFrame({'read_id': ['c', 'd'], 'assembly_id': ['H', 'H'], 'alignment_score': [9, 99]})
    out, before, after = abundance.unique_alignment(align_list=al, best_align_list=best, human_best_align_list=human, unique_align_threshold=95, device=False)
    # a: 100 * 0.95 > 90 (its own assembly's 95 does not count); b: 47.5 > 50 fails; c: 9.5 > 9 through the human table
    assert list(out.index) == [5, 10] and out['second_best_alignment_score'].tolist() == [90, 9] and (before, after) == (3, 2)
    assert list(out.columns) == ['read_id', 'assembly_id', 'alignment_score', 'second_best_alignment_score']
    out = abundance.unique_alignment(align_list=al, best_align_list=best, unique_align_threshold=90, device=False)[0]
    assert list(out.index) == [10] and out['second_best_alignment_score'].tolist() == [0]                  # 90 > 90 fails; c has no other row
    with pytest.raises(ValueError):
        abundance.unique_alignment(align_list=al, best_align_list=al, unique_align_threshold=90, device=False)
    both = abundance.combine_with_human_and_decoy(align_list=al, human_and_decoy_best_align_list=pd.DataFrame(
        {'read_id': ['a', 'c'], 'assembly_id': ['H', 'D'], 'alignment_score': [95, 10]}, index=[70, 71]))
    assert list(both.index) == [5, 8, 9, 70, 71] and list(both.columns) == ['alignment_score', 'assembly_id', 'read_id']
