"""CPU tests of the host forms behind assembly selection (megapath_nano_amd/abundance.py): host_good_rows and host_sum_by_key against
plain loops over dicts on every case of tests/select_cases.py, the threshold edges as literals; good_align_list, best_align_per_read,
align_stat_by_sequence_id and assembly_selection with device=False against goldens made by the reference's own functions
(tests/golden/make_assembly_selection_golden.py) -- index order, columns and integers exactly, derived floats bit for bit, the
summed tiebreaker within n * 2^-52 relative -- and the mirrors' edge behaviour."""
import re

import numpy as np
import pandas as pd
import pytest

from select_cases import (EDGE_RESULTS, SPECIES_LIST, TILE, brute_good_rows, brute_sum_by_key, caller_shapes, check_frame, golden, good_cases, inputs_digest,
                          selection_cases, selection_inputs, sum_cases, threshold_edge_cases)


@pytest.fixture(scope='module')
def selections():
    """golden record, inputs and the host result of assembly_selection per case, computed once"""
    from megapath_nano_amd import abundance
    out = []
    for rec in golden():
        inp = selection_inputs(rec['case'])
        assert inputs_digest(inp) == rec['tables_sha1'], 'the seeded tables are not the ones the golden was made from'
        got = abundance.assembly_selection(species_align_list=inp['species_align_list'], assembly_align_list=inp['assembly_align_list'],
                                           species_list=inp['species_list'], read_id_species_id=inp['read_id_species_id'],
                                           assembly_ID_min_average_depth=rec['case']['min_depth'], good_align_threshold=rec['case']['threshold'],
                                           assembly_length=inp['assembly_length'], assembly_tax=inp['assembly_tax'], device=False)
        out.append((rec, inp, got))
    return out


def test_the_tile_is_the_header_s_and_the_goldens_cover_the_cases():
    from megapath_nano_amd import abundance
    text = open(abundance.__file__.replace('megapath_nano_amd/abundance.py', 'include/mpn_abundance.h')).read()
    assert TILE == abundance.BEST_TILE == int(re.search(r'#define MPN_BEST_TILE (\d+)', text).group(1))
    assert [r['case'] for r in golden()] == selection_cases() and len(golden()) == 6


def test_host_good_rows_equals_the_loops_on_every_case_and_caller_shape():
    from megapath_nano_amd.abundance import host_good_rows
    kept_some = dropped_some = 0
    for name, case in good_cases():
        for shape, c in caller_shapes(case):
            good, best = host_good_rows(**c)
            want_good, want_best = brute_good_rows(c['read'], c['unit'], c['score'], c['tiebreak'], c['n_reads'], c['threshold'])
            assert good.dtype == np.int64 and best.dtype == np.int64 and good.tolist() == want_good and best.tolist() == want_best, (name, shape)
            everything = host_good_rows(**dict(c, threshold=None))[0]
            kept_some += len(good) > 0
            dropped_some += len(good) < len(everything)
    assert kept_some > 60 and dropped_some > 30


def test_threshold_edges_are_one_float64_product():
    from megapath_nano_amd.abundance import host_good_rows
    assert 100 * 0.07 > 7 and 10 * 0.7 == 7.0 and 100 * 0.9 == 90.0
    for name, case in threshold_edge_cases():
        assert host_good_rows(**case)[0].tolist() == EDGE_RESULTS[name], name
    # through the mirror: percent / 100 is the factor
    table = pd.DataFrame({'read_id': ['r', 'r', 'q', 'q', 'q'], 'assembly_id': ['A', 'B', 'A', 'B', 'C'], 'alignment_score': [10, 7, 100, 90, 7],
                          'alignment_score_tiebreaker': [0.5] * 5}, index=[7, 5, 3, 1, 9])
    from megapath_nano_amd.abundance import good_align_list
    assert 7 / 100 == 0.07
    assert list(good_align_list(align_list=table, good_align_threshold=7, device=False).index) == [3, 1, 7, 5]        # q's 7 misses 7.000000000000001
    assert list(good_align_list(align_list=table, good_align_threshold=70, device=False).index) == [3, 1, 7, 5]
    assert list(good_align_list(align_list=table, good_align_threshold=90, device=False).index) == [3, 1, 7]
    assert list(good_align_list(align_list=table, good_align_threshold=0, device=False).index) == [3, 1, 9, 7, 5]
    assert list(good_align_list(align_list=table, good_align_threshold=101, device=False).index) == []


def test_host_good_rows_refuses_what_the_entry_refuses():
    from megapath_nano_amd.abundance import host_good_rows
    ok = dict(read=[0, 1], unit=[0, 1], score=[5, 6], tiebreak=[0.5, 0.5], n_reads=2, n_units=2, threshold=0.9)
    assert host_good_rows(**ok)[0].tolist() == [0, 1]
    for bad in (dict(threshold=float('nan')), dict(threshold=float('inf')), dict(score=[5, 2 ** 53]), dict(score=[-2 ** 53, 5]), dict(read=[0, 2]),
                dict(unit=[-1, 0]), dict(tiebreak=[0.5, float('nan')])):
        with pytest.raises(ValueError):
            host_good_rows(**dict(ok, **bad))


def test_host_sum_by_key_equals_the_loops_on_every_case():
    from megapath_nano_amd.abundance import host_sum_by_key
    for name, c in sum_cases():
        count, sums = host_sum_by_key(**c)
        want_count, want_sums = brute_sum_by_key(c['key'], c['n_keys'], c['cols'])
        assert count.dtype == np.int64 and sums.dtype == np.int64 and sums.shape == (len(c['cols']), c['n_keys']), name
        assert count.tolist() == want_count and sums.tolist() == want_sums, name
    assert max(abs(v) for v in want_sums[0]) > 2 ** 50                     # the last case: sums far beyond float64's exact integers times 2^-3
    ok = dict(key=[0, 1], n_keys=2, cols=[[1, 2]])
    for bad in (dict(cols=[[1, 2]] * 7), dict(cols=[]), dict(key=[0, 2]), dict(key=[-1, 0]), dict(cols=[[2 ** 32, 0]]), dict(cols=[[0, -2 ** 32]])):
        with pytest.raises(ValueError):
            host_sum_by_key(**dict(ok, **bad))


def test_good_align_list_and_the_statistic_per_sequence_equal_the_reference_s(selections):
    from megapath_nano_amd import abundance
    for rec, inp, _ in selections:
        name, species = rec['case']['name'], inp['species_align_list']
        good = abundance.good_align_list(align_list=species, good_align_threshold=rec['case']['threshold'], device=False)
        check_frame(good, rec['good_align_list'], name, source=species)
        stat = abundance.align_stat_by_sequence_id(species, inp['sequence_length'], noise_bed=inp['noise_bed'], device=False)
        check_frame(stat, rec['align_stat_by_sequence_id'], name, rows_summed=stat['total_number_of_read'])
        assert (stat['noise_span_bp'] > 0).any() == (inp['noise_bed'] is not None), name
    assert sum(len(r['good_align_list']['index']) for r, _, _ in selections) > 500


def test_assembly_selection_equals_the_reference_s_step(selections):
    for rec, inp, got in selections:
        name = rec['case']['name']
        both = pd.concat([inp['assembly_align_list'], inp['species_align_list']], sort=True)
        for attr in ('align_list', 'best_align_list', 'good_align_list'):
            check_frame(getattr(got, attr), rec['selection_' + attr], (name, attr), source=both)
        check_frame(got.align_stat, rec['selection_align_stat'], name, rows_summed=got.align_stat['total_number_of_read'])
        check_frame(got.assembly_list, rec['selection_assembly_list'], name, rows_summed=got.assembly_list['total_number_of_read'])
        assert got.num_species_reached_min_average_depth + got.num_species_not_reached == len(SPECIES_LIST), name
        assert list(got.best_align_list['read_id']) == sorted(set(got.align_list['read_id'])), name
    assert any(0 < g.num_species_reached_min_average_depth < 3 for _, _, g in selections)


def test_equal_depths_occur_in_the_dedicated_case_only_and_the_tiebreakers_decide_it_safely(selections):
    """Where two assemblies of a species have one adjusted_average_depth, the summed tiebreaker picks; pandas and np.bincount sum it
    differently, so such a tie may only occur where the two sums lie far apart."""
    from megapath_nano_amd import abundance
    tied = []
    for rec, inp, got in selections:
        species_stat = abundance.align_stat_by_assembly_id(inp['species_align_list'], inp['assembly_length'], inp['assembly_tax'], device=False)
        for stat in (species_stat, got.align_stat):
            for _, group in stat.groupby(['species_tax_id', 'adjusted_average_depth']):
                if len(group) > 1:
                    tied.append(rec['case']['name'])
                    t = sorted(group['alignment_score_tiebreaker'])
                    assert t[1] - t[0] > 0.5
                    assert got.species_align_stat.set_index('species_tax_id').loc[100, 'assembly_id'] == 'A1'      # A2 has half A1's tiebreakers
    assert tied == ['two assemblies of equal depth']


def test_the_statistic_through_the_exact_sums_is_the_public_one(selections):
    from megapath_nano_amd import abundance
    for rec, inp, got in selections:
        pd.testing.assert_frame_equal(got.align_stat, abundance.align_stat_by_assembly_id(got.good_align_list, inp['assembly_length'], inp['assembly_tax'], device=False))


def test_empty_tables_and_a_sequence_under_two_assemblies(selections):
    from megapath_nano_amd import abundance
    _, inp, _ = selections[0]
    species = inp['species_align_list']
    empty = species.iloc[0:0]
    for out in (abundance.good_align_list(align_list=empty, good_align_threshold=90, device=False), abundance.best_align_per_read(empty, device=False)):
        assert out.shape[0] == 0 and list(out.columns) == list(species.columns)
    stat = abundance.align_stat_by_sequence_id(empty, inp['sequence_length'], device=False)
    full = abundance.align_stat_by_sequence_id(species, inp['sequence_length'], device=False)
    assert stat.shape[0] == 0 and list(stat.columns) == list(full.columns) and [str(t) for t in stat.dtypes] == [str(t) for t in full.dtypes]
    twice = species.assign(sequence_id=np.where(species['assembly_id'] == 'A2', 'A1_c1', species['sequence_id']))
    with pytest.raises(ValueError, match='A1_c1'):
        abundance.align_stat_by_sequence_id(twice, inp['sequence_length'], device=False)


def test_best_align_per_read_is_the_pandas_idiom(selections):
    from megapath_nano_amd import abundance
    for _, inp, _ in selections:
        table = inp['species_align_list']
        want = table.sort_values(['read_id', 'alignment_score', 'alignment_score_tiebreaker']).drop_duplicates(subset=['read_id'], keep='last')
        assert abundance.best_align_per_read(table, device=False).equals(want)


def test_no_species_or_every_species_reaching_the_depth(selections):
    from megapath_nano_amd import abundance
    rec, inp, _ = selections[0]
    kw = dict(species_align_list=inp['species_align_list'], assembly_align_list=inp['assembly_align_list'], species_list=inp['species_list'],
              read_id_species_id=inp['read_id_species_id'], good_align_threshold=rec['case']['threshold'], assembly_length=inp['assembly_length'],
              assembly_tax=inp['assembly_tax'], device=False)
    none = abundance.assembly_selection(assembly_ID_min_average_depth=1e9, **kw)
    assert (none.num_species_reached_min_average_depth, none.num_species_not_reached) == (0, 4)
    assert (none.align_list.index < 100000).all() and none.align_list.shape[0] > 0            # rows of the species table only
    every = abundance.assembly_selection(assembly_ID_min_average_depth=0.0, **kw)
    assert (every.num_species_reached_min_average_depth, every.num_species_not_reached) == (3, 1)      # species 400 has no alignment
    assert (every.align_list.index >= 100000).sum() == inp['assembly_align_list'].shape[0]
    assert sorted(every.assembly_list['species_tax_id']) == [100, 200, 300] and list(none.align_list.columns) == list(every.align_list.columns)
