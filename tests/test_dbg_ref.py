"""CPU test: pins tests/dbg_ref.py, the restatement of the reference's de Bruijn graph consensus.  The reference's own library needs
Boost and cannot be built here, so nothing of its output is stored: the cases below were derived by hand from the text of
debruijn_graph.cpp, and every constructed window of tests/dbg_cases.py that states an answer must give it."""
import pytest

import dbg_cases as dc
import dbg_ref


def test_the_base_reference_has_distinct_10mers():
    assert dbg_ref.k_bounds(dc.R60) == (10, 59) and dbg_ref.k_bounds(dc.R150) == (10, 101)


def test_no_reads_give_the_reference_alone():
    assert dbg_ref.get_consensus(dc.R60, []) == ([dc.R60], 10)


def test_a_snp_in_one_read_is_pruned():
    assert dbg_ref.get_consensus(dc.R60, [dc.S30]) == ([dc.R60], 10)


def test_a_snp_in_two_reads_gives_both_sorted():
    assert dbg_ref.get_consensus(dc.R60, [dc.S30, dc.S30]) == (sorted([dc.R60, dc.S30]), 10)


def test_a_bad_position_at_the_snp_gives_the_reference_alone():
    assert dbg_ref.get_consensus(dc.R60, [dc.S30, dc.S30], [{30}, {30}]) == ([dc.R60], 10)


def test_reference_of_11_bases_gives_itself_and_10_nothing():
    a, b = dc.rnd(11, 5), dc.rnd(10, 4)
    assert dbg_ref.get_consensus(a, []) == ([a], 10) and dbg_ref.get_consensus(b, []) == ([], 0)


def test_tandem_reference_starts_at_k_11():
    c = next(c for c in dc.cycles() if c['name'] == 'tandem_12mer')
    assert dbg_ref.k_bounds(c['ref'])[0] == 11


CASES = dc.all_cases()


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_constructed_case(c):
    haps, k = dc.expected(c)
    assert haps == sorted(haps) and (k == 0) <= (haps == [])
    if 'k' in c:
        assert k == c['k']
    if 'n' in c:
        assert len(haps) == c['n']
    if c.get('n') == 1:
        assert haps == [c['ref']]
    assert not dbg_ref.order_matters(c['ref'], c['reads'], c['bad'])     # no test uses a window where adjacency order could decide


def test_names_are_unique_and_every_family_is_there():
    names = [c['name'] for c in CASES]
    assert len(set(names)) == len(names) and set(dc.FAMILIES) == {'bounds', 'reads', 'support', 'dangling', 'cycles', 'cap', 'table'}


def test_cap_cases_hold_whatever_the_order():
    eight, nine = dc.cap()
    haps, _ = dc.expected(eight)
    assert len(set(haps)) == 256 and dbg_ref.get_consensus(nine['ref'], nine['reads'])[0] == []
