"""CPU test: the rules of the de Bruijn graph consensus (csrc/dbg_core.h) built for the host with g++ (scripts/dbg_host_check.cpp,
under AddressSanitizer and UBSan where the toolchain has their runtimes) and run with one lane, against the restatement
tests/dbg_ref.py: every constructed window, the table's refusal and growth, and a few thousand small random windows."""
import random

import pytest

import dbg_cases as dc
import dbg_ref


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return dc.build_host_check(tmp_path_factory.mktemp('dbg_host'))


def windows_of(cases):
    return [(c['ref'], c['reads'], c['bad']) for c in cases]


def test_constructed_cases_equal_the_restatement(exe, tmp_path):
    cases = dc.all_cases()
    got = dc.host_run(exe, tmp_path, windows_of(cases))
    for c, (status, k, haps, _) in zip(cases, got):
        want, want_k = dc.expected(c)
        assert (haps, k) == (want, want_k), c['name']
        assert status == dc.expected_status(c), c['name']


def test_a_full_table_is_refused_or_grown_never_cut(exe, tmp_path):
    c = dc.table()[0]
    refused = dc.host_run(exe, tmp_path, windows_of([c]), slots=1024, grow=0)[0]
    assert refused[0] == dc.TABLE_FULL and refused[2] == []
    for c in dc.table():
        status, k, haps, redone = dc.host_run(exe, tmp_path, windows_of([c]), slots=1024, grow=1)[0]
        assert status == dc.expected_status(c) and redone >= 1 and (haps, k) == dc.expected(c)


def test_a_long_insertion_grows_the_haplotype_buffers(exe, tmp_path):
    ref = dc.R60
    ins = ref[:30] + dc.rnd(200, 31) + ref[30:]
    want = dbg_ref.get_consensus(ref, [ins, ins])
    assert len(want[0]) == 2
    assert dc.host_run(exe, tmp_path, [(ref, [ins, ins], [set(), set()])], grow=0)[0][0] == dc.HAP_FULL
    status, k, haps, redone = dc.host_run(exe, tmp_path, [(ref, [ins, ins], [set(), set()])])[0]
    assert (status, haps, k) == (dc.OK,) + want and redone >= 1


def test_random_small_windows_equal_the_restatement(exe, tmp_path):
    r = random.Random(2024)
    windows = [dc.random_small_window(r) for _ in range(3000)]
    got = dc.host_run(exe, tmp_path, windows)
    kinds = set()
    for (ref, rd, bad), (status, k, haps, _) in zip(windows, got):
        want, want_k, over = dbg_ref.consensus(ref, rd, bad)
        if over:
            continue
        assert (haps, k) == (want, want_k), (ref, rd, bad)
        kinds.add((min(len(want), 3), want_k > 10))
    assert kinds >= {(0, False), (1, False), (2, False), (1, True), (2, True)}     # empty lists, several haplotypes, raised k
