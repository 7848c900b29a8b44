"""The de Bruijn graph consensus on the GPU (realigner.consensus_batch -> mpn_dbg_consensus_batch, realigner.get_consensus -> the
reference's own entry) against the plain restatement tests/dbg_ref.py, on the constructed families of tests/dbg_cases.py.  Every
comparison is exact on the list of haplotypes and on k."""
import ctypes as ct
import random

import pytest

import dbg_cases as dc
import dbg_ref
from megapath_nano_amd import _ffi, realigner

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('libmpn')]


def win(c):
    return dict(ref=c['ref'], reads=c['reads'], bad=c['bad'])


def want(cases):
    return [dc.expected(c) for c in cases]


@pytest.mark.parametrize('family', [f for f in dc.FAMILIES])
def test_family_alone_batched_and_reversed(family):
    """every window alone, all as one batch, the batch reversed: a window's result does not depend on its neighbours"""
    cases = dc.FAMILIES[family]()
    for c in cases:
        assert realigner.consensus_batch([win(c)]) == [dc.expected(c)], c['name']
    assert realigner.consensus_batch([win(c) for c in cases]) == want(cases)
    assert realigner.consensus_batch([win(c) for c in cases[::-1]]) == want(cases[::-1])


def test_stated_answers_and_statuses():
    """the counts the cases state (derived by hand from the reference's source), and the status that tells why a list is empty"""
    cases = dc.all_cases()
    rc, got, _ = realigner.consensus_call([win(c) for c in cases])
    assert rc == 0
    for c, (status, k, haps) in zip(cases, got):
        assert status == dc.expected_status(c), c['name']
        assert k == c.get('k', k) and len(haps) == c.get('n', len(haps)), c['name']


def test_all_windows_one_batch_grid_of_one_and_two_runs():
    cases = dc.all_cases()
    wins = [win(c) for c in cases]
    first = realigner.consensus_call(wins)
    assert first[0] == 0 and [(h, k) for _, k, h in first[1]] == want(cases)
    assert realigner.consensus_call(wins) == first                         # two runs: identical
    assert realigner.consensus_call(wins, grid_cap=1)[:2] == first[:2]      # one workgroup does every window in turn
    assert realigner.consensus_call(wins, grid_cap=3)[:2] == first[:2]


def test_small_tables_wrap_overflow_and_grow():
    cases = dc.table() + dc.cap()
    wins = [win(c) for c in cases]
    rc, got, redone = realigner.consensus_call(wins, table_cap=1024)
    assert rc == 0 and [(h, k) for _, k, h in got] == want(cases)
    assert redone >= 2                                                      # the noisy windows did not fit 1024 slots: done again, larger
    # every size between the smallest table and the windows' own: the same windows at other load factors, with probe runs that
    # wrap round the table's end, some of them redone and some not
    for cap in (2048, 4096, 8192, 16384):
        rc, got, _ = realigner.consensus_call(wins, table_cap=cap)
        assert rc == 0 and [(h, k) for _, k, h in got] == want(cases), cap


def test_long_insertion_grows_the_haplotype_buffers():
    ins = dc.R60[:30] + dc.rnd(300, 31) + dc.R60[30:]
    w = dict(ref=dc.R60, reads=[ins, ins], bad=None)
    rc, got, redone = realigner.consensus_call([w])
    assert rc == 0 and redone >= 1 and (got[0][2], got[0][1]) == dbg_ref.get_consensus(dc.R60, [ins, ins])
    assert len(got[0][2]) == 2


def test_random_small_windows():
    r = random.Random(77)
    windows = [dc.random_small_window(r) for _ in range(400)]
    got = realigner.consensus_batch([dict(ref=a, reads=b, bad=c) for a, b, c in windows])
    for (ref, rd, bad), g in zip(windows, got):
        haps, k, over = dbg_ref.consensus(ref, rd, bad)
        assert over or g == (haps, k), (ref, rd, bad)


def test_reference_entry_takes_the_scripts_strings():
    for c in dc.reads() + dc.support() + dc.cycles()[:2]:
        if any(',' in r for r in c['reads']):
            continue
        assert realigner.get_consensus(c['ref'], c['reads'], [sorted(b) for b in c['bad']]) == dc.expected(c)[0], c['name']
    # what the script sends for no reads at all: ''.split(',') is one empty read, with one empty list
    assert realigner.get_consensus(dc.R60, [''], ['']) == [dc.R60]
    # lists are split on ',', then on white space; positions outside the read and lists beyond the reads are ignored
    assert realigner.get_consensus(dc.R60, [dc.S30, dc.S30], [' 30  999', '30\t-4', '7']) == [dc.R60]
    assert realigner.get_consensus(dc.R60, [dc.S30, dc.S30], ['x 30', '']) == sorted([dc.R60, dc.S30])   # `ss >> int` stops at x


def test_refusals_come_before_anything_is_done():
    lib = _ffi.lib()
    with pytest.raises(_ffi.MpnError, match='lists of low-quality'):
        realigner.get_consensus(dc.R60, [dc.S30, dc.S30], ['30'])                        # fewer quality lists than reads
    with pytest.raises(_ffi.MpnError, match='over the limit of 1000'):
        realigner.consensus_batch([dict(ref=dc.rnd(1001, 5), reads=[], bad=None)])
    with pytest.raises(_ffi.MpnError, match='NULL'):
        realigner.consensus_batch([dict(ref=None, reads=[], bad=None)])
    lib.get_consensus.restype = ct.c_void_p
    lib.get_consensus.argtypes = [ct.c_char_p, ct.c_char_p, ct.c_char_p, ct.c_int]
    assert lib.get_consensus(None, b'', b'', 0) is None and 'NULL' in _ffi.last_error()
    assert realigner.consensus_call([dict(ref=dc.R60, reads=[], bad=None)], table_cap=-1)[0] == -2
    assert realigner.consensus_batch([dict(ref=dc.rnd(1000, 6), reads=[], bad=None)])[0][1] == 10     # the limit itself is served
    assert realigner.consensus_batch([]) == []
