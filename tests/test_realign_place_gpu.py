"""The realigner's placement stage on the GPU, through its stage entry (realigner.place_batch -> mpn_realign_place_batch, which
runs the two functions realign_batch begins with): realign_fast_kernel's hits with their discovery time t and read offset p, the
k-mer bitmaps, and the coverage test and score bookkeeping made from them, against the plain restatement
(tests/realign_place_ref.py) on the constructed families of tests/realign_place_cases.py.  Every comparison is exact."""
import ctypes as ct

import pytest

import realign_place_cases as pc
import realign_place_ref as ref
from megapath_nano_amd import _ffi, realigner
from oracle import realign_oracle as ro

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('libmpn')]


def _want(w):
    return ref.results(pc.placed(w))


def _family(family):
    return [(n, w) for f, n, w in pc.make_cases() if f == family]


@pytest.mark.parametrize('family', pc.FAMILIES)
def test_family_equals_restatement_alone_batched_and_reversed(family):
    """each window alone, all as one batch, the batch reversed: a window's results do not depend on its neighbours"""
    cases = _family(family)
    for name, w in cases:
        (got,), launches = realigner.place_batch([w])
        assert got == _want(w), name
        assert launches == (1 if w['seqs'] and w['haplotypes'] else 0), name
    wins = [w for _, w in cases]
    got, _ = realigner.place_batch(wins)
    assert got == [_want(w) for w in wins]
    got, _ = realigner.place_batch(wins[::-1])
    assert got == [_want(w) for w in wins[::-1]]


def test_all_families_as_one_batch_and_small_grids():
    """grid_cap 1 and 2: every wave strides over many pairs (4 x gridDim apart)"""
    wins = [w for _, _, w in pc.make_cases()]
    want = [_want(w) for w in wins]
    assert sum(len(w['seqs']) * len(w['haplotypes']) for w in wins) > 64
    for grid_cap in (0, 1, 2):
        got, launches = realigner.place_batch(wins, grid_cap=grid_cap)
        assert got == want and launches == 1, grid_cap


@pytest.mark.parametrize('case', [('ties', 'tandem'), ('lengths', 'hl160'), ('clamp', 'only_clamp')])
def test_forced_overflow_takes_a_second_launch(case):
    w = pc.case(*case)
    want = _want(w)
    n = len(want['hits'])
    assert n >= 2
    for list_cap, launches in ((1, 2), (n - 1, 2), (n, 1), (n + 1, 1)):
        (got,), took = realigner.place_batch([w], list_cap=list_cap)
        assert took == launches and got == want, list_cap
    got, took = realigner.place_batch([w, pc.case('clamp', 'far'), w], list_cap=n, grid_cap=1)   # 2 n + 1 hits
    assert took == 2 and got == [want, _want(pc.case('clamp', 'far')), want]


def test_natural_overflow_at_the_default_knobs():
    """66 720 hits of one all-A haplotype: above the 65 536 the list starts with"""
    w = pc.all_a_window()
    (got,), launches = realigner.place_batch([w])
    assert launches == 2 and len(got['hits']) == pc.ALL_A_HITS
    assert got == _want(w)


def test_end_results_of_the_same_windows_equal_the_oracle(oracle_built):
    wins = [w for _, _, w in pc.make_cases()] + [pc.all_a_window()]
    got = realigner.realign_batch(wins)
    for (f, n, _), w, g in zip(pc.make_cases() + (('overflow', 'all_a', None),), wins, got):
        assert g == ro.realign_reads(**w), (f, n)


def test_refusals_leave_the_outputs_untouched():
    w = pc.case('shapes', 'pairs4')
    rc, out = realigner.place_call([w])
    assert rc == 0 and out['n_hits'].value > 0 and out['launches'].value == 1

    def refused(words, windows, **kw):
        rc, out = realigner.place_call(windows, **kw)
        assert rc == -2 and words in _ffi.last_error(), (rc, _ffi.last_error())
        for k, v in out.items():
            assert bytes(v) == b'\x55' * ct.sizeof(v), k

    refused('negative', [w], list_cap=-1)
    refused('negative', [w], grid_cap=-1)
    refused('negative', [w], hit_cap=-1)
    refused('room for', [w], hit_cap=out['n_hits'].value)            # below the bound asked for, though the hits would fit
    refused('malformed', [w, dict(w, reference=None)])
    refused('< 32', [w, dict(w, haplotypes=[w['haplotypes'][0], 'ACGT' * 7 + 'ACG'])])
    lib = _ffi.lib()
    n = ct.c_int64(-7)
    assert lib.mpn_realign_place_batch(-1, None, 0, 0, 0, None, ct.byref(n), None, None, None, None, None, ct.byref(ct.c_int32())) == -2
    assert lib.mpn_realign_place_batch(1, None, 0, 0, 0, None, ct.byref(n), None, None, None, None, None, ct.byref(ct.c_int32())) == -2
    assert n.value == -7
    with pytest.raises(_ffi.MpnError, match='mpn_realign_place_batch'):
        realigner.place_batch([w], list_cap=-1)
    assert realigner.place_batch([]) == ([], 0)
