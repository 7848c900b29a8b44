"""GPU tests (-m gpu) of mpn_good_rows and mpn_sum_by_key (include/mpn_abundance.h; csrc/interval_kernels.hip) and of the functions
that stand on them: both entries must equal their numpy statements exactly on every case of tests/select_cases.py -- the good rows
in the three shapes their callers give them (assembly units, sequence units, the single unit) -- and good_align_list,
best_align_per_read, align_stat_by_sequence_id and assembly_selection with device=True must equal device=False as frames, floats bit
for bit (the one float sum is formed on the host either way).  Bad arguments and rows outside the domain are refused before
anything is written."""
import ctypes as ct

import numpy as np
import pandas as pd
import pytest

from select_cases import EDGE_RESULTS, caller_shapes, golden, good_cases, selection_inputs, sum_cases, threshold_edge_cases

pytestmark = pytest.mark.gpu


def _same(dev, host):
    """equal as arrays: shapes, order, dtypes, values"""
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(dev, host))


def _bits(frame):
    """the frame with its float columns as their bits, so that equality is bit for bit"""
    return frame.assign(**{c: frame[c].to_numpy().view(np.int64) for c in frame.columns if frame[c].dtype == np.float64})


def _equal_frames(dev, host):
    pd.testing.assert_frame_equal(_bits(dev), _bits(host), check_exact=True)


@pytest.fixture(scope='module')
def good_results():
    """host_good_rows on every case and caller shape, computed once"""
    from megapath_nano_amd.abundance import host_good_rows
    return [(name, shape, c, host_good_rows(**c)) for name, case in good_cases() for shape, c in caller_shapes(case)]


def test_device_good_rows_equals_the_host_form_on_every_case_and_caller_shape(libmpn, good_results):
    from megapath_nano_amd.abundance import device_good_rows
    for name, shape, c, host in good_results:
        dev = device_good_rows(**c)
        assert _same(dev, host) and len(dev[0]) == len(host[0]), (name, shape)                     # good_row, n_good, read_best
    big = [h for name, shape, _, h in good_results if name == 'one read through 300 tiles' and shape == 'assemblies'][0]
    assert len(big[0]) == 5 and big[1].tolist() == [599]                                          # unit 2 stays below the bar


def test_threshold_edges_on_the_device(libmpn):
    from megapath_nano_amd.abundance import device_good_rows, good_align_list
    for name, case in threshold_edge_cases():
        assert device_good_rows(**case)[0].tolist() == EDGE_RESULTS[name], name
    table = pd.DataFrame({'read_id': ['r', 'r', 'q', 'q', 'q'], 'assembly_id': ['A', 'B', 'A', 'B', 'C'], 'alignment_score': [10, 7, 100, 90, 7],
                          'alignment_score_tiebreaker': [0.5] * 5}, index=[7, 5, 3, 1, 9])
    for percent, want in ((7, [3, 1, 7, 5]), (70, [3, 1, 7, 5]), (90, [3, 1, 7]), (0, [3, 1, 9, 7, 5]), (101, [])):
        assert list(good_align_list(align_list=table, good_align_threshold=percent).index) == want, percent      # device=None is the device


def test_device_sum_by_key_equals_the_host_form_on_every_case(libmpn):
    from megapath_nano_amd.abundance import device_sum_by_key, host_sum_by_key
    for name, c in sum_cases():
        dev, host = device_sum_by_key(**c), host_sum_by_key(**c)
        assert _same(dev, host), name
    count, total = host                                                                            # the last case: 2^20 rows at +-(2^32 - 1)
    assert int(total[0][0]) == (2 ** 32 - 1) * int(count[0]) > 2 ** 50 and int(total[2].sum()) == -(2 ** 32 - 1) * 2 ** 20


def test_mirrors_on_the_device_equal_their_host_forms(libmpn):
    from megapath_nano_amd import abundance
    for rec in golden():
        case, inp = rec['case'], selection_inputs(rec['case'])
        species = inp['species_align_list']
        for table in (species, inp['assembly_align_list']):
            _equal_frames(abundance.good_align_list(align_list=table, good_align_threshold=case['threshold'], device=True),
                          abundance.good_align_list(align_list=table, good_align_threshold=case['threshold'], device=False))
            _equal_frames(abundance.best_align_per_read(table, device=True), abundance.best_align_per_read(table, device=False))
        _equal_frames(abundance.align_stat_by_sequence_id(species, inp['sequence_length'], noise_bed=inp['noise_bed'], device=True),
                      abundance.align_stat_by_sequence_id(species, inp['sequence_length'], noise_bed=inp['noise_bed'], device=False))
        kw = dict(species_align_list=species, assembly_align_list=inp['assembly_align_list'], species_list=inp['species_list'],
                  read_id_species_id=inp['read_id_species_id'], assembly_ID_min_average_depth=case['min_depth'], good_align_threshold=case['threshold'],
                  assembly_length=inp['assembly_length'], assembly_tax=inp['assembly_tax'])
        dev, host = abundance.assembly_selection(device=True, **kw), abundance.assembly_selection(device=False, **kw)
        for attr in ('align_list', 'best_align_list', 'good_align_list', 'align_stat', 'assembly_list', 'species_align_stat'):
            _equal_frames(getattr(dev, attr), getattr(host, attr))
        assert (dev.num_species_reached_min_average_depth, dev.num_species_not_reached) == (host.num_species_reached_min_average_depth, host.num_species_not_reached)
        # the statistic per assembly through mpn_good_rows and mpn_sum_by_key is the existing one through mpn_cover_by_group alone
        _equal_frames(dev.align_stat, abundance.align_stat_by_assembly_id(dev.good_align_list, inp['assembly_length'], inp['assembly_tax'], device=True))
    rec = golden()[0]
    inp = selection_inputs(rec['case'])
    empty = inp['species_align_list'].iloc[0:0]
    assert abundance.good_align_list(align_list=empty, good_align_threshold=90).shape[0] == 0 and abundance.best_align_per_read(empty).shape[0] == 0
    _equal_frames(abundance.align_stat_by_sequence_id(inp['species_align_list'], inp['sequence_length']),                      # device=None is the device
                  abundance.align_stat_by_sequence_id(inp['species_align_list'], inp['sequence_length'], device=False))


def test_bad_arguments_return_minus_two_and_leave_the_outputs_untouched(libmpn):
    from megapath_nano_amd import _ffi, abundance
    lib = abundance._lib()
    read, unit = np.array([0, 1, 1], np.int32), np.array([0, 1, 0], np.int32)
    score, tiebreak = np.array([5, 5, 6], np.int64), np.array([0.5, 0.5, 0.25], np.float64)

    def good(read=read, unit=unit, score=score, tiebreak=tiebreak, use=1, threshold=0.9, n=3):
        out, best, n_good = np.full(4, -7, np.int64), np.full(2, -7, np.int64), ct.c_int64(-7)
        rc = lib.mpn_good_rows(n, read.ctypes.data, unit.ctypes.data, score.ctypes.data, tiebreak.ctypes.data, 2, 2, use, threshold, out.ctypes.data,
                               ct.byref(n_good), best.ctypes.data)
        return rc, bool((out == -7).all() and (best == -7).all() and n_good.value == -7), n_good.value, out[:2].tolist(), best.tolist()

    assert good() == (0, False, 2, [0, 2], [5, 6])
    for bad, where in ((dict(threshold=float('nan')), 'finite threshold'), (dict(threshold=float('inf')), 'finite threshold'),
                       (dict(threshold=float('nan'), use=0), 'finite threshold'), (dict(n=-1), 'bad arguments'),
                       (dict(score=np.array([5, 2 ** 53, 6], np.int64)), 'record 1'), (dict(score=np.array([5, 5, -2 ** 53], np.int64)), 'record 2'),
                       (dict(read=np.array([0, 2, 1], np.int32)), 'record 1'), (dict(unit=np.array([-1, 1, 0], np.int32)), 'record 0'),
                       (dict(tiebreak=np.array([0.5, 0.5, np.nan])), 'record 2')):
        rc, untouched = good(**bad)[:2]
        assert rc == -2 and untouched and where in _ffi.last_error(), bad

    key, cols = np.array([0, 1, 1], np.int32), np.array([1, 2, 3, 10, 20, 30], np.int64)

    def sums(key=key, cols=cols, n_cols=2, n_keys=2):
        count, out = np.full(3, -7, np.int64), np.full(16, -7, np.int64)
        rc = lib.mpn_sum_by_key(3, key.ctypes.data, n_keys, n_cols, cols.ctypes.data, count.ctypes.data, out.ctypes.data)
        return rc, bool((count == -7).all() and (out == -7).all()), count[:2].tolist(), out[:4].tolist()

    assert sums() == (0, False, [1, 2], [1, 5, 10, 50])
    wide = np.zeros(21, np.int64)
    for bad, where in ((dict(cols=wide, n_cols=7), 'bad arguments'), (dict(n_cols=0), 'bad arguments'), (dict(key=np.array([0, 2, 1], np.int32)), 'record 1'),
                       (dict(key=np.array([0, 1, -1], np.int32)), 'record 2'), (dict(cols=np.array([1, 2, 3, 10, 2 ** 32, 30], np.int64)), 'record 1'),
                       (dict(cols=np.array([-2 ** 32, 2, 3, 10, 20, 30], np.int64)), 'record 0')):
        rc, untouched = sums(**bad)[:2]
        assert rc == -2 and untouched and where in _ffi.last_error(), bad
    with pytest.raises(_ffi.MpnError):
        abundance.device_good_rows([0], [0], [1], [0.5], 1, 1, threshold=float('nan'))
    with pytest.raises(_ffi.MpnError):
        abundance.device_good_rows([0], [0], [2 ** 53], [0.5], 1, 1)
    with pytest.raises(_ffi.MpnError):
        abundance.device_sum_by_key([0], 1, [[1]] * 7)
    with pytest.raises(_ffi.MpnError):
        abundance.device_sum_by_key([2], 2, [[1]])
