"""GPU tests (-m gpu) of mpn_best_candidates, mpn_pick_weighted and mpn_second_best_by_read (include/mpn_abundance.h;
csrc/interval_kernels.hip): every entry must equal its numpy statement as arrays -- order, integer widths and the bits of every
double included -- on random small cases that also go against plain loops, on tiny inputs, at row counts around the multiples of
the scans' tile, with one read through hundreds of tiles beside thousands of one-row reads, at both ends of the score domain and
with tiebreakers, weights and draws at the edges of theirs; and the mirrors of the reference's align_list_to_best_align_list,
step_short_alignment_removal, step_unique_alignment and step_closing_spike_filter must equal their host forms and the goldens made
by the reference's own functions."""
import ctypes as ct

import numpy as np
import pandas as pd
import pytest

from best_cases import (BELOW_ONE, LENGTHS, TINY, best_table, brute_candidates, brute_pick, brute_second, check_against_brute_force, check_against_golden,
                        counter_rng, golden, golden_cases, noise_bed_for, random_pick_case, random_small_case, read_classes)

pytestmark = pytest.mark.gpu


def _same(dev, host):
    """equal as arrays: lengths, order, dtypes; doubles bit for bit"""
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x,
                                                                            y.view(np.int64) if y.dtype == np.float64 else y) for x, y in zip(dev, host))


def _brief(arg):
    return {k: (v if np.ndim(v) == 0 or len(v) < 40 else f'[{len(v)}]') for k, v in arg.items()}


def _cands(**arg):
    from megapath_nano_amd.abundance import device_best_candidates, host_best_candidates
    dev, host = device_best_candidates(**arg), host_best_candidates(**arg)
    assert _same(dev, host), _brief(arg)
    return dev


def _pick(**arg):
    from megapath_nano_amd.abundance import device_pick_weighted, host_pick_weighted
    dev, host = device_pick_weighted(**arg), host_pick_weighted(**arg)
    assert _same(dev, host), _brief(arg)
    return dev


def _second(**arg):
    from megapath_nano_amd.abundance import device_second_best_by_read, host_second_best_by_read
    dev, host = device_second_best_by_read(**arg), host_second_best_by_read(**arg)
    assert _same([dev], [host]), _brief(arg)
    return dev


def _rows(read, assembly, score, tiebreak, n_reads, n_assemblies):
    return dict(read=np.asarray(read, np.int32), assembly=np.asarray(assembly, np.int32), score=np.asarray(score, np.int64),
                tiebreak=np.asarray(tiebreak, np.float64), n_reads=n_reads, n_assemblies=n_assemblies)


def test_device_equals_host_equals_the_loops_on_small_cases(libmpn):
    rng = np.random.default_rng(61)
    several = 0
    for trial in range(150):
        c = random_small_case(rng)
        got = _cands(**c)
        assert [[int(v) for v in a] for a in got] == [list(w) for w in brute_candidates(c['read'], c['assembly'], c['score'], c['tiebreak'], c['n_reads'])], trial
        p = random_pick_case(rng, got[1], c['n_reads'])
        new, winner = _pick(**p)
        want_new, want_winner = brute_pick(p['read'], p['weight'], p['tiebreak'], p['draw'], p['n_reads'])
        assert [x.hex() for x in new.tolist()] == [x.hex() for x in want_new] and winner.tolist() == want_winner, trial
        several += int((got[2] > 1).sum())
        excluded = rng.integers(-1, c['n_assemblies'], size=c['n_reads']).astype(np.int32)
        second = _second(read=c['read'], assembly=c['assembly'], score=c['score'], n_reads=c['n_reads'], excluded=excluded)
        assert second.tolist() == brute_second(c['read'], c['assembly'], c['score'], c['n_reads'], excluded), trial
    assert several > 100


def test_tiny_inputs_and_the_tie_rules(libmpn):
    row, rd, count, first = _cands(**_rows([], [], [], [], 3, 2))                                          # n = 0
    assert len(row) == 0 and len(rd) == 0 and count.tolist() == [0, 0, 0] and first.tolist() == [0, 0, 0]
    assert [a.tolist() for a in _cands(**_rows([], [], [], [], 0, 0))] == [[], [], [], []]
    assert [a.tolist() for a in _cands(**_rows([2], [1], [-5], [0.5], 4, 2))] == [[0], [2], [0, 0, 1, 0], [0, 0, 0, 1]]     # n = 1
    assert [a.tolist() for a in _cands(**_rows([0], [0], [7], [0.0], 1, 1))] == [[0], [0], [1], [0]]      # one read with one row
    # every row of one read on one assembly: the largest (score, tiebreak), the last of the equal ones
    assert _cands(**_rows([0] * 6, [3] * 6, [5, 9, 9, 9, 2, 9], [0.9, 0.4, 0.7, 0.1, 0.9, 0.7], 1, 4))[0].tolist() == [5]
    # every row identical in score and tiebreak: the last input row of every assembly; then the last assembly wins the equal draws
    row, rd, count, _ = _cands(**_rows([0] * 6, [2, 1, 2, 1, 0, 0], [9] * 6, [0.5] * 6, 1, 3))
    assert row.tolist() == [5, 3, 2] and count.tolist() == [3]
    new, winner = _pick(read=rd, weight=[0, 0, 0], tiebreak=[0.5] * 3, draw=[0.25] * 3, n_reads=1)
    assert new.tolist() == [0.25] * 3 and winner.tolist() == [2]
    assert _cands(**_rows([0, 0], [0, 0], [1, 1], [0.0, -0.0], 1, 1))[0].tolist() == [1]                   # -0.0 == 0.0: the later row
    assert _cands(**_rows([0, 0], [0, 0], [1, 1], [-0.0, 0.0], 1, 1))[0].tolist() == [1]
    new, winner = _pick(read=[], weight=[], tiebreak=[], draw=[], n_reads=2)                              # no candidates
    assert len(new) == 0 and winner.tolist() == [-1, -1]
    assert _pick(read=[1], weight=[0], tiebreak=[0.75], draw=[0.5], n_reads=3)[1].tolist() == [-1, 0, -1]
    assert _second(read=[], assembly=[], score=[], n_reads=2, excluded=[-1, 0]).tolist() == [0, 0]
    assert _second(read=[0, 0, 1, 2], assembly=[0, 1, 1, 0], score=[9, -4, 6, 5], n_reads=4, excluded=[0, 1, -1, -1]).tolist() == [-4, 0, 5, 0]


def test_both_ends_of_the_score_and_tiebreak_domains(libmpn):
    top, bottom = 2 ** 63 - 1, -(2 ** 63) + 1
    # read 0: the top score on two assemblies; read 1: only bottom scores, told apart by denormal tiebreakers; read 2: tiebreakers at
    # 0.0, just below 1 and denormal on one assembly
    got = _cands(**_rows([0, 0, 0, 1, 1, 1, 2, 2, 2, 2], [0, 1, 2, 0, 0, 1, 0, 0, 0, 0], [top, top - 1, top, bottom, bottom, bottom, 3, 3, 3, 3],
                         [0.5, 0.5, 0.0, TINY, 2 * TINY, 0.0, 0.0, BELOW_ONE, TINY, 1.0 - 2.0 ** -52], 3, 3))
    assert [a.tolist() for a in got] == [[0, 2, 4, 5, 7], [0, 0, 1, 1, 2], [2, 2, 1], [0, 2, 4]]
    assert _second(read=[0, 0, 1, 1], assembly=[0, 1, 0, 1], score=[top, bottom, bottom, top], n_reads=2, excluded=[0, 1]).tolist() == [bottom, bottom]
    # the draw: a read whose weights are all 0, one weight 0 among positive ones, sums near 2^52, draws at 0.0, below 1 and denormal
    big = 2 ** 52 - 1
    new, winner = _pick(read=[0, 0, 0, 1, 1, 1, 2, 2, 3, 3, 3, 5], weight=[0, 0, 0, 3, 0, 1, big, big, big, 1, big - 1, 7],
                        tiebreak=[0.9] * 11 + [0.125], draw=[0.25, BELOW_ONE, TINY, 0.5, BELOW_ONE, 0.5, TINY, BELOW_ONE, 1 / 3, BELOW_ONE, 2 / 3, 0.7], n_reads=6)
    assert new[:6].tolist() == [0.25, BELOW_ONE, TINY, 0.375, 0.0, 0.125] and new[11] == 0.125 and winner.tolist() == [1, 3, 7, 10, -1, 11]


def _sizes():
    from megapath_nano_amd.abundance import BEST_TILE
    return sorted({t * BEST_TILE + d for t in (1, 2, 3, 5) for d in (-1, 0, 1)})


def test_row_counts_around_the_tile_boundaries(libmpn):
    rng = np.random.default_rng(62)
    for n in _sizes():
        # (a) about seven rows a read on six assemblies, scores from four adjacent values, tiebreakers that repeat
        n_reads = n // 7 + 1
        c = _rows(rng.integers(0, n_reads, size=n), rng.integers(0, 6, size=n), -2 + rng.integers(0, 4, size=n), rng.integers(0, 4, size=n) / 4, n_reads, 6)
        row, rd, count, first = _cands(**c)
        assert (count == 1).sum() > n_reads // 4 and (count > 1).sum() > n_reads // 4 and count.sum() == len(row)
        _second(read=c['read'], assembly=c['assembly'], score=c['score'], n_reads=n_reads, excluded=rng.integers(-1, 6, size=n_reads).astype(np.int32))
        # (b) one read on one assembly through every tile: all rows identical -> the last row; one larger row somewhere -> that row
        same = _rows(np.zeros(n), np.zeros(n), np.full(n, 5), np.full(n, 0.5), 1, 1)
        assert _cands(**same)[0].tolist() == [n - 1]
        at = int(rng.integers(0, n))
        same['tiebreak'][at] = 0.75
        assert _cands(**same)[0].tolist() == [at]
        # (c) every row identical, three assemblies in turn: the last row of each, ordered by assembly
        turn = _rows(np.zeros(n), np.arange(n) % 3, np.full(n, 5), np.full(n, 0.5), 1, 3)
        assert _cands(**turn)[0].tolist() == sorted(range(n - 3, n), key=lambda i: i % 3)
        # (d) every row a read of its own, in reverse: n candidates, nothing may be carried from read to read
        own = _rows(np.arange(n)[::-1], rng.integers(0, 6, size=n), rng.integers(-9, 9, size=n), rng.random(n), n, 6)
        row, rd, count, first = _cands(**own)
        assert np.array_equal(row, np.arange(n)[::-1]) and (count == 1).all()
        # the draw over n candidates: reads of one to five candidates, one read from the middle of a tile to the end
        read = np.repeat(np.arange(n), rng.integers(1, 6, size=n))[:n]
        read[n // 2:] = read[n // 2]
        weight = np.where(rng.random(n) < 0.2, 0, rng.integers(0, 2 ** 38, size=n))              # the long read's sum stays below 2^51
        new, winner = _pick(read=read.astype(np.int32), weight=weight, tiebreak=rng.random(n), draw=rng.integers(0, 64, size=n) / 64, n_reads=int(read.max()) + 1)
        assert (winner >= 0).all() and (new[read == read[-1]] <= new[winner[read[-1]]]).all()


def test_one_read_through_hundreds_of_tiles_beside_thousands_of_one_row_reads(libmpn):
    """700 000 rows: read 100 000 holds 500 000 of them on six assemblies (244 tiles; every (read, assembly) group runs through
    about 40 and straddles tile edges), 200 000 reads hold one row each, before and behind it in the order of the codes; the input
    order is shuffled, so rows that end up adjacent come from all over the input."""
    rng = np.random.default_rng(63)
    big, n_big, n_reads = 100000, 500000, 200001
    read = np.concatenate([np.full(n_big, big), np.delete(np.arange(n_reads), big)]).astype(np.int32)
    order = rng.permutation(len(read))
    read = read[order]
    n = len(read)
    c = _rows(read, rng.integers(0, 6, size=n), rng.integers(-3, 1, size=n), rng.integers(0, 8, size=n) / 8, n_reads, 6)
    row, rd, count, first = _cands(**c)
    assert count[big] == 6 and (np.delete(count, big) == 1).all() and first[big] == big and first[-1] == n_reads + 4
    mine = row[first[big]:first[big] + 6]
    assert (c['score'][mine] == 0).all() and (c['tiebreak'][mine] == 0.875).all() and c['assembly'][mine].tolist() == [0, 1, 2, 3, 4, 5]
    for a, i in enumerate(mine):                                     # the last input row among the equal ones
        assert i == np.flatnonzero((read == big) & (c['assembly'] == a) & (c['score'] == 0) & (c['tiebreak'] == 0.875))[-1]
    excluded = np.full(n_reads, -1, dtype=np.int32)
    excluded[big], excluded[5] = 3, int(c['assembly'][read == 5][0])
    second = _second(read=read, assembly=c['assembly'], score=c['score'], n_reads=n_reads, excluded=excluded)
    assert second[big] == 0 and second[5] == 0
    # the draw: one read of 500 000 candidates (the entry's domain allows it) between reads of one and of two
    cand_read = np.sort(np.concatenate([np.full(n_big, big), np.arange(n_reads), np.arange(0, n_reads, 2)])).astype(np.int32)
    m = len(cand_read)
    new, winner = _pick(read=cand_read, weight=rng.integers(0, 2 ** 33, size=m), tiebreak=rng.random(m), draw=rng.random(m), n_reads=n_reads)
    assert (winner >= 0).all() and new[winner[big]] == new[cand_read == big].max()


def test_quotients_and_products_are_numpy_s_bit_for_bit(libmpn):
    """300 000 candidates in reads of two to six: weights from 0 to 2^50 (sums stay below 2^53), every draw a random double, some
    denormal -- one rounding of the division or the product done another way would show in a last bit somewhere"""
    rng = np.random.default_rng(64)
    read = np.repeat(np.arange(100000), rng.integers(2, 7, size=100000))[:300000].astype(np.int32)
    m = len(read)
    weight = np.where(rng.random(m) < 0.1, 0, rng.integers(0, 2 ** 50, size=m) >> rng.integers(0, 50, size=m))
    draw = np.where(rng.random(m) < 0.05, rng.integers(1, 2 ** 40, size=m) * TINY, rng.random(m))
    new, winner = _pick(read=read, weight=weight, tiebreak=rng.random(m), draw=draw, n_reads=100000)
    assert len(np.unique(new)) > m // 2 and (new == 0).sum() > m // 20


def test_bad_arguments_return_minus_two_and_leave_the_outputs_untouched(libmpn):
    from megapath_nano_amd import _ffi, abundance
    lib = abundance._lib()
    read, assembly = np.array([0, 1, 1], np.int32), np.array([0, 1, 0], np.int32)
    score, tiebreak = np.array([5, 5, 6], np.int64), np.array([0.5, 0.5, 0.25], np.float64)

    def cands(read=read, assembly=assembly, score=score, tiebreak=tiebreak):
        out = [np.full(4, -7, np.int64), np.full(4, -7, np.int32), np.full(2, -7, np.int64), np.full(2, -7, np.int64)]
        n_cand = ct.c_int64(-7)
        rc = lib.mpn_best_candidates(3, read.ctypes.data, assembly.ctypes.data, score.ctypes.data, tiebreak.ctypes.data, 2, 2, out[0].ctypes.data,
                                     out[1].ctypes.data, ct.byref(n_cand), out[2].ctypes.data, out[3].ctypes.data)
        return rc, all((a == -7).all() for a in out) and n_cand.value == -7, n_cand.value, out[0][:2].tolist()

    assert cands() == (0, False, 2, [0, 2])
    for bad, where in ((dict(read=np.array([0, 2, 1], np.int32)), 'record 1'), (dict(read=np.array([0, 1, -1], np.int32)), 'record 2'),
                       (dict(assembly=np.array([2, 1, 0], np.int32)), 'record 0'), (dict(score=np.array([5, -2 ** 63, 6], np.int64)), 'record 1'),
                       (dict(tiebreak=np.array([0.5, 0.5, np.nan])), 'record 2'), (dict(tiebreak=np.array([np.inf, 0.5, 0.5])), 'record 0')):
        rc, untouched = cands(**bad)[:2]
        assert rc == -2 and untouched and where in _ffi.last_error(), bad

    c_read, weight, draw = np.array([0, 0, 1], np.int32), np.array([1, 3, 0], np.int64), np.array([0.5, 0.5, 0.5], np.float64)

    def pick(read=c_read, weight=weight, tiebreak=tiebreak, draw=draw):
        new, winner = np.full(4, -7.0), np.full(3, -7, np.int64)
        rc = lib.mpn_pick_weighted(3, read.ctypes.data, weight.ctypes.data, tiebreak.ctypes.data, draw.ctypes.data, 2, new.ctypes.data, winner.ctypes.data)
        return rc, bool((new == -7).all() and (winner == -7).all()), new[:3].tolist(), winner[:2].tolist()

    assert pick() == (0, False, [0.125, 0.375, 0.25], [1, 2])
    for bad, where in ((dict(read=np.array([1, 0, 1], np.int32)), 'candidate 1'), (dict(read=np.array([0, 0, 2], np.int32)), 'candidate 2'),
                       (dict(weight=np.array([1, -1, 0], np.int64)), 'candidate 1'), (dict(weight=np.array([2 ** 52, 2 ** 52, 0], np.int64)), 'candidate 1'),
                       (dict(draw=np.array([0.5, np.nan, 0.5])), 'candidate 1'), (dict(tiebreak=np.array([0.5, 0.5, -np.inf])), 'candidate 2')):
        rc, untouched = pick(**bad)[:2]
        assert rc == -2 and untouched and where in _ffi.last_error(), bad

    excluded = np.array([1, -1], np.int32)

    def second(read=read, assembly=assembly, score=score, excluded=excluded):
        out = np.full(3, -7, np.int64)
        rc = lib.mpn_second_best_by_read(3, read.ctypes.data, assembly.ctypes.data, score.ctypes.data, 2, excluded.ctypes.data, out.ctypes.data)
        return rc, bool((out == -7).all()), out[:2].tolist()

    assert second() == (0, False, [5, 6])
    for bad, where in ((dict(read=np.array([0, 2, 1], np.int32)), 'record 1'), (dict(assembly=np.array([0, 1, -1], np.int32)), 'record 2'),
                       (dict(score=np.array([-2 ** 63, 5, 6], np.int64)), 'record 0'), (dict(excluded=np.array([1, -2], np.int32)), 'read 1')):
        rc, untouched = second(**bad)[:2]
        assert rc == -2 and untouched and where in _ffi.last_error(), bad
    with pytest.raises(_ffi.MpnError):
        abundance.device_best_candidates([0], [3], [1], [0.5], 1, 2)
    with pytest.raises(_ffi.MpnError):
        abundance.device_pick_weighted([1, 0], [1, 1], [0.5, 0.5], [0.5, 0.5], 2)


def test_mirrors_on_the_device_equal_the_goldens_the_loops_and_their_host_forms(libmpn):
    from megapath_nano_amd import abundance
    for rec in golden():
        check_against_golden(rec, device=True)
    draws = 0
    for case in golden_cases():
        table = best_table(**case['table'])
        noise = noise_bed_for(table, case['noise_seed']) if 'noise_seed' in case else None
        draws += check_against_brute_force(table, noise, device=True)
    assert draws > 500
    table = best_table(seed=91, n_reads=300)
    one, several, without = read_classes(table)
    assert one >= 75 and several >= 75 and 'A6' in without
    noise = noise_bed_for(table, 7)
    kw = dict(align_list=table, assembly_length=LENGTHS, noise_bed=noise)
    host = abundance.align_list_to_best_align_list(rng=counter_rng(), device=False, **kw)
    for device in (True, None):                                                                     # None is the device
        rng = counter_rng()
        pd.testing.assert_frame_equal(abundance.align_list_to_best_align_list(rng=rng, device=device, **kw), host)
        assert rng.calls > several * 2 - 1
    assert host.shape[0] == one + several
    dev = abundance.short_alignment_removal(align_list=table, min_align_length=900, assembly_length=LENGTHS, rng=counter_rng(), device=True)
    hst = abundance.short_alignment_removal(align_list=table, min_align_length=900, assembly_length=LENGTHS, rng=counter_rng(), device=False)
    pd.testing.assert_frame_equal(dev[0], hst[0])
    assert dev[1:] == hst[1:] and 0 < dev[2] < dev[1]
    dev = abundance.unique_alignment(align_list=table, best_align_list=host, unique_align_threshold=99.9, device=True)
    hst = abundance.unique_alignment(align_list=table, best_align_list=host, unique_align_threshold=99.9, device=False)
    pd.testing.assert_frame_equal(dev[0], hst[0])
    assert dev[1:] == hst[1:] and 0 < dev[2] < dev[1]
    short = table[(table['sequence_to'] - table['sequence_from']) >= 400]
    arg = dict(align_list=short, align_list_with_short_alignment=table, noise_bed=noise, assembly_length=LENGTHS, max_align_noise_overlap=30, expected_max_depth_stdev=1)
    dev, hst = abundance.closing_spike_step(rng=counter_rng(), device=True, **arg), abundance.closing_spike_step(rng=counter_rng(), device=False, **arg)
    for d, h in zip(dev[:4], hst[:4]):
        pd.testing.assert_frame_equal(d, h)
    assert dev[4:] == hst[4:] and 0 < dev[5] <= dev[4]
