"""CPU test: the rules of the device BAM writer (csrc/bam_out_core.h), built for the host with g++ (scripts/bam_out_host_check.cpp, under
AddressSanitizer and UBSan where the toolchain has their runtimes).  Scan + encode of SAM lines against bam.encode_record byte for
byte, every refusal with its status, the BGZF block cut and the BAI builder against bam.BgzfWriter / bam.BaiBuilder on the same
sizes and stored-mode offsets -- before any of it meets a GPU."""
import pytest

import bam_out_cases as bc
from megapath_nano_amd import bam


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return bc.build_host_check(tmp_path_factory.mktemp('bam_out_host'))


def check_equal(got, lines):
    for g, l in zip(got, lines):
        tid, pos0, end0, flag, rec = bc.expected(l)
        assert g[0] == bc.OK, (l[:80], g[0])
        assert g[1:5] == (tid, pos0, end0, flag), l[:80]
        assert g[5] == rec, l[:80]


def test_records_equal_encode_record(exe, tmp_path):
    lines = bc.good_lines()
    got = bc.host_encode(exe, tmp_path, lines)
    assert len(got) == len(lines)
    check_equal(got, lines)


def test_lines_without_a_line_feed_encode_alike(exe, tmp_path):
    lines = [l.rstrip(b'\n') for l in bc.basic_lines()]
    check_equal(bc.host_encode(exe, tmp_path, lines), lines)


def test_every_four_digit_fraction_is_the_float_strtod_gives(exe, tmp_path):
    lines = bc.float_lines()
    check_equal(bc.host_encode(exe, tmp_path, lines), lines)


def test_refusals_carry_their_status(exe, tmp_path):
    cases = bc.refused_lines()
    got = bc.host_encode(exe, tmp_path, [l for l, _ in cases])
    assert [(g[0], len(g[5])) for g in got] == [(st, 0) for _, st in cases]
    assert {st for _, st in cases} == set(range(bc.FEW_FIELDS, bc.CR + 1))          # every refusal of a line is among the cases


def test_skipped_and_excluded_lines_have_no_record(exe, tmp_path):
    cases = bc.skipped_lines()
    got = bc.host_encode(exe, tmp_path, [l for l, _ in cases], exclude_flags=1028)
    assert [(g[0], len(g[5])) for g in got] == [(st, 0) for _, st in cases]


def test_unknown_references_without_any_reference(exe, tmp_path):
    lines = [bc.line(rname='t1', rnext='t2'), bc.line(rname='*')]
    got = bc.host_encode(exe, tmp_path, lines, refs=[])
    assert [(g[0], g[1]) for g in got] == [(bc.OK, -1), (bc.OK, -1)]
    assert [g[5] for g in got] == [bam.encode_record(l.decode().rstrip('\n').split('\t'), {})[4] for l in lines]


@pytest.fixture(scope='module')
def cut_results(exe, tmp_path_factory):
    tmp = tmp_path_factory.mktemp('bam_out_cut')
    cases = bc.cut_cases() + [bc.index_sam_case()]
    want = [bc.python_cut(tmp, c) for c in cases]
    got = bc.host_index(exe, tmp, [(len(names), bc.header_bytes(text, names, lens), [(t, p, e, s, 0 if f & 4 else 1) for t, p, e, f, s in recs])
                                  for _, text, names, lens, recs in cases])
    return {c[0]: (c, w, g) for c, w, g in zip(cases, want, got)}


CUT_NAMES = ['fills_a_block', 'one_byte_over', 'after_some_then_exact', 'large_then_small', 'multiple_of_block', 'header_over_a_block', 'no_records',
             'unplaced_only', 'spread', 'index_sam']


@pytest.mark.parametrize('name', CUT_NAMES)
def test_cut_and_index_equal_the_python_writer(cut_results, name):
    case, (sizes, bai), (starts, first, end, voff, got_bai) = cut_results[name]
    assert [b - a for a, b in zip(starts, starts[1:])] == sizes
    assert all(0 < s <= bam.BGZF_BLOCK for s in sizes)
    assert first >> 16 == -(-bc.header_bytes(*case[1:4]) // bam.BGZF_BLOCK) and first & 0xffff == 0
    assert end == len(sizes) << 16
    assert got_bai == bai


def test_cut_cases_reach_the_edges(cut_results):
    B = bam.BGZF_BLOCK
    sizes = {n: cut_results[n][1][0] for n in CUT_NAMES}
    # one byte over: a full block, and the records behind go on in the block that holds the last byte
    behind = sum(4 + r[4] for r in cut_results['one_byte_over'][0][4][4:])
    assert sizes['fills_a_block'][1] == B and sizes['one_byte_over'][2:4] == [B, 1 + behind]
    assert sizes['after_some_then_exact'][1] == B
    assert sizes['large_then_small'][1:4] == [B, B, B] and sizes['large_then_small'][4] > 200004 - 3 * B
    assert len(sizes['header_over_a_block']) == 3 and sizes['header_over_a_block'][0] == B
    assert len(sizes['no_records']) == 1 and len(sizes['spread']) > 100
    assert len(cut_results['index_sam'][0][4]) > 0


def test_two_references_of_one_name_are_refused_before_anything_is_loaded():
    with pytest.raises(bam.DeviceRefused):
        bam.DeviceBamBuilder(['t1', 't2', 't1'], [5, 6, 7], '@HD\tVN:1.6\tSO:coordinate\n')
