"""GPU tests of megapath_nano_amd/read_realign.py against the restatement (tests/read_realign_ref.py): the rows of the counter, the
windows, the memberships and the final lines are compared separately, on constructed files (tests/read_realign_cases.py) that
reach the edges: CIGARs of 63, 64, 65 and 130 operations; insertions and soft clips of 65 and 130 bases with one base of quality
19 in the last step; counts and indels at the borders of a chunk's row and region; negative positions and the wrapped base before
position 0; a clip that reaches back into the row before; lagging chunks behind a gap of 11 000 bases; a dropped record that
triggers a yield; MAPQ 13 / 14 and 19 / 20; N, H and P; lower-case contig bases; IUPAC read bases; a candidate in a split overlap;
windows 160 and 161 apart, of 1000 and 1001 bases, with 1001 reads; overlap ties; a row over one, two and many workgroups; HP tags
of each integer type; a chunk that spans two texts.  All comparisons are exact."""
import io
import random

import numpy as np
import pytest

import read_realign_cases as rc
import read_realign_ref as ref

pytestmark = pytest.mark.gpu

CASES = rc.edge_cases() + [rc.plain_variants(), rc.deep_window()]
_cache = {}


@pytest.fixture(scope='module')
def rr(libmpn, oracle_built):
    from megapath_nano_amd import read_realign
    return read_realign


def both(rr, tmp_path_factory, case, env=None):
    """-> (the restatement's lines and trace, the product's text, trace and counts, its timings), computed once per case"""
    key = (case['name'], tuple(sorted((env or {}).items())))
    if key not in _cache:
        name = case['name']
        if name not in _cache:
            want_trace = []
            _cache[name] = (ref.realign(rc.sam_lines(case), case['contig'], rc.CTG, case['min_mq'], case['min_coverage'], trace=want_trace), want_trace)
        bam_fn, ref_fn = rc.write_case(tmp_path_factory.mktemp(name), case)
        out, trace, timings = io.BytesIO(), [], {}
        with pytest.MonkeyPatch.context() as mp:
            for k, v in (env or {}).items():
                mp.setenv(k, v)
            got = rr.realign_file(bam_fn, ref_fn, rc.CTG, out, min_mq=case['min_mq'], min_coverage=case['min_coverage'], trace=trace, timings=timings)
        _cache[key] = (_cache[name], out.getvalue().decode('latin-1'), trace, got, timings)
    return _cache[key]


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_rows(rr, tmp_path_factory, case):
    (_, want), _, trace, _, _ = both(rr, tmp_path_factory, case)
    assert [t['chunk_start'] for t in trace] == [w['chunk_start'] for w in want]
    for t, w in zip(trace, want):
        assert np.array_equal(t['row'], np.asarray(w['row'], dtype=np.int32)), (case['name'], t['chunk_start'])
    assert any(np.any(t['row']) for t in trace)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_windows(rr, tmp_path_factory, case):
    (_, want), _, trace, _, _ = both(rr, tmp_path_factory, case)
    assert [t['windows'] for t in trace] == [w['windows'] for w in want]


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_memberships(rr, tmp_path_factory, case):
    (_, want), _, trace, _, _ = both(rr, tmp_path_factory, case)
    for t, w in zip(trace, want):
        if w['members'] is None:
            assert t['members'] is None
            continue
        assert t['members'] == [m or [[] for _ in s] for m, s in zip(w['members'], w['windows'])], (case['name'], t['chunk_start'])


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_lines(rr, tmp_path_factory, case):
    (lines, _), text, _, got, _ = both(rr, tmp_path_factory, case)
    assert text == rc.header_text(case) + ''.join(lines)
    assert got['reads'] == len(lines) and got['viewed'] == len([r for r in case['records'] if r['mapq'] >= case['min_mq']])


def test_the_cases_reach_what_they_are_for(rr, tmp_path_factory):
    """a read whose CIGAR changes, one realigned in two windows of overlapping splits, a window of 1000 reads cut from 1001"""
    by_name = {c['name']: c for c in CASES}
    (lines, _), _, _, got, _ = both(rr, tmp_path_factory, by_name['plain_variants_21'])
    assert got['changed'] > 0
    (_, want), _, trace, _, _ = both(rr, tmp_path_factory, by_name['windows'])
    first = trace[0]
    assert first['windows'][0][-1] == first['windows'][1][0] == (910, 1080)                  # the candidates 990 and 1000 belong to both splits
    assert first['members'][0][-1] == first['members'][1][0] and len(first['members'][0][-1]) >= 4
    assert (3020, 3180) in first['windows'][3] and (3181, 3341) in first['windows'][3] and (2020, 2340) in first['windows'][2]
    assert trace[1]['windows'][0] == [(5020, 6020)] and trace[2]['windows'][0] == [(10020, 11021)]
    _, _, trace, got, _ = both(rr, tmp_path_factory, by_name['deep_window'])
    assert max(len(m) for t in trace if t['members'] for s in t['members'] for m in s) == 1001


@pytest.mark.parametrize('slice_', ['1', '100', '100000'])
def test_a_row_over_one_two_and_many_workgroups(rr, tmp_path_factory, slice_):
    """the one row of plain_variants with a workgroup per record, with several of at most 100 records, and with one"""
    case = rc.plain_variants()
    (_, want), text, trace, _, _ = both(rr, tmp_path_factory, case, {'MPN_RR_SLICE': slice_})
    for t, w in zip(trace, want):
        assert np.array_equal(t['row'], np.asarray(w['row'], dtype=np.int32))
    assert text == both(rr, tmp_path_factory, case)[1]


def test_support_splits_rows_as_told(rr, tmp_path):
    """mpn_rr_support itself: the number of split rows, and the same counters bit for bit however the row is sliced"""
    import torch
    from megapath_nano_amd import ingest
    case = rc.plain_variants()
    bam_fn, _ = rc.write_case(tmp_path, case)
    contig = torch.from_numpy(np.frombuffer(case['contig'].upper().encode(), dtype=np.uint8).copy()).cuda()
    with ingest.BamTexts(bam_fn) as texts:
        t = next(texts)
        recs = rr.rr_records(t.text, t.text_len, t.rows)
        keep = np.flatnonzero(recs['mapq'] >= 20)
        takes = np.zeros(len(keep), dtype=rr.RR_TAKE)
        takes['off'], takes['pos'] = t.rows['off'][keep], recs['pos'][keep]
        reach = recs['l_seq'][keep].astype(np.int64) + recs['span'][keep]
        rows = []
        assert len(keep) > 2
        for slice_, n_split in ((0, int(len(keep) > 256)), (1, 1), (len(keep), 0), (len(keep) - 1, 1)):
            d = torch.zeros((1, rr.ROW), dtype=torch.int32, device='cuda')
            bad, split = rr.rr_support(t.text, t.text_len, takes, reach, [0], [-21], contig, d, slice_)
            assert bad == -1 and split == n_split
            rows.append(d.cpu().numpy())
        assert all(np.array_equal(rows[0], r) for r in rows[1:]) and rows[0].any()


def test_a_chunk_that_spans_two_texts(rr, tmp_path_factory):
    case = rc.plain_variants(seed=33, n=9000, depth=25)
    (lines, want), text, trace, _, timings = both(rr, tmp_path_factory, case, {'MPN_INGEST_BATCH_BYTES': '1'})
    assert timings['walk_launches'] >= 3                                  # one text per BGZF block
    for t, w in zip(trace, want):
        assert np.array_equal(t['row'], np.asarray(w['row'], dtype=np.int32)), t['chunk_start']
        assert t['windows'] == w['windows']
    assert text == rc.header_text(case) + ''.join(lines)


def test_region_test_of_an_indel_on_both_sides(rr, tmp_path):
    """mpn_rr_support with a chunk_start of the caller's: a deletion at chunk_start - 21 / - 20 and chunk_end + 20 / + 21"""
    import torch
    from megapath_nano_amd import ingest
    ctg, rng = rc.contig(12000, 41), random.Random(42)
    case = rc.case('region', ctg, [rc.read(ctg, p - 30, '30M3D30M', rng) for p in (5979, 5980, 11020, 11021)])
    bam_fn, _ = rc.write_case(tmp_path, case)
    contig = torch.from_numpy(np.frombuffer(ctg.encode(), dtype=np.uint8).copy()).cuda()
    with ingest.BamTexts(bam_fn) as texts:
        t = next(texts)
        recs = rr.rr_records(t.text, t.text_len, t.rows)
        takes = np.zeros(4, dtype=rr.RR_TAKE)
        takes['off'], takes['pos'], takes['chunk_start'] = t.rows['off'], recs['pos'], 6000
        d = torch.zeros((2, rr.ROW), dtype=torch.int32, device='cuda')
        bad, _ = rr.rr_support(t.text, t.text_len, takes, recs['l_seq'].astype(np.int64) + recs['span'], [0, 1], [5950, 10990], contig, d)
        assert bad == -1
        d = d.cpu().numpy()
    want = np.zeros((2, rr.ROW), dtype=np.int32)
    want[0, 5980 - 5950:5983 - 5950] = 1            # chunk_start - 20 is inside the region, chunk_start - 21 is not
    want[1, 11020 - 10990:11023 - 10990] = 1        # chunk_end + 20 is inside, chunk_end + 21 is not
    assert np.array_equal(d, want)


def test_assignment_on_many_reads(rr):
    """ties go to the first window, no overlap and a start above the last window's end to none; 700 reads cross the 256-read steps of
    the compaction, whose lists keep the member order"""
    rng = random.Random(5)
    splits = [[(100, 200), (300, 400)], [], [(0, 50)], [(150, 350), (351, 360), (500, 1500)]]
    reads = [(150, 350), (150, 250), (250, 350), (200, 300), (401, 500), (400, 500), (0, 1000), (120, 130), (50, 100)]
    reads += [(a, a + rng.randrange(1, 300)) for a in (rng.randrange(0, 1600) for _ in range(700))]
    got = rr.rr_assign([r[0] for r in reads], [r[1] for r in reads], splits)
    for s, windows in enumerate(splits):
        want = [[] for _ in windows]
        for k, r in enumerate(reads):
            if windows and r[0] <= max(w[1] for w in windows):
                w = ref.best_window(r[0], r[1], windows)
                if w is not None:
                    want[w].append(k)
        assert [g.tolist() for g in got[s]] == want, s
    assert got[0][0].tolist()[:4] == [0, 1, 6, 7] and 2 in got[0][1].tolist()
