"""GPU tests (-m gpu) of the pile-up kernels (include/mpn_pileup.h): the per-record table of mpn_pileup_records, the counters of
mpn_pileup_counts and the table of mpn_pileup_candidates against the restatement tests/pileup_ref.py on constructed BAMs, at the
smallest shapes where the kernels can go wrong (tile edges, CIGAR lengths around the 64 operations of a wave step, every alignment
of the packed bases, the record-slice split), and candidates.pileup() end to end across BGZF groups and contigs.  The malformed
records have been through the host build of the same arithmetic under the sanitizers (tests/test_pileup_host.py)."""
import io
import random

import numpy as np
import pytest

import pileup_cases as pc
import pileup_ref as ref

pytestmark = pytest.mark.gpu
TILE = 2048


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    monkeypatch.delenv('MPN_INGEST_BATCH_BYTES', raising=False)
    monkeypatch.delenv('MPN_BAM_WALK_RECORDS', raising=False)


def upload(data):
    import torch
    buf = np.zeros(max((len(data) + 15) & ~15, 16), dtype=np.uint8)
    buf[:len(data)] = np.frombuffer(data, dtype=np.uint8)
    return torch.from_numpy(buf).cuda()


class Resident:
    """A BAM text in HBM, its records restated, and the per-record table of the device checked against the restatement."""

    def __init__(self, text, tid=0):
        from megapath_nano_amd import candidates, ingest
        self.text, self.d_text = text, upload(text)
        self.recs = ref.records(text)
        rows = np.zeros(len(self.recs), dtype=ingest.BAM_ROW)
        rows['off'] = [r['off'] for r in self.recs]
        rows['l_seq'] = [len(r['codes']) for r in self.recs]
        rows['flag'] = [r['flag'] for r in self.recs]
        rows['l_read_name'] = [len(r['name']) + 1 for r in self.recs]
        self.table = candidates.pileup_records(self.d_text, len(text), rows)
        for r, g in zip(self.recs, self.table):
            assert (int(g['status']), int(g['soft']), int(g['total']), int(g['span'])) == ref.summary(r), r['name']
            assert (int(g['ref_id']), int(g['pos']), int(g['n_cigar']), int(g['mapq'])) == (r['ref_id'], r['pos'], len(r['ops']), r['mapq']), r['name']
        # taken: every record of the contig, in file order (the 0.55 test is the Python layer's), leading indels by the first-of-POS rule
        self.taken, last = [], None
        for k, r in enumerate(self.recs):
            if r['ref_id'] == tid:
                self.taken.append((k, last is None or r['pos'] > last))
                last = r['pos']

    def device(self, lo, hi, slice_records=0):
        import torch
        from megapath_nano_amd import candidates
        takes = np.zeros(len(self.taken), dtype=candidates.PILE_TAKE)
        takes['off'] = [self.recs[k]['off'] for k, _ in self.taken]
        takes['pos'] = [self.recs[k]['pos'] for k, _ in self.taken]
        takes['lead'] = [int(lead) for _, lead in self.taken]
        counts = torch.zeros((hi - lo, 7), dtype=torch.int32, device='cuda')
        bad, sliced = candidates.pileup_counts(self.d_text, len(self.text), takes, self.table['span'][[k for k, _ in self.taken]], lo, hi, counts, slice_records)
        assert bad == -1
        return counts, sliced

    def pile(self):
        pile = {}
        for k, lead in self.taken:
            ref.add_record(pile, self.recs[k], lead)
        return pile

    def want(self, lo, hi):
        out = np.zeros((max(hi - lo, 0), 7), dtype=np.int32)
        for p, c in self.pile().items():
            if lo <= p < hi:
                out[p - lo] = c
        return out


PATTERN = ['5M', '1I', '3=', '2D', '1X', '3N', '2M', '1P', '2I', '40M']


def cigar_of(n_ops):
    return ''.join(PATTERN[k % len(PATTERN)] for k in range(n_ops))


@pytest.fixture(scope='module')
def geometry(libmpn, tmp_path_factory):
    """a contig of three tiles plus one position, and reads at its edges"""
    rng = random.Random(20)
    n = 3 * TILE + 1
    ctg = pc.random_contig(rng, n)
    reads = [(2047, '2050M', 'span'),                 # from the last position of tile 0 to the first of tile 2
             (2040, '8M2I10M', 'ins_prev'),           # the insertion stands at 2048 and counts at 2047, in the tile before
             (2048, '3D10M', 'lead_del_a'),           # a leading deletion at 2047: counts for the first record of its POS only
             (2048, '3D10M', 'lead_del_b'),
             (4090, '6M4D10M', 'del_prev'),           # the deletion starts at 4096 and counts at 4095
             (0, '2I5M', 'before_zero'),              # position -1 does not exist
             (500, '30S1M', 'all_clip'),
             (6100, '45M', 'to_the_end'),             # ends on the last position
             (6140, '10M', 'overhang')]               # five bases past the end
    for k, (n_ops, pos) in enumerate(((1, 100), (63, 1900), (64, 1950), (65, 2000), (200, 3000))):
        reads.append((pos, cigar_of(n_ops), f'ops{n_ops}'))
    # odd and even l_seq behind names of many lengths, until the packed bases start at every offset modulo 16 (all seeded: the
    # same file every time)
    for v in range(1, 40):
        packed = [(600 + 3 * k, f'{32 + k}M', 'n' * (1 + (k * k * v) % 29)) for k in range(1, 49)]
        every, rr = sorted(reads + packed, key=lambda r: r[0]), random.Random(21)
        lines = [pc.sam_line(name, 0, 'c', pos + 1, 60, cg, pc.read_for(rr, ctg, pos, cg)) for pos, cg, name in every]
        path = pc.write_bam(tmp_path_factory.mktemp('geometry') / 'g.bam', [('c', ctg)], lines)
        text = pc.text_of(path)
        if {(r['off'] + 36 + len(r['name']) + 1 + 4 * len(r['ops'])) % 16 for r in ref.records(text)} == set(range(16)):
            break
    else:
        raise AssertionError('no read set puts the packed bases at every offset modulo 16')
    res = Resident(text)
    assert {len(r['ops']) for r in res.recs} >= {1, 63, 64, 65, 200}
    return res, ctg, path


WINDOWS = [(0, 3 * TILE + 1), (2100, 2500), (2048, 4097), (2047, 2049), (300, 300), (5400, 5900), (6144, 6145), (1, 4096)]


@pytest.mark.parametrize('lo,hi', WINDOWS)
def test_counts_at_the_tile_edges(geometry, lo, hi):
    res, ctg, _ = geometry
    counts, sliced = res.device(lo, hi)
    want = res.want(lo, hi)
    assert np.array_equal(counts.cpu().numpy(), want)
    assert sliced == 0
    if (lo, hi) == (5400, 5900):
        assert want.sum() == 0                         # a window without records
    if (lo, hi) == (2048, 4097):
        pile = res.pile()
        assert pile[2047][4] == 1 and pile[2047][5] == 1     # the indels at lo - 1 exist, and are outside
    if (lo, hi) == (0, 3 * TILE + 1):
        assert want[2047, 4] == 1 and want[2047, 5] == 1 and want[4095, 5] == 1 and want[6144].sum() == 2


def test_a_small_slice_splits_the_tiles_and_adds_the_same(geometry):
    res, _, _ = geometry
    lo, hi = 0, 3 * TILE + 1
    counts, sliced = res.device(lo, hi, slice_records=3)
    assert sliced >= 1
    assert np.array_equal(counts.cpu().numpy(), res.want(lo, hi))


@pytest.mark.parametrize('lo,hi,bed,cov,thr', [(0, 3 * TILE + 1, None, 1.0, 0.125), (600, 2300, [(0, 650), (700, 701), (2040, 5000)], 2.5, 0.2),
                                                (2048, 4097, None, 1.0, 0.5), (300, 300, None, 4.0, 0.125)])
def test_candidate_table(geometry, lo, hi, bed, cov, thr):
    from megapath_nano_amd import candidates
    res, ctg, _ = geometry
    counts, _ = res.device(lo, hi)
    refb = np.frombuffer(ctg.encode(), dtype=np.uint8)[lo:hi]
    b = None if bed is None else (np.array([s for s, _ in bed]), np.array([e for _, e in bed]))
    rows = candidates.pileup_candidates(counts, lo, refb, b, cov, thr)
    pile = {p: c for p, c in res.pile().items() if lo <= p < hi}
    want = ref.candidates(pile, ctg, None, None, thr, cov, bed)
    got = [(int(r['pos']), chr(r['ref_base']), int(r['depth']), list(zip(r['label'].tobytes().decode(), r['count'].tolist()))) for r in rows]
    assert got == [(p, rb, d, [(l, c) for l, c in order]) for p, rb, d, order in want]
    if hi - lo > 1000 and bed is None:
        assert len(got) > 20


def test_many_candidates_come_back_in_order(libmpn):
    """more rows than the first capacity of the Python layer, over many blocks of the scan"""
    import torch
    from megapath_nano_amd import candidates
    n = 150_001
    rng = np.random.default_rng(5)
    counts = rng.integers(0, 9, size=(n, 7)).astype(np.int32)
    refb = np.frombuffer(b'ACGTNacgtRYU*', dtype=np.uint8)[rng.integers(0, 13, size=n)]
    rows = candidates.pileup_candidates(torch.from_numpy(counts).cuda(), 1000, refb, None, 4.0, 0.2)
    pile = {1000 + i: c for i, c in enumerate(counts.tolist())}
    want = ref.candidates(pile, '?' * 1000 + refb.tobytes().decode(), None, None, 0.2, 4.0)
    assert len(want) > (1 << 16)
    assert rows['pos'].tolist() == [w[0] for w in want]
    assert rows['depth'].tolist() == [w[2] for w in want]
    assert rows['count'].tolist() == [[c for _, c in w[3]] for w in want]
    assert rows['label'].tobytes().decode() == ''.join(l for w in want for l, _ in w[3])


def test_3000_reads_on_one_tile_twice(libmpn, tmp_path):
    rng = random.Random(30)
    ctg = pc.random_contig(rng, TILE)
    starts = sorted(rng.randrange(0, TILE - 70) for _ in range(3000))
    lines = []
    for k, s in enumerate(starts):
        cg = '20M2I10M1D29M' if k % 3 == 0 else '60M'
        lines.append(pc.sam_line(f'r{k}', 0, 'c', s + 1, 60, cg, pc.read_for(rng, ctg, s, cg)))
    res = Resident(pc.text_of(pc.write_bam(tmp_path / 'deep.bam', [('c', ctg)], lines)))
    a, sliced = res.device(0, TILE)
    b, _ = res.device(0, TILE)
    assert sliced == 1                                  # 3000 records > MPN_PILEUP_SLICE: the slices add with atomics
    want = res.want(0, TILE)
    assert np.array_equal(a.cpu().numpy(), want) and np.array_equal(b.cpu().numpy(), want)
    assert want[:, :4].sum() > 170_000


def test_contigs_interleaved_at_the_boundary(libmpn, tmp_path):
    from megapath_nano_amd import candidates
    rng = random.Random(40)
    c1, c2 = pc.random_contig(rng, 3000), pc.random_contig(rng, 2500)
    one = [(p, 'c1', c1) for p in (10, 700, 1500, 2800, 2900, 2950)]
    two = [(p, 'c2', c2) for p in (0, 5, 40, 900, 2400)]
    order = one[:4] + [two[0], one[4], two[1], one[5]] + two[2:]          # the records of the two contigs mixed where one ends
    lines = [pc.sam_line(f'{nm}_{p}', 0, nm, p + 1, 60, '30M1I20M2D10M', pc.read_for(rng, c, p, '30M1I20M2D10M')) for p, nm, c in order]
    path = pc.write_bam(tmp_path / 'two.bam', [('c1', c1), ('c2', c2)], lines)
    text = pc.text_of(path)
    for nm, c in (('c1', c1), ('c2', c2)):
        p = candidates.pileup(path, nm)
        assert (p.lo, p.hi, p.n_records) == (0, len(c), len(lines))
        assert p.n_taken == sum(1 for _, n, _ in order if n == nm)
        assert np.array_equal(p.counts.cpu().numpy(), ref.counts_array(text, nm, 0, len(c)))
    assert candidates.pileup(path, 'c3').n_taken == 0


@pytest.fixture(scope='module')
def ont(libmpn, tmp_path_factory):
    """seeded random reads at 40x over 10 kb with the ONT error mix"""
    rng = random.Random(50)
    ctg = pc.random_contig(rng, 10_000)
    lines = pc.ont_reads(51, ('amp', ctg), 40, 1000)
    d = tmp_path_factory.mktemp('ont')
    path = pc.write_bam(d / 'ont.bam', [('amp', ctg)], lines)
    fa = pc.write_fasta(d / 'amp.fa', [('amp', ctg)])
    return path, fa, ctg, pc.text_of(path)


def test_random_ont_reads_and_group_boundaries(ont, monkeypatch):
    from megapath_nano_amd import candidates
    path, _, ctg, text = ont
    want = ref.counts_array(text, 'amp', 0, len(ctg), 20)
    whole = candidates.pileup(path, 'amp', min_mq=20)
    assert np.array_equal(whole.counts.cpu().numpy(), want)
    assert 0 < whole.n_taken < whole.n_records and want[:, 4].sum() > 1000 and want[:, 5].sum() > 1000
    # records that straddle the groups of BGZF blocks, walked seven at a time
    monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', '70000')
    monkeypatch.setenv('MPN_BAM_WALK_RECORDS', '7')
    timings = {}
    cut = candidates.pileup(path, 'amp', min_mq=20, timings=timings)
    assert len(text) > 4 * 70000 and timings['walk_device_ms'] > 0
    assert np.array_equal(cut.counts.cpu().numpy(), want) and cut.n_taken == whole.n_taken
    part = candidates.pileup(path, 'amp', 2001, 2300, min_mq=20)
    assert (part.lo, part.hi) == (2000, 2300)
    assert np.array_equal(part.counts.cpu().numpy(), want[2000:2300])


def test_random_ont_reads_to_lines(ont):
    from megapath_nano_amd import candidates
    path, fa, ctg, text = ont
    out = io.BytesIO()
    n = candidates.extract_variant_candidates(path, fa, 'amp', threshold=0.2, min_coverage=4, min_mq=0, out=out)
    want = ref.lines('amp', ref.candidates(ref.counts(text, 'amp', 0), ctg, None, None, 0.2, 4))
    assert out.getvalue().decode() == want and n == want.count('\n') > 10
