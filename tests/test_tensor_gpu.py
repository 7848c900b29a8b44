"""GPU tests (-m gpu) of the tensor kernels on their own, through the native calls of include/mpn_tensor.h, against the restatement
(tests/tensor_ref.py): the join, the centre flags, the fill and the emission, at the smallest shapes at which they can go wrong --
operations on both sides of the 64 a wave takes per step, ranges of records on both sides of a ballot, tensors of 100 reads and of
one, numbers of one, two and three digits."""
import io
import random

import numpy as np
import pytest

import pileup_cases as pc
import tensor_cases as tc
import tensor_ref as ref

pytestmark = pytest.mark.gpu
CTG = 'c'


class Resident:
    """A BAM made of SAM lines: its text on the device, its records as the restatement reads them, and the reference bytes there."""

    def __init__(self, tmp_path, ctg, lines):
        import torch
        from megapath_nano_amd import clair_tensor
        path = pc.write_bam(tmp_path / 'in.bam', [(CTG, ctg)], lines)
        raw = pc.text_of(path)
        self.ctg, self.recs, self.text_len = ctg, ref.records(raw), len(raw)
        self.text = torch.from_numpy(np.frombuffer(raw + bytes(-len(raw) % 16), dtype=np.uint8).copy()).cuda()
        self.d_ref = torch.from_numpy(np.frombuffer(ctg.encode(), dtype=np.uint8).copy()).cuda()
        self.reads = np.zeros(len(self.recs), dtype=clair_tensor.TENSOR_READ)
        self.reads['off'] = [r['off'] for r in self.recs]
        self.reads['pos'] = [r['pos'] for r in self.recs]
        self.reads['reverse'] = [r['reverse'] for r in self.recs]
        self.pos, self.span = [r['pos'] for r in self.recs], [r['span'] for r in self.recs]

    def join(self, centres, left=True, ranges=None):
        from megapath_nano_amd import clair_tensor
        begin, end = ranges if ranges is not None else clair_tensor.join_ranges(self.pos, self.span, centres, left)
        return clair_tensor.tensor_join(self.pos, self.span, centres, begin, end, left)[:3]


def many_ops(n_before, inside):
    """a CIGAR of n_before operations over 2 * (n_before // 2) + (n_before & 1) reference positions (1M and 1I in turn) and then
    `inside`"""
    return ''.join('1M' if k % 2 == 0 else '1I' for k in range(n_before)) + inside


def read(rng, ctg, name, pos0, cigar, flag=0, qual=None):
    seq = pc.read_for(rng, ctg, pos0, cigar)
    return tc.sam_line(name, flag, CTG, pos0 + 1, 60, cigar, seq, qual)


@pytest.mark.parametrize('n_before', [0, 63, 64, 65, 129])
def test_fill_operations_before_the_window(libmpn, tmp_path, n_before):
    from megapath_nano_amd import clair_tensor
    rng = random.Random(n_before)
    ctg = pc.random_contig(rng, 600)
    c0 = 300
    m_before = (n_before + 1) // 2                         # reference positions the operations before the window take
    lines = []
    for k, inside in enumerate(['40M', '3M2I5M3D20M', '2I10M1D1I20M', '1D30M', ''.join('1M1D1M1I' for _ in range(12))]):
        # the window's first position is the first position of `inside`, one before it, and one behind it
        for shift in (0, -1, 1):
            lines.append((c0 - 16 - m_before + shift, read(rng, ctg, f'r{k}.{shift}', c0 - 16 - m_before + shift, many_ops(n_before, inside), 16 * (k & 1))))
    lines = [l for _, l in sorted(lines, key=lambda x: x[0])]
    R = Resident(tmp_path, ctg, lines)
    for left in (True, False):
        counts, off, pairs = R.join([c0], left)
        joined = [r for r in R.recs if ref.joins(r, c0, left)]
        assert int(counts[0]) == len(joined) > 3
        jobs = np.array([(0, c0, len(joined), 0, 0)], dtype=clair_tensor.TENSOR_JOB)
        block, depth, bad = clair_tensor.tensor_fill(R.text, R.text_len, R.reads, pairs, None, jobs, R.d_ref, 0, left)
        want = ref.fill(joined, c0, left, ctg, 0)
        assert bad == -1 and np.array_equal(block.cpu().numpy().reshape(33, 8, 4), want)
        assert int(depth[0]) == int(want[16, :, 0].sum())
        assert want[:, :, 1].sum() > want[:, :, 0].sum() > 0 and want[:, :, 2].sum() > want[:, :, 0].sum()      # insertions and deletions count


def test_fill_a_window_cut_by_a_step(libmpn, tmp_path):
    """the operations inside the window lie on both sides of the 64th, and of the 128th, operation"""
    from megapath_nano_amd import clair_tensor
    rng = random.Random(7)
    ctg = pc.random_contig(rng, 600)
    c0 = 300
    lines = []
    for n_before in (50, 56, 60, 116, 120):
        pos0 = c0 - 16 - (n_before + 1) // 2 - 3
        lines.append((pos0, read(rng, ctg, f'r{n_before}', pos0, many_ops(n_before, ''.join('1M1I1M1D' for _ in range(14)) + '5M'), 16 if n_before & 4 else 0)))
    R = Resident(tmp_path, ctg, [l for _, l in sorted(lines, key=lambda x: x[0])])
    counts, off, pairs = R.join([c0])
    assert int(counts[0]) == 5
    jobs = np.array([(0, c0, 5, 0, 0)], dtype=clair_tensor.TENSOR_JOB)
    block, depth, bad = clair_tensor.tensor_fill(R.text, R.text_len, R.reads, pairs, None, jobs, R.d_ref, 0, True)
    assert bad == -1 and np.array_equal(block.cpu().numpy().reshape(33, 8, 4), ref.fill(R.recs, c0, True, ctg, 0))


def test_fill_100_reads_1_read_and_reads_that_add_nothing(libmpn, tmp_path):
    """through a selection array, in any order; twice, bit for bit"""
    from megapath_nano_amd import clair_tensor
    rng = random.Random(8)
    ctg = pc.random_contig(rng, 400)
    c0 = 200
    lines = [(p, read(rng, ctg, f'r{i}', p, rng.choice(['50M', '20M2I28M', '10M5D40M']), 16 * (i & 1)))
             for i, p in enumerate(sorted(rng.randrange(150, 200) for _ in range(130)))]
    lines += [(c0 + 17, read(rng, ctg, f'edge{i}', c0 + 17, '30M')) for i in range(3)]       # join at c0 + 17 only
    R = Resident(tmp_path, ctg, [l for _, l in lines])
    counts, off, pairs = R.join([c0, c0 + 40])
    assert counts.tolist() == [133, len([r for r in R.recs if ref.joins(r, c0 + 40, True)])]
    order = list(range(133))
    rng.shuffle(order)
    sel = order[:100] + [order[100]] + [130, 131, 132] + [int(off[1])]
    jobs = np.array([(0, c0, 100, 1, 0), (100, c0, 1, 1, 0), (101, c0, 3, 1, 0), (0, c0, 0, 1, 0), (104, c0 + 40, 1, 1, 0), (0, c0, 100, 0, 0)],
                    dtype=clair_tensor.TENSOR_JOB)
    first, depth, bad = clair_tensor.tensor_fill(R.text, R.text_len, R.reads, pairs, sel, jobs, R.d_ref, 0, True)
    again, depth2, _ = clair_tensor.tensor_fill(R.text, R.text_len, R.reads, pairs, sel, jobs, R.d_ref, 0, True)
    got = first.cpu().numpy().reshape(-1, 33, 8, 4)
    assert bad == -1 and np.array_equal(got, again.cpu().numpy().reshape(-1, 33, 8, 4)) and np.array_equal(depth, depth2)
    joined2 = [r for r in R.recs if ref.joins(r, c0 + 40, True)]
    want = [ref.fill([R.recs[i] for i in order[:100]], c0, True, ctg, 0), ref.fill([R.recs[order[100]]], c0, True, ctg, 0),
            np.zeros((33, 8, 4), dtype=np.int32), np.zeros((33, 8, 4), dtype=np.int32), ref.fill(joined2[:1], c0 + 40, True, ctg, 0),
            ref.fill(R.recs[:100], c0, True, ctg, 0)]
    for g, w, d in zip(got, want, depth):
        assert np.array_equal(g, w) and int(d) == int(w[16, :, 0].sum())
    assert want[0].max() > 9 and want[1].sum() > 0
    with pytest.raises(Exception, match='more than 100'):
        clair_tensor.tensor_fill(R.text, R.text_len, R.reads, pairs, None, np.array([(0, c0, 101, 0, 0)], dtype=clair_tensor.TENSOR_JOB), R.d_ref, 0, True)


@pytest.mark.parametrize('left', [True, False])
def test_join_ranges_of_0_1_64_and_65_records(libmpn, tmp_path, left):
    rng = random.Random(11)
    ctg = pc.random_contig(rng, 4000)
    lines, groups = [], [(500, 1), (1000, 64), (1500, 65), (2000, 130)]
    for c0, n in groups:
        for i in range(n):
            p = c0 - 60 + (i * 75) // n                 # some end before the window, some start inside it
            lines.append((p, read(rng, ctg, f'g{c0}.{i}', p, rng.choice(['30M', '44M', '80M', '20M30D20M']))))
    # a short read inside a range of long ones
    lines += [(2500, read(rng, ctg, 'long0', 2500, '300M')), (2510, read(rng, ctg, 'short', 2510, '5M')), (2520, read(rng, ctg, 'long1', 2520, '300M'))]
    R = Resident(tmp_path, ctg, [l for _, l in sorted(lines, key=lambda x: x[0])])
    centres = [100, 500, 1000, 1500, 2000, 2600, 2790, 3500]
    counts, off, pairs = R.join(centres, left)
    pairs = pairs.cpu().numpy()
    for k, c0 in enumerate(centres):
        want = [i for i, r in enumerate(R.recs) if ref.joins(r, c0, left)]
        assert pairs[off[k]:off[k + 1]].tolist() == want, c0
    names = [R.recs[i]['name'] for i in pairs[off[5]:off[6]]]
    assert names == ['long0', 'long1'] and counts[0] == 0 and counts[-1] == 0
    # the whole file as every centre's range gives the same lists
    n = len(R.recs)
    c2, o2, p2 = R.join(centres, left, (np.zeros(len(centres), dtype=np.int64), np.full(len(centres), n, dtype=np.int64)))
    assert np.array_equal(c2, counts) and np.array_equal(p2.cpu().numpy(), pairs)
    # ranges of exactly 0, 1, 64 and 65 records
    for width in (0, 1, 64, 65):
        b = np.array([10], dtype=np.int64)
        c3, o3, p3 = R.join([1000], left, (b, b + width))
        assert p3.cpu().numpy().tolist() == [i for i in range(10, 10 + width) if ref.joins(R.recs[i], 1000, left)]


def test_centre_flags(libmpn, tmp_path):
    from megapath_nano_amd import clair_tensor
    rng = random.Random(12)
    ctg = pc.random_contig(rng, 400)
    c0 = 200

    def q(at, ch, n=50):
        return ''.join(ch if i == at else 'I' for i in range(n))
    lines = [
        read(rng, ctg, 'q6', 180, '50M', qual=q(20, chr(33 + 6))), read(rng, ctg, 'q7', 180, '50M', qual=q(20, chr(33 + 7))),
        read(rng, ctg, 'q0', 180, '50M', qual=q(20, '!')), read(rng, ctg, 'next_low', 180, '50M', qual=q(21, '!')),
        read(rng, ctg, 'del', 180, '15M10D25M'), read(rng, ctg, 'ins_then_low', 180, '18M4I28M', qual=q(24, '#')),
        read(rng, ctg, 'clip_low', 180, '7S43M', qual=q(27, '#')), read(rng, ctg, 'no_qual', 180, '50M', qual='*'),
        read(rng, ctg, 'ends_before', 180, '20M'), read(rng, ctg, 'many_ops_low', 190, many_ops(20, '30M'), qual=q(20, '"')),
        read(rng, ctg, 'lead_del', 200, '3D30M'), read(rng, ctg, 'lead_match', 200, '30M'), read(rng, ctg, 'behind', 205, '30M'),
    ]
    R = Resident(tmp_path, ctg, lines)
    for left in (True, False):
        counts, off, pairs = R.join([c0], left)
        n = int(counts[0])
        flags, bad = clair_tensor.centre_flags(R.text, R.text_len, R.reads, pairs, np.arange(n), np.full(n, c0), left)
        joined = [r for r in R.recs if ref.joins(r, c0, left)]
        want = {r['name']: int(ref.high_quality(r, c0, left)) for r in joined}
        assert bad == -1 and dict(zip([r['name'] for r in joined], flags.tolist())) == want
        assert (want['q6'], want['q7'], want['q0'], want['del'], want['no_qual'], want['ends_before']) == (0, 1, 0, 1, 1, 0)
        if left:
            assert (want['lead_del'], want['lead_match'], want['behind'], want['many_ops_low']) == (0, 1, 0, 0)


def test_emit_digits_and_a_short_reference_string(libmpn):
    import torch
    from megapath_nano_amd import clair_tensor
    rng = np.random.default_rng(3)
    block = np.zeros((4, 1056), dtype=np.int32)
    block[0] = rng.integers(0, 10, 1056)
    block[1] = rng.integers(0, 1000, 1056)
    block[2] = np.arange(1056) % 101 + 90
    block[3, [0, 1055]] = [1234567, 2147483647]
    seq = b'ACGTNacgtn' * 10
    d_ref = torch.from_numpy(np.frombuffer(seq, dtype=np.uint8).copy()).cuda()
    lines = np.array([(2, 0, 33, 17), (0, 5, 33, 1000000), (1, 80, 20, 97), (3, 99, 1, 9), (1, 100, 0, 10), (0, 67, 33, 84)], dtype=clair_tensor.TENSOR_LINE)
    want = ''.join(ref.line('chr1_random', int(l['centre']), seq[int(l['ref_off']):int(l['ref_off']) + int(l['ref_n'])].decode(), block[int(l['tensor'])])
                   for l in lines)
    d_block = torch.from_numpy(block).cuda()
    out = io.BytesIO()
    assert clair_tensor.tensor_emit(d_block, lines, d_ref, 'chr1_random', out) == len(want)
    assert out.getvalue().decode() == want
    with pytest.raises(Exception, match='reference slice'):
        clair_tensor.tensor_emit(d_block, np.array([(0, 90, 33, 1)], dtype=clair_tensor.TENSOR_LINE), d_ref, 'c', io.BytesIO())


def test_emit_in_rounds(libmpn, monkeypatch):
    import torch
    from megapath_nano_amd import clair_tensor
    block = torch.arange(3 * 1056, dtype=torch.int32).reshape(3, 1056).cuda() % 257
    d_ref = torch.from_numpy(np.frombuffer(b'A' * 40, dtype=np.uint8).copy()).cuda()
    lines = np.array([(k % 3, 0, 33, 20 + k) for k in range(7)], dtype=clair_tensor.TENSOR_LINE)
    whole = io.BytesIO()
    clair_tensor.tensor_emit(block, lines, d_ref, 'c', whole)
    monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', '9000')          # two lines a round; a line alone is longer than 1 byte would allow
    cut = io.BytesIO()
    clair_tensor.tensor_emit(block, lines, d_ref, 'c', cut)
    assert cut.getvalue() == whole.getvalue() and whole.getvalue().count(b'\n') == 7
    host = block.cpu().numpy()
    assert whole.getvalue().decode() == ''.join(ref.line('c', 20 + k, 'A' * 33, host[k % 3]) for k in range(7))
