"""fastx.nanosplit on the host against golden output files of the reference's own nanosplit binary, and the numpy statement of the
read split (mapper.host_split_reads) against a plain loop over dicts on every case of tests/split_cases.py -- with the proof,
from the plans themselves, that the cases reach the mechanisms the device kernels have."""
import gzip
import io
import json
import os

import numpy as np
import pytest

from megapath_nano_amd import fastx, mapper

import split_cases

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, 'golden', 'nanosplit_golden.json')))
CASES = split_cases.make_cases()


def _lay_out(case, d):
    for fn, text in case['files'].items():
        data = text.encode()
        with open(os.path.join(d, fn), 'wb') as f:
            f.write(gzip.compress(data) if fn in case['gz'] else data)
    with open(os.path.join(d, 'list.tsv'), 'w') as f:
        f.write(case['list'].replace('{dir}', d))
    return os.path.join(d, 'list.tsv'), [os.path.join(d, x) for x in case['inputs']]


@pytest.mark.parametrize('case', GOLD['cases'], ids=[c['name'] for c in GOLD['cases']])
def test_nanosplit_host_reproduces_the_reference_files(case, tmp_path):
    d = str(tmp_path)
    lst, inputs = _lay_out(case, d)
    before = set(os.listdir(d))
    written = fastx.nanosplit(lst, inputs, device=False)
    made = sorted(set(os.listdir(d)) - before)
    assert made == sorted(case['outputs'])                          # every listed file is created, the empty one too
    for fn in made:
        assert open(os.path.join(d, fn), 'rb').read() == case['outputs'][fn].encode('latin-1'), fn
    assert sorted(os.path.basename(p) for p, _ in written) == made
    counts = {os.path.basename(p): k for p, k in written}
    for fn in made:
        assert counts[fn] == len(list(fastx.iter_fastx_full(io.BytesIO(case['outputs'][fn].encode('latin-1')))))


def test_golden_cases_are_the_ones_promised():
    by = {c['name']: c for c in GOLD['cases']}
    a = by['fastq_and_fasta']
    assert a['outputs']['out_empty'] == ''                           # listed only for a name that does not occur
    assert a['list'].count('r2 {dir}/out_y') == 2 and a['outputs']['out_y'].count('@r2\n') == 1      # a pair twice, written once
    assert '@r1 ' in a['outputs']['out_x'] and '@r1 ' in a['outputs']['out_y']                        # a read in two files
    assert '@shared in_fastq' in a['outputs']['out_x'] and '>shared in_fasta' in a['outputs']['out_x']   # a name in two inputs
    assert '@r3 empty\n\n+\n\n' in a['outputs']['out_x']               # an empty sequence
    assert not a['list'].endswith('\n')                                # the last line has no newline
    assert 'ACGTACGTACGTACGTACGTTTTTTTTTTTTTTTTTTTTTGG' in a['outputs']['out_z']   # multi-line FASTA on one line
    assert by['gzip_and_repeat']['gz'] and by['gzip_and_repeat']['outputs']['odd'].count('@z3 ') == 2
    assert by['fasta_then_fastq']['outputs']['s'].startswith('>shared')


def test_malformed_list_line_is_an_error(tmp_path):
    lst = tmp_path / 'list.tsv'
    lst.write_text(f'r1\t{tmp_path}/a\nlonely\n')
    fq = tmp_path / 'x.fq'
    fq.write_text('@r1\nA\n+\n!\n')
    with pytest.raises(ValueError, match='list.tsv:2'):
        fastx.nanosplit(str(lst), [str(fq)], device=False)


@pytest.mark.parametrize('i', range(len(CASES)), ids=[c['name'] for c in CASES])
def test_host_split_equals_the_loop_over_dicts(i):
    split_cases.assert_same(split_cases.expected(i), split_cases.restate(CASES[i]), CASES[i]['name'])


def test_host_split_validates():
    c = CASES[0]
    for kw in (dict(mem_read=[len(c['lens'])], mem_group=[0]), dict(mem_read=[-1], mem_group=[0]), dict(mem_read=[0], mem_group=[1]),
               dict(mem_read=[0], mem_group=[-1])):
        with pytest.raises(ValueError):
            mapper.host_split_plan(c['lens'], kw['mem_read'], kw['mem_group'], 1)
    with pytest.raises(ValueError):
        mapper.host_split_plan([3, -1], [0], [0], 1)


def test_layout_rules_hold_on_every_case():
    for i, c in enumerate(CASES):
        e = split_cases.expected(i)
        assert (e['group_byte'] % 16 == 0).all() and e['out_bytes'] % 16 == 0, c['name']
        ends = e['out_off'] + c['lens'][e['out_read']]
        assert (ends + 4 <= e['out_bytes']).all(), c['name']          # 4 readable bytes behind the last base of every group
        for g in range(c['n_groups']):
            lo, hi = e['group_first'][g], e['group_first'][g + 1]
            assert (np.diff(e['out_read'][lo:hi]) > 0).all(), (c['name'], g)      # input order, a read once
            if hi > lo:
                assert e['out_off'][lo] == e['group_byte'][g]
                assert (e['out_off'][lo + 1:hi] == ends[lo:hi - 1]).all()         # back to back
                assert ends[hi - 1] <= e['group_byte'][g + 1]


def test_cases_reach_the_mechanisms():
    """From the plans: what the device kernels do differently is met by some case."""
    pair4, src16, dst16, shift16 = set(), set(), set(), set()
    padded = unpadded = collapsed = empty_group = read_in_every_group = spans_chunks = short_only_slots = False
    slow_tail_at_source_end = second_round = zero_len_placed = False
    for i, c in enumerate(CASES):
        e = split_cases.expected(i)
        src, dst, ln = c['off'][e['out_read']], e['out_off'], c['lens'][e['out_read']].astype(np.int64)
        moved = ln > 0
        pair4 |= set(zip((src[moved] % 4).tolist(), (dst[moved] % 4).tolist()))
        src16 |= set((src[moved] % 16).tolist())
        dst16 |= set((dst[moved] % 16).tolist())
        shift16 |= set(((src - dst)[ln >= 32] % 16).tolist())         # (32 bytes hold a whole 16-byte slot: the vector path)
        sizes = np.array([int(ln[e['group_first'][g]:e['group_first'][g + 1]].sum()) for g in range(c['n_groups'])], dtype=np.int64)
        if c['n_groups'] > 1:
            inner = sizes[:-1][sizes[:-1] > 0]
            padded |= bool((inner % 16 != 0).any())
            unpadded |= bool((inner % 16 == 0).any())
        distinct = len(set(zip(c['mem_read'].tolist(), c['mem_group'].tolist())))
        collapsed |= distinct < len(c['mem_read'])
        assert distinct == e['n_out']
        counts = np.diff(e['group_first'])
        empty_group |= bool((counts == 0).any()) and bool((counts > 0).any())
        if len(c['lens']) and c['n_groups'] > 1:
            read_in_every_group |= any((e['out_read'] == r).sum() == c['n_groups'] for r in range(len(c['lens'])))
        spans_chunks |= bool((ln > 64 * 1024).any())                   # a read over more than 64 wave steps
        short_only_slots |= bool(((ln > 0) & (ln < 16)).any())
        zero_len_placed |= bool((ln == 0).any())
        src_end = int((c['off'] + c['lens']).max()) if len(c['lens']) else 0
        if len(c['buf']) == src_end and len(ln):
            # the last whole 16-byte slot of a read that ends where the source ends: when its second aligned source vector would pass
            # the source's end (rounded up to 4) the byte path has to take it
            for j in np.flatnonzero((src + ln == src_end) & (ln >= 32)):
                slot = (dst[j] + ln[j]) // 16 * 16 - 16
                s = src[j] + slot - dst[j]
                slow_tail_at_source_end |= bool(slot >= dst[j] and s % 16 != 0 and s - s % 16 + 32 > -(-src_end // 4) * 4)
        second_round |= e['out_bytes'] > 2048 * 4 * 1024
    assert pair4 == {(a, b) for a in range(4) for b in range(4)}, sorted(pair4)
    assert src16 == set(range(16)) and dst16 == set(range(16)) and shift16 == set(range(16))
    assert padded and unpadded and collapsed and empty_group and read_in_every_group
    assert spans_chunks and short_only_slots and zero_len_placed and slow_tail_at_source_end and second_round
    # pairs in reverse and in shuffled order
    assert any(len(c['mem_read']) > 1 and (np.diff(c['mem_group'].astype(np.int64) << 32 | c['mem_read']) < 0).all() for c in CASES)
    assert any(len(c['mem_read']) > 2 and len(set(np.sign(np.diff(c['mem_group'].astype(np.int64) << 32 | c['mem_read'])).tolist())) == 3 for c in CASES)
    assert any(len(c['mem_read']) == 0 and len(c['lens']) > 0 for c in CASES) and any(len(c['lens']) == 0 for c in CASES)
    assert {c['n_groups'] for c in CASES} >= {1, 2, 1000}
    assert any(c['qbuf'] is not None for c in CASES) and any(c['qbuf'] is None and len(c['lens']) for c in CASES)


def test_split_reads_groups_are_views_with_names_and_qualities():
    names = [f'r{i}' for i in range(6)]
    seqs = [b'ACGTACGTACGTACGTACGTA', b'', b'GG', b'TTTTTTTTTTTTTTTTT', b'C', b'NNNN']
    quals = [bytes([40 + i]) * len(s) for i, s in enumerate(seqs)]
    packed = mapper.PackedReads(names, seqs, quals=quals)
    sp = mapper.split_reads(packed, [5, 0, 3, 0, 1, 2], [1, 1, 0, 0, 1, 3], 4, device=False)
    want = {0: [0, 3], 1: [0, 1, 5], 2: [], 3: [2]}
    for g, reads in want.items():
        p = sp.group(g)
        assert p.n == len(reads) == sp.n_reads(g) and p.names == [names[r] for r in reads] and p.dev is None
        assert [p.seq(i).tobytes() for i in range(p.n)] == [seqs[r] for r in reads]
        assert [p.qbuf[p.off[i]:p.off[i] + p.lens[i]].tobytes() for i in range(p.n)] == [quals[r] for r in reads]
        assert p.buf.base is not None and np.shares_memory(p.buf, sp.res['seqs'])      # a view of the one output buffer
        assert len(p.buf) >= p.bases + 4 and (p.off[:1] == 0).all()
    plain = mapper.split_reads(mapper.PackedReads(names, seqs), [0], [0], 1, device=False).group(0)
    assert plain.qbuf is None and plain.names == ['r0']
