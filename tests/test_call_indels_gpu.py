"""GPU tests (-m gpu) of the pile-up look-ups (megapath_nano_amd/clair_call.py indel_events, csrc/clair_call_kernels.hip) against the
restatement (tests/clair_call_ref.py): the events of every site, integer-exact, in the order of first appearance."""
import os
import random

import numpy as np
import pytest

import clair_call_cases as cc
import clair_call_ref as ref
import pileup_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def call(libmpn):
    from megapath_nano_amd import clair_call
    return clair_call


def write(tmp_path, seq, lines, name='in.bam'):
    return pc.write_bam(os.path.join(str(tmp_path), name), [('other', 50), (cc.CTG, seq)], lines)


def expected(seq, lines, sites):
    reads = [ref.read_of(l) for l in lines]
    return [ref.events_of(ref.closed_sequences(reads, s), s, len(seq)) for s in sites]


@pytest.mark.parametrize('n_sites', [0, 1, 63, 64, 65, 257])
def test_site_counts(call, tmp_path, n_sites):
    seq = cc.contig(n=600)
    lines = cc.random_reads(21, 300, lo=40, hi=400, long_events=True)
    sites = sorted(random.Random(n_sites).sample(range(30, 500), n_sites))
    got = call.indel_events(write(tmp_path, seq, lines), cc.CTG, sites, len(seq))
    assert got.host() == expected(seq, lines, sites)
    assert n_sites < 63 or sum(len(e) for e in got.host()) > 20


@pytest.mark.parametrize('depth', [0, 1, 64, 65, 249, 250, 251, 300])
@pytest.mark.parametrize('starts', ['one', 'distinct', 'mixed'])
def test_reads_over_a_site(call, tmp_path, depth, starts):
    """the 250 rule: all reads sharing one start, each with its own, and mixed, with reads the flag filter drops between them"""
    rng = random.Random(depth)
    seq = cc.contig(n=900)
    lines = []
    for i in range(depth):
        pos0 = 100 if starts == 'one' else 100 + i if starts == 'distinct' else 100 + i // 40
        body = [('M', 400 - pos0), ('I', 1 + i % 3), ('M', 30)] if i % 2 else [('M', 400 - pos0), ('D', 1 + i % 4), ('M', 30)]
        lines.append(cc.line_of(rng, f'r{i}', 16 if i % 5 == 0 else 0, pos0, body))
        if i % 7 == 0:
            lines.append(cc.line_of(rng, f'f{i}', rng.choice([4, 256, 2048]), pos0, [('M', 400 - pos0), ('I', 9), ('M', 30)]))
    sites = [400, 401]
    got = call.indel_events(write(tmp_path, seq, lines), cc.CTG, sites, len(seq)).host()
    assert got == expected(seq, lines, sites)
    if depth >= 251 and starts == 'one':
        assert sum(e[2] for e in got[0]) == 250


def test_event_shapes(call, tmp_path):
    """lengths 1, 15, 16, 50 and 51, ties by first appearance, an insertion right after a deletion, pads, the event at the last
    operation of a 64-operation step and at the first of the next, more than 128 operations, reverse strands, a clipped deletion"""
    rng = random.Random(4)
    seq = cc.contig(n=700)
    lines = []
    for i, n in enumerate([1, 15, 16, 50, 51, 50, 16, 1]):
        lines.append(cc.line_of(rng, f'i{i}', 16 * (i % 2), 100, [('M', 100), ('I', n), ('M', 20)]))
        lines.append(cc.line_of(rng, f'd{i}', 16 * (i % 2), 100, [('M', 100), ('D', n), ('M', 20)]))
    lines.append(cc.line_of(rng, 'di', 0, 100, [('M', 98), ('D', 2), ('I', 3), ('M', 20)]))
    lines.append(cc.line_of(rng, 'pi', 0, 100, [('M', 100), ('P', 2), ('I', 3), ('M', 20)]))
    lines.append(cc.line_of(rng, 'ipi', 16, 100, [('M', 100), ('I', 1), ('P', 1), ('I', 2), ('M', 20)]))
    for edge in (63, 64, 65, 127, 128, 129):                 # the covering operation is number `edge`; the event is the next
        body = [('M', 1), ('I', 1)] * (edge // 2) + [('M', 100 - edge // 2)]
        lines.append(cc.line_of(rng, f'e{edge}', 0, 100, body + [('I', 4), ('M', 1)] * 40, soft=2 if edge % 2 else 0))
    end = len(seq)
    lines.append(cc.line_of(rng, 'clip', 0, end - 21, [('M', 20), ('D', 5), ('M', 3)]))
    lines.sort(key=lambda l: int(l.split('\t')[3]))
    sites = [199, 200, 201, 202, end - 1]
    got = call.indel_events(write(tmp_path, seq, lines), cc.CTG, sites, end).host()
    want = expected(seq, lines, sites)
    assert got == want
    assert {(e[0], e[1]) for e in want[1]} >= {(0, 1), (0, 15), (0, 16), (0, 50), (1, 1), (1, 50)} and all(e[1] <= 50 for e in want[1])
    assert want[4] == [(1, 5, 1, 0, 1, '')]


def test_a_second_text_group_and_twice_the_same(call, tmp_path, monkeypatch):
    seq = cc.contig(n=600)
    lines = cc.random_reads(33, 400, lo=40, hi=450, long_events=True)
    sites = list(range(60, 460, 3))
    bam_fn = write(tmp_path, seq, lines)
    a = call.indel_events(bam_fn, cc.CTG, sites, len(seq))
    b = call.indel_events(bam_fn, cc.CTG, sites, len(seq))
    assert a.events.cpu().numpy().tobytes() == b.events.cpu().numpy().tobytes() and a.bases.cpu().numpy().tobytes() == b.bases.cpu().numpy().tobytes()
    monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', '16384')
    c = call.indel_events(bam_fn, cc.CTG, sites, len(seq))
    assert c.host() == a.host() == expected(seq, lines, sites)


def test_an_insertion_directly_followed_by_a_deletion(call, tmp_path):
    case = cc.insdel_case()
    got = call.indel_events(write(tmp_path, case['seq'], case['lines']), cc.CTG, [100], len(case['seq'])).host()
    assert got == expected(case['seq'], case['lines'], [100]) and got[0][0][5].endswith('-2NN') and got[0][2][5] is None


def test_refusals(call, tmp_path):
    rng = random.Random(2)
    seq = cc.contig()
    bam_fn = write(tmp_path, seq, [cc.line_of(rng, 'insdel', 0, 80, [('M', 20), ('I', 2), ('D', 2), ('M', 20)])])
    with pytest.raises(ValueError, match='ascending'):
        call.indel_events(bam_fn, cc.CTG, [100, 90], len(seq))
    assert call.indel_events(bam_fn, cc.CTG, [100], len(seq)).host()[0][0][4] == 2          # the deletion behind the insertion
    assert call.indel_events(bam_fn, cc.CTG, [99], len(seq)).host() == [[]]
